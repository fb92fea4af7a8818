"""tt_ga_breed_guided against tt_ga_breed and against the local search that
follows a breed in a generation, on comp01 and on med, 8,192 members and 8,192
children:

    python tools/bench_cx.py [--configs comp01,med] [--rows 8192] [--repeats 5]
                             [--out FILE] [--lib LIBRARY]

Two regimes of members: "random" (tt_random_init + tt_local_search_eval(200):
none feasible) and "greedy" (tt_greedy_init + tt_local_search_eval(1000): mostly
feasible, as in tools/bench_lahc.py). Per instance and regime, in one process
and alternating, each call between device events on restored buffers and
streams, `repeats` times over after a warm-up round:

  breed_uniform / breed_guided / breed_guided_repair
      tt_ga_breed, tt_ga_breed_guided with repair 0 and 1 (p_cross 0.8,
      p_mut 0.5, the discarded draws included), from the same members and streams
  search_uniform / search_guided / search_guided_repair
      tt_local_search_eval(1000) on each of the three sets of children

One JSON line goes to stdout and to profiles/cx_bench.json (--out): per call
the median us with the lowest and highest repeat; per set of children the mean
hcv before the search, crossed / clean / meanCost / repaired (guided sets), the
phase-2 share of the search's steps and the share feasible after it; and the
ratios breed over search. The one failing exit (1) is the sanity bound: the
guided breed with repair takes longer than the search of the uniform children
in the same regime. Every other ratio is recorded, not gated. Needs a GPU:
there is no CPU path."""
import argparse
import json
import pathlib
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "timetabling-ga-mpi-openmp_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ttga  # noqa: E402
from ttga import native  # noqa: E402

SEARCH_STEPS = 1000
KINDS = ("uniform", "guided", "guided_repair")


def members(dp, P, regime):
    """(slot, room, penalty, feasible share): P members of the regime."""
    rng = torch.from_numpy(ttga.population_seeds(5000, P)).cuda()
    slot = torch.empty((P, dp.E), dtype=torch.uint8, device="cuda")
    room = torch.empty_like(slot)
    out = tuple(torch.empty(P, dtype=d, device="cuda") for d in (torch.int32, torch.int32, torch.uint8, torch.int32))
    if regime == "greedy":
        dp.greedy_init(rng, slot, room)
        dp.local_search(slot, room, rng, 1000, out=out)
    else:
        dp.random_init(rng, slot, room)
        dp.local_search(slot, room, rng, 200, out=out)
    return slot, room, out[3], float(out[2].float().mean())


def bench(config, P, regime, repeats):
    inst = ttga.config_instance(config)
    dp = native.DeviceProblem(inst)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    pop_slot, pop_room, pop_pen, pop_feasible = members(dp, P, regime)
    seeds = torch.from_numpy(ttga.population_seeds(7000, P)).cuda()
    i32 = lambda: torch.zeros(P, dtype=torch.int32, device=dev)                    # noqa: E731
    slot = torch.empty((P, dp.E), dtype=torch.uint8, device=dev)
    room, rng, flags = torch.empty_like(slot), seeds.clone(), torch.zeros(P, dtype=torch.uint8, device=dev)
    cost, repaired = i32(), i32()
    out = (i32(), i32(), torch.empty(P, dtype=torch.uint8, device=dev), i32())     # hcv, scv, feasible, penalty

    def breed(kind):
        if kind == "uniform":
            return lambda: dp.ga_breed(pop_slot, pop_room, pop_pen, rng, slot, room, flags, 0.8, 0.5, True)
        return lambda: dp.ga_breed_guided(pop_slot, pop_room, pop_pen, rng, slot, room, flags, 0.8, 0.5, True,
                                          repair=kind == "guided_repair", cost=cost, repaired=repaired)

    # the three sets of children, bred once: what the searches are restored to
    saved, sets = {}, {}
    for kind in KINDS:
        rng.copy_(seeds)
        breed(kind)()
        saved[kind] = (slot.clone(), room.clone(), rng.clone())
        hcv = dp.eval(slot, room)[0]
        crossed = (flags & 1) != 0
        sets[kind] = {"mean_hcv_before_search": float(hcv.float().mean()), "crossed": int(crossed.sum())}
        if kind != "uniform":
            n = max(1, int(crossed.sum()))
            sets[kind].update(clean=int((crossed & (cost == 0)).sum()), meanCost=float(cost.sum()) / n,
                              repaired=int(repaired.sum()))

    def restore_breed():
        rng.copy_(seeds)

    def restore_search(kind):
        def f():
            s, r, g = saved[kind]
            slot.copy_(s)
            room.copy_(r)
            rng.copy_(g)
        return f
    search = lambda: dp.local_search(slot, room, rng, SEARCH_STEPS, out=out)       # noqa: E731
    calls = {}
    for kind in KINDS:
        calls["breed_" + kind] = (restore_breed, breed(kind))
    for kind in KINDS:
        calls["search_" + kind] = (restore_search(kind), search)

    def timed(fn):
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record(st)
        fn()
        e.record(st)
        e.synchronize()
        return b.elapsed_time(e)

    times = {k: [] for k in calls}
    for rep in range(repeats + 1):                # round 0 warms up: code objects, the allocator, clocks
        for k, (restore, fn) in calls.items():
            restore()
            t = timed(fn)
            if rep:
                times[k].append(t)
            if rep == repeats and k.startswith("search_"):
                ph2, steps = dp.local_search_stats()
                sets[k[len("search_"):]].update(ls_phase2_step_share=ph2 / steps if steps else None,
                                                feasible_after_search=float(out[2].float().mean()))
    if dp.status() != 0:
        raise SystemExit(f"bench_cx: device status {dp.status()}")
    us = {k: {"median": 1e3 * float(np.median(v)), "min": 1e3 * float(min(v)), "max": 1e3 * float(max(v))}
          for k, v in times.items()}
    med = lambda k: us[k]["median"]                                                 # noqa: E731
    ratios = {"guided_repair_breed_over_uniform_search": med("breed_guided_repair") / med("search_uniform"),
              "guided_breed_over_uniform_breed": med("breed_guided") / med("breed_uniform"),
              "guided_repair_breed_over_uniform_breed": med("breed_guided_repair") / med("breed_uniform"),
              "guided_generation_over_uniform": (med("breed_guided") + med("search_guided"))
              / (med("breed_uniform") + med("search_uniform")),
              "guided_repair_generation_over_uniform": (med("breed_guided_repair") + med("search_guided_repair"))
              / (med("breed_uniform") + med("search_uniform"))}
    dp.close()
    return {"config": config, "E": inst.E, "S": inst.S, "regime": regime, "members": P, "children": P,
            "members_feasible": pop_feasible, "search_steps": SEARCH_STEPS, "us": us, "children_sets": sets,
            "ratios": ratios}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="comp01,med")
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(REPO / "profiles" / "cx_bench.json"))
    ap.add_argument("--lib", default=None, help="profiling: an A/B build instead of the in-tree library")
    a = ap.parse_args()
    if a.lib:
        native._lib = native.load(pathlib.Path(a.lib).resolve())
    runs = [bench(c, a.rows, regime, a.repeats) for c in a.configs.split(",") for regime in ("random", "greedy")]
    worst = max(r["ratios"]["guided_repair_breed_over_uniform_search"] for r in runs)
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "runs": runs,
           "worst_guided_repair_breed_over_uniform_search": worst, "sanity_bound_held": worst <= 1.0}
    line = json.dumps(res)
    print(line)
    path = pathlib.Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(line + "\n")
    return 0 if worst <= 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
