"""tt_slot_swap against tt_eval and the local search it follows in a generation,
on comp01 and on med, for 8,192 rows:

    python tools/bench_slotswap.py [--configs comp01,med] [--rows 8192] [--steps 200]
                                   [--repeats 9] [--out FILE] [--lib LIBRARY]

The rows are the members of an Island of that size after initialize()
(searched rows, the kind the GA feeds the move). Per instance, in one process
and alternating, each call between device events, `repeats` times over after a
warm-up round:

  swap_1             (a) tt_slot_swap(max_passes = 1)
  swap               (b) tt_slot_swap(max_passes = 2^31 - 1), uncapped
  eval               (c) tt_eval
  search             (d) tt_local_search_eval(steps), the drivers' default maxSteps
  swap_random        (e) (b) on as many tt_random_init rows: their descents are longer
  restore            the device copies that put the saved rows and Random
                     streams back before each of (a)-(e); outside their events

so every repeat does the same work. One JSON line goes to stdout and to
profiles/slotswap_bench.json (--out): per call the median us, the lowest and
the highest repeat; per swap call the mean and the longest descent in passes,
the rows improved and the mean gain; (b) over (d) and (e) over (d), which are
reported and not gated; and the one bar, "swap1_le_search": (a), one pass,
takes no longer than (d) on every instance -- a sanity bound, a pass of an
operator that runs behind every search must stay below the search. Exits 1
when the bar is missed. Needs a GPU: there is no CPU path."""
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
from ttga.ga import Island  # noqa: E402

UNCAPPED = 2 ** 31 - 1


def bench(config, P, steps, repeats):
    inst = ttga.config_instance(config)
    dp = native.DeviceProblem(inst)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    isl = Island(dp, pop_size=P, children=1, max_steps=steps, seed=1)
    isl.initialize()
    isl.sync()
    saved = (isl.pop["slot"].clone(), isl.pop["room"].clone())
    feasible_share = float(isl.pop["feasible"].float().mean().item())
    seeds = torch.from_numpy(ttga.population_seeds(3000, P)).cuda()
    rng = seeds.clone()
    random_slot, random_room = torch.empty_like(saved[0]), torch.empty_like(saved[1])
    dp.random_init(seeds.clone(), random_slot, random_room)
    slot, room = saved[0].clone(), saved[1].clone()
    gain = torch.zeros(P, dtype=torch.int32, device=dev)
    passes = torch.zeros(P, dtype=torch.int32, device=dev)
    out = (torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev),
           torch.empty(P, dtype=torch.uint8, device=dev), torch.empty(P, dtype=torch.int32, device=dev))

    def restore(src=saved):
        slot.copy_(src[0])
        room.copy_(src[1])
        rng.copy_(seeds)

    calls = {
        "swap_1": (restore, lambda: dp.slot_swap(slot, 1, gain=gain, passes=passes)),
        "swap": (restore, lambda: dp.slot_swap(slot, UNCAPPED, gain=gain, passes=passes)),
        "eval": (restore, lambda: dp.eval(slot, room, out=out)),
        "search": (restore, lambda: dp.local_search(slot, room, rng, steps, out=out)),
        "swap_random": (lambda: restore((random_slot, random_room)),
                        lambda: dp.slot_swap(slot, UNCAPPED, gain=gain, passes=passes)),
    }

    def timed(fn):
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record(st)
        fn()
        e.record(st)
        e.synchronize()
        return b.elapsed_time(e)

    times = {k: [] for k in list(calls) + ["restore"]}
    descents = {}
    for rep in range(repeats + 1):                # round 0 warms up: code objects, the allocator, clocks
        for k, (before, fn) in calls.items():
            tr = timed(before)
            t = timed(fn)
            if rep:
                times[k].append(t)
                times["restore"].append(tr)
            if k.startswith("swap"):
                g, n = gain.cpu().numpy(), passes.cpu().numpy()
                descents[k] = {"improved": int((n > 0).sum()), "mean_passes": float(n.mean()),
                               "max_passes": int(n.max()), "mean_gain": float(g.mean())}
    if dp.status() != 0:
        raise SystemExit(f"bench_slotswap: device status {dp.status()}")
    us = {k: {"median": 1e3 * float(np.median(v)), "min": 1e3 * float(min(v)), "max": 1e3 * float(max(v))}
          for k, v in times.items()}
    return {"config": config, "E": inst.E, "S": inst.S, "rows": P, "steps": steps,
            "feasible_share_of_rows": feasible_share, "us": us, "descents": descents,
            "swap_over_search": us["swap"]["median"] / us["search"]["median"],
            "swap_random_over_search": us["swap_random"]["median"] / us["search"]["median"],
            "swap1_over_search": us["swap_1"]["median"] / us["search"]["median"],
            "swap1_le_search": us["swap_1"]["median"] <= us["search"]["median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="comp01,med")
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=str(REPO / "profiles" / "slotswap_bench.json"))
    ap.add_argument("--lib", default=None, help="profiling: an A/B build instead of the in-tree library")
    a = ap.parse_args()
    if a.lib:
        native._lib = native.load(pathlib.Path(a.lib).resolve())
    runs = [bench(c, a.rows, a.steps, a.repeats) for c in a.configs.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "runs": runs,
           "swap1_le_search": all(r["swap1_le_search"] for r in runs)}
    line = json.dumps(res)
    print(line)
    path = pathlib.Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(line + "\n")
    return 0 if res["swap1_le_search"] else 1


if __name__ == "__main__":
    sys.exit(main())
