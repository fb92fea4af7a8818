"""tt_kempe_move against tt_mutation and the local search that follows it in a
generation, on comp01 and on med, for 8,192 children:

    python tools/bench_kempe.py [--configs comp01,med] [--children 8192] [--steps 200]
                                [--repeats 9] [--out FILE]

The children are the members of an Island of that size after initialize()
(searched rows, the kind the GA feeds the move). Per instance, in one process
and alternating, each call between device events, `repeats` times over after a
warm-up round:

  kempe              (a) tt_kempe_move(prob = 1, max_chain = 0)
  kempe_cap4         (b) tt_kempe_move(prob = 1, max_chain = 4)
  mutation           (c) tt_mutation
  search             (d) tt_local_search_eval(steps), the drivers' default maxSteps
  restore            the device copies that put the saved rows and Random
                     streams back before each of (a)-(d); outside their events

so every repeat does the same work. One JSON line goes to stdout and to
profiles/kempe_bench.json (--out): per call the median ms, the lowest and the
highest repeat; the chain lengths of (a) and (b) (mean, median and maximum
length of the chains moved, chains rejected by the cap); (a) over (c), which is
reported and not gated (both load the row, build the buckets and re-match two
slots, so the difference is the chain search); and the one bar,
"kempe_le_search": (a) takes no longer than (d) on every instance -- an
operator that runs before every search must stay below the search. Exits 1 when
the bar is missed. Needs a GPU: there is no CPU path."""
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
    slot, room = saved[0].clone(), saved[1].clone()
    chain = torch.zeros(P, dtype=torch.int32, device=dev)
    out = (torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev),
           torch.empty(P, dtype=torch.uint8, device=dev), torch.empty(P, dtype=torch.int32, device=dev))

    def restore():
        slot.copy_(saved[0])
        room.copy_(saved[1])
        rng.copy_(seeds)

    calls = {
        "kempe": lambda: dp.kempe_move(slot, room, rng, 1.0, 0, chain),
        "kempe_cap4": lambda: dp.kempe_move(slot, room, rng, 1.0, 4, chain),
        "mutation": lambda: dp.mutation(slot, room, rng),
        "search": lambda: dp.local_search(slot, room, rng, steps, out=out),
    }

    def timed(fn):
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record(st)
        fn()
        e.record(st)
        e.synchronize()
        return b.elapsed_time(e)

    times = {k: [] for k in list(calls) + ["restore"]}
    chains = {}
    for rep in range(repeats + 1):                # round 0 warms up: code objects, the allocator, clocks
        for k, fn in calls.items():
            tr = timed(restore)
            t = timed(fn)
            if rep:
                times[k].append(t)
                times["restore"].append(tr)
            if k.startswith("kempe"):
                c = chain.cpu().numpy()
                moved = c[c > 0]
                chains[k] = {"moved": int(moved.size), "rejected": int((c < 0).sum()),
                             "mean_chain": float(moved.mean()) if moved.size else 0.0,
                             "median_chain": float(np.median(moved)) if moved.size else 0.0,
                             "max_chain": int(np.abs(c).max())}
    if dp.status() != 0:
        raise SystemExit(f"bench_kempe: device status {dp.status()}")
    ms = {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()}
    return {"config": config, "E": inst.E, "R": inst.R, "EW64": (inst.E + 63) // 64, "children": P, "steps": steps,
            "feasible_share_of_rows": feasible_share, "ms": ms, "chains": chains,
            "kempe_over_mutation": ms["kempe"]["median"] / ms["mutation"]["median"],
            "kempe_over_search": ms["kempe"]["median"] / ms["search"]["median"],
            "kempe_le_search": ms["kempe"]["median"] <= ms["search"]["median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="comp01,med")
    ap.add_argument("--children", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=str(REPO / "profiles" / "kempe_bench.json"))
    a = ap.parse_args()
    runs = [bench(c, a.children, a.steps, a.repeats) for c in a.configs.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "runs": runs,
           "kempe_le_search": all(r["kempe_le_search"] for r in runs)}
    line = json.dumps(res)
    print(line)
    path = pathlib.Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(line + "\n")
    return 0 if res["kempe_le_search"] else 1


if __name__ == "__main__":
    sys.exit(main())
