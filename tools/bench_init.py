"""tt_greedy_init against tt_random_init and the local search it is meant to
shorten, on med and on comp01 at population 65,536:

    python tools/bench_init.py [--configs med,comp01] [--pop 65536] [--steps 200]
                               [--repeats 5] [--out FILE]

Per instance, in one process and alternating, each call between device events,
`repeats` times over after a warm-up round:

  random_init        (a) tt_random_init
  greedy_init        (b) tt_greedy_init with the order precomputed
  greedy_order       (c) tt_greedy_order
  search_random      (d) tt_local_search(steps) with fused evaluation on the rows of (a)
  search_greedy      (e) the same search on the rows of (b)

The Random streams are restored before every initialisation and the saved rows
before every search (device copies, outside the events), so each repeat does the
same work. One JSON line goes to stdout and to profiles/greedy_init.json
(--out): per call the median ms, the lowest and the highest repeat; the mean
hcv and the feasible share after (a), (b), (d) and (e); and the one bar,
"init_le_search": (b) takes no longer than (d) on every instance -- the
construction exists to save search work, so it must cost less than the search
it is meant to shorten. Whether (e) is faster than (d) is reported, not gated.
Exits 1 when the bar is missed. Needs a GPU: there is no CPU path."""
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


def bench(config, P, steps, repeats):
    inst = ttga.config_instance(config)
    dp = native.DeviceProblem(inst)
    E = inst.E
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    seeds = torch.from_numpy(ttga.population_seeds(1000, P)).cuda()
    ls_seeds = torch.from_numpy(ttga.population_seeds(2000, P)).cuda()
    rng = seeds.clone()
    slot = torch.empty((P, E), dtype=torch.uint8, device=dev)
    room = torch.empty_like(slot)
    out = (torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev),
           torch.empty(P, dtype=torch.uint8, device=dev), torch.empty(P, dtype=torch.int32, device=dev))
    order = dp.greedy_order()
    work = torch.empty(int(dp.lib.tt_greedy_work_bytes(dp.handle)), dtype=torch.uint8, device=dev)
    order2 = torch.empty_like(order)

    def quality():
        hcv, _, feas, _ = out
        return {"mean_hcv": float(hcv.float().mean().item()), "feasible_share": float(feas.float().mean().item())}

    # the rows of (a) and (b), saved with their evaluation
    saved, stats = {}, {}
    for kind, init in (("random", dp.random_init), ("greedy", dp.greedy_init)):
        rng.copy_(seeds)
        init(rng, slot, room)
        dp.eval(slot, room, out=out)
        saved[kind] = (slot.clone(), room.clone())
        stats[kind + "_init"] = quality()

    def init_call(fn):
        def prepare():
            rng.copy_(seeds)
        return prepare, lambda: fn(rng, slot, room)

    def search_call(kind):
        def prepare():
            slot.copy_(saved[kind][0])
            room.copy_(saved[kind][1])
            rng.copy_(ls_seeds)
        return prepare, lambda: dp.local_search(slot, room, rng, steps, out=out)

    def order_call():
        native._check(dp.lib, dp.lib.tt_greedy_order(dp.handle, order2.data_ptr(), work.data_ptr(), dp._stream(order2)))

    calls = {
        "random_init": init_call(dp.random_init),
        "greedy_init": init_call(lambda r, s, m: dp.greedy_init(r, s, m, order=order)),
        "greedy_order": (lambda: None, order_call),
        "search_random": search_call("random"),
        "search_greedy": search_call("greedy"),
    }

    def timed(prepare, fn):
        prepare()
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record(st)
        fn()
        e.record(st)
        e.synchronize()
        return b.elapsed_time(e)

    times = {k: [] for k in calls}
    for rep in range(repeats + 1):                # round 0 warms up: code objects, the allocator, clocks
        for k, (prepare, fn) in calls.items():
            t = timed(prepare, fn)
            if rep:
                times[k].append(t)
            if k.startswith("search_"):
                stats[k] = quality()
    if not torch.equal(order2, order):
        raise SystemExit("bench_init: tt_greedy_order is not reproducible")
    if dp.status() != 0:
        raise SystemExit(f"bench_init: device status {dp.status()}")
    ms = {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()}
    return {"config": config, "E": E, "R": inst.R, "P": P, "steps": steps, "ms": ms, "after": stats,
            "greedy_init_over_search_random": ms["greedy_init"]["median"] / ms["search_random"]["median"],
            "search_greedy_over_search_random": ms["search_greedy"]["median"] / ms["search_random"]["median"],
            "init_le_search": ms["greedy_init"]["median"] <= ms["search_random"]["median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="med,comp01")
    ap.add_argument("--pop", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(REPO / "profiles" / "greedy_init.json"))
    a = ap.parse_args()
    runs = [bench(c, a.pop, a.steps, a.repeats) for c in a.configs.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "runs": runs,
           "init_le_search": all(r["init_le_search"] for r in runs)}
    line = json.dumps(res)
    print(line)
    path = pathlib.Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(line + "\n")
    return 0 if res["init_le_search"] else 1


if __name__ == "__main__":
    sys.exit(main())
