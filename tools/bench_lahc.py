"""tt_lahc against the local search it follows in a generation, on comp01 and on
med, for 8,192 rows that are feasible at entry:

    python tools/bench_lahc.py [--configs comp01,med] [--rows 8192] [--history 500]
                               [--repeats 5] [--out FILE] [--lib LIBRARY]

The rows come from tt_greedy_init + tt_local_search_eval(1000) on as many
streams; only the feasible ones are kept and the kept set is repeated to the
row count (every row keeps a stream of its own, so equal rows walk apart). Per
instance, in one process and alternating, each call between device events on
restored rows and streams, `repeats` times over after a warm-up round:

  lahc_1000    tt_lahc(steps = 1,000, history)
  lahc_10000   tt_lahc(steps = 10,000, history)
  search       tt_local_search_eval(1000) on the same rows

One JSON line goes to stdout and to profiles/lahc_bench.json (--out): how many
distinct rows there were, per call the median us with the lowest and highest
repeat, per tt_lahc call the ns per step and row, the mean gain, the accepted
share of the steps and the rows improved, and lahc_1000 over search, which is
recorded and not gated. The one failing exit (1): a row whose fresh tt_eval
has hcv != 0 or an scv other than the scv tt_lahc updated in place. Needs a
GPU: there is no CPU path."""
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


def feasible_rows(dp, P):
    """(slot, room, distinct): P rows feasible at entry, and how many of them differ."""
    rng = torch.from_numpy(ttga.population_seeds(5000, P)).cuda()
    slot = torch.empty((P, dp.E), dtype=torch.uint8, device="cuda")
    room = torch.empty_like(slot)
    dp.greedy_init(rng, slot, room)
    out = tuple(torch.empty(P, dtype=d, device="cuda") for d in (torch.int32, torch.int32, torch.uint8, torch.int32))
    dp.local_search(slot, room, rng, SEARCH_STEPS, out=out)
    feas = out[2]
    keep = torch.nonzero(feas != 0).flatten()
    if keep.numel() == 0:
        raise SystemExit("bench_lahc: no feasible row after the search")
    idx = keep[torch.arange(P, device="cuda") % keep.numel()]
    s, r = slot[idx].contiguous(), room[idx].contiguous()
    distinct = int(torch.unique(torch.cat([s[:keep.numel()], r[:keep.numel()]], dim=1), dim=0).shape[0])
    return s, r, int(keep.numel()), distinct


def bench(config, P, L, repeats):
    inst = ttga.config_instance(config)
    dp = native.DeviceProblem(inst)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    saved_slot, saved_room, kept, distinct = feasible_rows(dp, P)
    seeds = torch.from_numpy(ttga.population_seeds(7000, P)).cuda()
    slot, room, rng = saved_slot.clone(), saved_room.clone(), seeds.clone()
    i32 = lambda: torch.zeros(P, dtype=torch.int32, device=dev)                    # noqa: E731
    gain, accepted, best_step = i32(), i32(), i32()
    out = (i32(), i32(), torch.empty(P, dtype=torch.uint8, device=dev), i32())     # hcv, scv, feasible, penalty
    hcv0, scv0, _, pen0 = (t.clone() for t in dp.eval(saved_slot, saved_room))
    assert int(hcv0.abs().sum()) == 0
    scv, pen = scv0.clone(), pen0.clone()

    def restore():
        slot.copy_(saved_slot)
        room.copy_(saved_room)
        rng.copy_(seeds)
        scv.copy_(scv0)
        pen.copy_(pen0)

    def lahc(n):
        return lambda: dp.lahc(slot, room, rng, n, L, 0.5, scv=scv, penalty=pen, gain=gain, accepted=accepted,
                               best_step=best_step)
    calls = {"lahc_1000": lahc(1000), "lahc_10000": lahc(10000),
             "search": lambda: dp.local_search(slot, room, rng, SEARCH_STEPS, out=out)}

    def timed(fn):
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record(st)
        fn()
        e.record(st)
        e.synchronize()
        return b.elapsed_time(e)

    times = {k: [] for k in calls}
    walks, wrong = {}, 0
    for rep in range(repeats + 1):                # round 0 warms up: code objects, the allocator, clocks
        for k, fn in calls.items():
            restore()
            t = timed(fn)
            if rep:
                times[k].append(t)
            if k.startswith("lahc") and rep in (0, repeats):
                n = int(k.split("_")[1])
                h, s, _, p = dp.eval(slot, room)
                wrong += int(((h != 0) | (s != scv) | (p != pen) | (s != scv0 - gain)).sum())
                g, a = gain.cpu().numpy(), accepted.cpu().numpy()
                walks[k] = {"mean_gain": float(g.mean()), "improved": int((g > 0).sum()),
                            "accepted_share": float(a.mean()) / n, "mean_best_step": float(best_step.float().mean())}
    if dp.status() != 0:
        raise SystemExit(f"bench_lahc: device status {dp.status()}")
    us = {k: {"median": 1e3 * float(np.median(v)), "min": 1e3 * float(min(v)), "max": 1e3 * float(max(v))}
          for k, v in times.items()}
    for k, w in walks.items():
        w["ns_per_step_per_row"] = 1e3 * us[k]["median"] / (int(k.split("_")[1]) * P)
    return {"config": config, "E": inst.E, "S": inst.S, "rows": P, "history": L, "search_steps": SEARCH_STEPS,
            "feasible_rows_kept": kept, "distinct_rows": distinct, "mean_scv_at_entry": float(scv0.float().mean()),
            "us": us, "walks": walks, "lahc1000_over_search": us["lahc_1000"]["median"] / us["search"]["median"],
            "rows_wrong": wrong}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="comp01,med")
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--history", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(REPO / "profiles" / "lahc_bench.json"))
    ap.add_argument("--lib", default=None, help="profiling: an A/B build instead of the in-tree library")
    a = ap.parse_args()
    if a.lib:
        native._lib = native.load(pathlib.Path(a.lib).resolve())
    runs = [bench(c, a.rows, a.history, a.repeats) for c in a.configs.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "runs": runs,
           "rows_wrong": sum(r["rows_wrong"] for r in runs)}
    line = json.dumps(res)
    print(line)
    path = pathlib.Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(line + "\n")
    return 0 if res["rows_wrong"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
