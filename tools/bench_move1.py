"""tt_move1_scan and tt_move1_descent against the walk and the local search, on
comp01 and on med, for tools/bench_lahc.py's 8,192 rows that are feasible at
entry:

    python tools/bench_move1.py [--configs comp01,med] [--rows 8192] [--repeats 5] [--out FILE]

Per instance, in one process and alternating, each call between device events
on restored rows and streams, `repeats` times over after a warm-up round:

  scan_summary   tt_move1_scan with the summary only
  scan_tables    tt_move1_scan with the summary and both tables
  descent_1      tt_move1_descent(max_passes = 1)
  descent_all    tt_move1_descent(max_passes = INT_MAX)
  lahc_1000      tt_lahc(steps = 1,000, history 500)
  search         tt_local_search_eval(1000) on the same rows

One JSON line goes to stdout and to profiles/move1_bench.json (--out): per call
the median us with the lowest and highest repeat, the descent's mean and
longest passes and mean gain, the mean feasible and improving counts of the
rows, the same rows' mean gain under the walk, and scan_summary over search,
which is recorded and not gated. It exits 1 only if

  * a descended row's fresh tt_eval has hcv != 0 or an scv other than the one
    the descent credited in place, or
  * scan_summary takes longer than (E * 44 / 1000) * lahc_1000 on the same
    rows: the exhaustive scan looks at E * 44 candidates a row, the walk at
    1,000, and the scan must not pay more per candidate than the walk pays per
    step. The bound is derived, not tuned.

Needs a GPU: there is no CPU path."""
import argparse
import json
import pathlib
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "timetabling-ga-mpi-openmp_amd"))
sys.path.insert(0, str(REPO / "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ttga  # noqa: E402
from ttga import native  # noqa: E402
from bench_lahc import SEARCH_STEPS, feasible_rows  # noqa: E402

INT_MAX = 2 ** 31 - 1
HISTORY = 500


def bench(config, P, repeats):
    inst = ttga.config_instance(config)
    dp = native.DeviceProblem(inst)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()
    saved_slot, saved_room, kept, distinct = feasible_rows(dp, P)
    seeds = torch.from_numpy(ttga.population_seeds(7000, P)).cuda()
    slot, room, rng = saved_slot.clone(), saved_room.clone(), seeds.clone()
    i32 = lambda *shape: torch.zeros(shape or (P,), dtype=torch.int32, device=dev)      # noqa: E731
    gain, passes, accepted, best_step = i32(), i32(), i32(), i32()
    summary, d_scv = i32(P, 6), i32(P, inst.E, 45)
    to_room = torch.zeros((P, inst.E, 45), dtype=torch.uint8, device=dev)
    out = (i32(), i32(), torch.empty(P, dtype=torch.uint8, device=dev), i32())          # hcv, scv, feasible, penalty
    hcv0, scv0, _, pen0 = (t.clone() for t in dp.eval(saved_slot, saved_room))
    assert int(hcv0.abs().sum()) == 0
    scv, pen = scv0.clone(), pen0.clone()

    def restore():
        slot.copy_(saved_slot)
        room.copy_(saved_room)
        rng.copy_(seeds)
        scv.copy_(scv0)
        pen.copy_(pen0)

    def descent(n):
        return lambda: dp.move1_descent(slot, room, n, scv=scv, penalty=pen, gain=gain, passes=passes)
    calls = {"scan_summary": lambda: dp.move1_scan(slot, room, summary=summary),
             "scan_tables": lambda: dp.move1_scan(slot, room, summary=summary, d_scv=d_scv, to_room=to_room),
             "descent_1": descent(1), "descent_all": descent(INT_MAX),
             "lahc_1000": lambda: dp.lahc(slot, room, rng, 1000, HISTORY, 0.5, scv=scv, penalty=pen, gain=gain,
                                          accepted=accepted, best_step=best_step),
             "search": lambda: dp.local_search(slot, room, rng, SEARCH_STEPS, out=out)}

    def timed(fn):
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record(st)
        fn()
        e.record(st)
        e.synchronize()
        return b.elapsed_time(e)

    times = {k: [] for k in calls}
    stats, wrong = {}, 0
    for rep in range(repeats + 1):                # round 0 warms up: code objects, the allocator, clocks
        for k, fn in calls.items():
            restore()
            t = timed(fn)
            if rep:
                times[k].append(t)
            if rep not in (0, repeats):
                continue
            if k.startswith("descent") or k == "lahc_1000":
                h, s, _, p = dp.eval(slot, room)
                bad = int(((h != 0) | (s != scv) | (p != pen) | (s != scv0 - gain)).sum())
                wrong += bad if k.startswith("descent") else 0
                g = gain.cpu().numpy()
                stats[k] = {"mean_gain": float(g.mean()), "improved": int((g > 0).sum())}
                if k.startswith("descent"):
                    n = passes.cpu().numpy()
                    stats[k].update(mean_passes=float(n.mean()), longest_passes=int(n.max()), rows_wrong=bad)
                    if k == "descent_all":        # the rows are local optima now
                        dp.move1_scan(slot, room, summary=summary)
                        stats[k]["rows_with_an_improving_move_left"] = int((summary[:, 2] != 0).sum())
            if k == "scan_summary":
                sm = summary.cpu().numpy()
                stats[k] = {"rows_scanned": int(sm[:, 0].sum()), "mean_feasible_moves": float(sm[:, 1].mean()),
                            "mean_improving_moves": float(sm[:, 2].mean()), "mean_best_delta": float(sm[:, 3].mean())}
    if dp.status() != 0:
        raise SystemExit(f"bench_move1: device status {dp.status()}")
    us = {k: {"median": 1e3 * float(np.median(v)), "min": 1e3 * float(min(v)), "max": 1e3 * float(max(v))}
          for k, v in times.items()}
    candidates = inst.E * 44
    bound = candidates / 1000 * us["lahc_1000"]["median"]
    return {"config": config, "E": inst.E, "S": inst.S, "rows": P, "history": HISTORY, "search_steps": SEARCH_STEPS,
            "feasible_rows_kept": kept, "distinct_rows": distinct, "mean_scv_at_entry": float(scv0.float().mean()),
            "us": us, "stats": stats, "candidates_per_row": candidates,
            "ns_per_candidate_scan_summary": 1e3 * us["scan_summary"]["median"] / (candidates * P),
            "ns_per_step_lahc_1000": 1e3 * us["lahc_1000"]["median"] / (1000 * P),
            "scan_summary_bound_us": bound, "scan_summary_within_bound": us["scan_summary"]["median"] <= bound,
            "scan_summary_over_search": us["scan_summary"]["median"] / us["search"]["median"],
            "descent_all_over_search": us["descent_all"]["median"] / us["search"]["median"],
            "rows_wrong": wrong}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="comp01,med")
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(REPO / "profiles" / "move1_bench.json"))
    a = ap.parse_args()
    runs = [bench(c, a.rows, a.repeats) for c in a.configs.split(",")]
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "runs": runs,
           "rows_wrong": sum(r["rows_wrong"] for r in runs),
           "scan_summary_within_bound": all(r["scan_summary_within_bound"] for r in runs)}
    line = json.dumps(res)
    print(line)
    path = pathlib.Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(line + "\n")
    return 0 if res["rows_wrong"] == 0 and res["scan_summary_within_bound"] else 1


if __name__ == "__main__":
    sys.exit(main())
