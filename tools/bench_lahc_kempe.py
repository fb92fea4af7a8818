"""tt_lahc_kempe and tt_lahc_kempe_aug against tt_lahc, on comp01 and on med, on tools/bench_lahc.py's
rows (8,192 rows that are feasible at entry):

    python tools/bench_lahc_kempe.py [--configs comp01,med] [--rows 8192] [--history 500]
                                     [--repeats 5] [--out FILE] [--lib LIBRARY]

Per instance, in one process and alternating, each call between device events
on restored rows and streams, `repeats` times over after a warm-up round, all
at 1,000 steps:

  lahc           tt_lahc(p_swap 0.5)
  kempe20        tt_lahc_kempe(p_swap 0.5, p_kempe 0.2)
  kempe20_cap8   the same with max_chain 8
  kempe50        tt_lahc_kempe(p_swap 0.25, p_kempe 0.5)
  kempe50_cap8   the same with max_chain 8

and next to each tt_lahc_kempe call its twin <name>_aug: tt_lahc_kempe_aug with
the same arguments and room_rule 1 (rooms by augmenting paths).

One JSON line goes to stdout and to profiles/lahc_kempe_aug_bench.json (--out):
per call the median us with the lowest and highest repeat, the mean gain, the
accepted share of the steps, and per tt_lahc_kempe call the five Kempe counts
summed over the rows, the no-room share of the candidates and the mean length
of the accepted chains; per twin the seven counts and chain_step_over_direct,
the time of its chain steps over its direct twin's (each call's time less the
tt_lahc time of its ordinary steps). Nothing is gated but correctness, the one failing exit
(1): a row whose fresh tt_eval has hcv != 0 or an scv other than the scv
updated in place. Needs a GPU: there is no CPU path."""
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
from bench_lahc import feasible_rows  # noqa: E402
from ttga import native  # noqa: E402

STEPS = 1000
# name: (p_swap, p_kempe, max_chain); None: tt_lahc
DIRECT = {"kempe20": (0.5, 0.2, 0), "kempe20_cap8": (0.5, 0.2, 8), "kempe50": (0.25, 0.5, 0),
          "kempe50_cap8": (0.25, 0.5, 8)}
# and behind every one of them its twin with a fourth entry, tt_lahc_kempe_aug's room_rule
CALLS = {"lahc": None}
for _name, _arg in DIRECT.items():
    CALLS[_name] = _arg
    CALLS[_name + "_aug"] = _arg + (1,)


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
    stats = torch.zeros((P, 5), dtype=torch.int32, device=dev)
    stats7 = torch.zeros((P, 7), dtype=torch.int32, device=dev)
    hcv0, scv0, _, pen0 = (t.clone() for t in dp.eval(saved_slot, saved_room))
    assert int(hcv0.abs().sum()) == 0
    scv, pen = scv0.clone(), pen0.clone()

    def restore():
        slot.copy_(saved_slot)
        room.copy_(saved_room)
        rng.copy_(seeds)
        scv.copy_(scv0)
        pen.copy_(pen0)

    def call(arg):
        if arg is None:
            return lambda: dp.lahc(slot, room, rng, STEPS, L, 0.5, scv=scv, penalty=pen, gain=gain, accepted=accepted,
                                   best_step=best_step)
        if len(arg) == 4:
            return lambda: dp.lahc_kempe_aug(slot, room, rng, STEPS, L, arg[0], arg[1], arg[2], arg[3], scv=scv,
                                             penalty=pen, gain=gain, accepted=accepted, best_step=best_step,
                                             kempe_stats=stats7)
        return lambda: dp.lahc_kempe(slot, room, rng, STEPS, L, arg[0], arg[1], arg[2], scv=scv, penalty=pen, gain=gain,
                                     accepted=accepted, best_step=best_step, kempe_stats=stats)

    def timed(fn):
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record(st)
        fn()
        e.record(st)
        e.synchronize()
        return b.elapsed_time(e)

    times = {k: [] for k in CALLS}
    walks, wrong = {}, 0
    for rep in range(repeats + 1):                # round 0 warms up: code objects, the allocator, clocks
        for k, arg in CALLS.items():
            restore()
            t = timed(call(arg))
            if rep:
                times[k].append(t)
            if rep in (0, repeats):
                h, s, _, p = dp.eval(slot, room)
                wrong += int(((h != 0) | (s != scv) | (p != pen) | (s != scv0 - gain)).sum())
                g, a = gain.cpu().numpy(), accepted.cpu().numpy()
                walks[k] = {"mean_gain": float(g.mean()), "improved": int((g > 0).sum()),
                            "accepted_share": float(a.mean()) / STEPS}
                if arg is not None:
                    counts = [int(x) for x in (stats7 if len(arg) == 4 else stats).sum(dim=0).cpu()]
                    tried, capped, no_room, acc, events = counts[:5]
                    walks[k].update(p_swap=arg[0], p_kempe=arg[1], max_chain=arg[2], tried=tried, capped=capped,
                                    no_room=no_room, accepted=acc, chain_events=events,
                                    no_room_share=no_room / tried if tried else 0.0,
                                    mean_chain=events / acc if acc else 0.0)
                    if len(arg) == 4:
                        walks[k].update(room_rule=arg[3], rescued=counts[5], displaced=counts[6],
                                        rescued_share=counts[5] / tried if tried else 0.0)
    if dp.status() != 0:
        raise SystemExit(f"bench_lahc_kempe: device status {dp.status()}")
    us = {k: {"median": 1e3 * float(np.median(v)), "min": 1e3 * float(min(v)), "max": 1e3 * float(max(v))}
          for k, v in times.items()}
    for k, w in walks.items():
        w["over_lahc"] = us[k]["median"] / us["lahc"]["median"]
    for k, arg in DIRECT.items():
        ordinary = (1.0 - arg[1]) * us["lahc"]["median"]
        walks[k + "_aug"]["chain_step_over_direct"] = (us[k + "_aug"]["median"] - ordinary) / (us[k]["median"] - ordinary)
    return {"config": config, "E": inst.E, "R": inst.R, "S": inst.S, "rows": P, "history": L, "steps": STEPS,
            "feasible_rows_kept": kept, "distinct_rows": distinct, "mean_scv_at_entry": float(scv0.float().mean()),
            "us": us, "walks": walks, "rows_wrong": wrong}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="comp01,med")
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--history", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(REPO / "profiles" / "lahc_kempe_aug_bench.json"))
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
