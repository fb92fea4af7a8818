"""tt_eval_parts against the evaluation kernels that do the same work, at the
benchmark shape (med, P = 65,536 by default):

    python tools/bench_parts.py [--config med] [--pop 65536] [--launches 200] [--repeats 5] [--out FILE]

After a warm-up of every call it times, in one process and alternating,
tt_eval_parts (event_hcv = NULL), tt_eval_variant(..., 2) (eval_block: one
workgroup per individual, as tt_eval_parts) and tt_eval (the automatic
variant), each with device events around `launches` back-to-back launches,
`repeats` times over; then, the same way, tt_eval_parts with event_hcv and
tt_slot_histogram. One JSON line goes to stdout and to profiles/report_bench.json
(--out): per call the median us per launch, the lowest and highest repeat, and
"parts_le_block": the requirement that tt_eval_parts' median is no longer than
eval_block's. The results of the calls are compared first (the parts add up to
tt_eval's hcv and scv on every row). Needs a GPU: there is no CPU path."""
import argparse
import ctypes
import json
import pathlib
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "timetabling-ga-mpi-openmp_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ttga  # noqa: E402
from ttga import native  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="med")
    ap.add_argument("--pop", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(REPO / "profiles" / "report_bench.json"))
    a = ap.parse_args()
    inst = ttga.config_instance(a.config)
    dp = native.DeviceProblem(inst)
    P, E = a.pop, inst.E
    seeds = torch.from_numpy(ttga.population_seeds(12345, P)).cuda()
    slot = torch.empty((P, E), dtype=torch.uint8, device="cuda")
    room = torch.empty_like(slot)
    dp.random_init(seeds, slot, room)
    parts = torch.empty((P, 6), dtype=torch.int32, device="cuda")
    ehcv = torch.empty((P, E), dtype=torch.int32, device="cuda")
    hist = torch.empty((E, 45), dtype=torch.int32, device="cuda")
    out = dp.eval(slot, room)
    st = torch.cuda.current_stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    lib, h = dp.lib, dp.handle

    def check(rc):
        if rc != 0:
            raise native.TTError(rc, lib.tt_last_error().decode(errors="replace"))

    calls = {
        "eval_parts": lambda: check(lib.tt_eval_parts(h, slot.data_ptr(), room.data_ptr(), P, parts.data_ptr(), None,
                                                      sp)),
        "eval_block": lambda: dp.eval(slot, room, variant=2, out=out),
        "eval_auto": lambda: dp.eval(slot, room, variant=0, out=out),
        "eval_parts_event_hcv": lambda: check(lib.tt_eval_parts(h, slot.data_ptr(), room.data_ptr(), P,
                                                                parts.data_ptr(), ehcv.data_ptr(), sp)),
        "slot_histogram": lambda: check(lib.tt_slot_histogram(h, slot.data_ptr(), P, hist.data_ptr(), sp)),
    }
    # the calls agree before they are timed
    calls["eval_parts_event_hcv"]()
    hcv, scv = (t.clone() for t in dp.eval(slot, room, variant=2)[:2])
    p64 = parts.to(torch.int64)
    agree = bool(torch.equal(p64[:, :3].sum(1), hcv.to(torch.int64)) and
                 torch.equal(p64[:, 3:].sum(1), scv.to(torch.int64)) and
                 torch.equal(ehcv.to(torch.int64).sum(1), 2 * (p64[:, 0] + p64[:, 1])))
    calls["slot_histogram"]()
    agree = agree and bool((hist.sum(1) == P).all())
    if not agree:
        raise SystemExit("bench_parts: the calls' results disagree")

    def timed(fn):
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record(st)
        for _ in range(a.launches):
            fn()
        e.record(st)
        e.synchronize()
        return b.elapsed_time(e) * 1e3 / a.launches

    for fn in calls.values():                     # warm-up: code objects, occupancy queries, clocks
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for group in (("eval_parts", "eval_block", "eval_auto"), ("eval_parts_event_hcv", "slot_histogram")):
        for _ in range(a.repeats):
            for k in group:
                times[k].append(timed(calls[k]))
    us = {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()}
    res = {"config": a.config, "P": P, "E": E, "launches": a.launches, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0), "eval_variant_auto": dp.eval_variant(), "agree": agree,
           "us_per_launch": us,
           "parts_over_block": us["eval_parts"]["median"] / us["eval_block"]["median"],
           "parts_over_auto": us["eval_parts"]["median"] / us["eval_auto"]["median"],
           "parts_le_block": us["eval_parts"]["median"] <= us["eval_block"]["median"]}
    line = json.dumps(res)
    print(line)
    path = pathlib.Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(line + "\n")
    return 0 if res["parts_le_block"] else 1


if __name__ == "__main__":
    sys.exit(main())
