"""tt_ga_replace_unique against tt_ga_replace and tt_eval at the GA bench's
shape (comp01, population 65,536, 8,192 children by default):

    python tools/bench_unique.py [--config comp01] [--pop 65536] [--children 8192]
                                 [--launches 200] [--repeats 5] [--out FILE] [--lib path]

From one saved population (evaluated and sorted, as a previous replacement
leaves it) and two saved sets of evaluated children -- one with no duplicate,
one with every second child a copy of a member -- it times, in one process and
alternating, each with device events around `launches` back-to-back launches,
`repeats` times over:

  replace            restore the population, tt_ga_replace with the first set
  unique_nodup       restore, tt_ga_replace_unique with the first set
  unique_halfdup     restore, tt_ga_replace_unique with the second set
  restore            the restore alone (a device copy of the six arrays)
  eval               tt_eval over the same N + C rows
  first_random       tt_genome_first over the N saved members
  first_identical    tt_genome_first over N copies of one member

One JSON line goes to stdout and to profiles/unique_bench.json (--out): per
call the median us per launch, the lowest and highest repeat, and the bar
"extra_le_eval": unique_nodup - replace and unique_halfdup - replace are each
no more than eval (the existing kernel that reads the same rows once; the new
work is one memory-bound pass over them, a sort of C keys and the candidates'
comparisons). The results are checked first: with no duplicate the population
is tt_ga_replace's bit for bit, with half of them exactly those are dropped.
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
from ttga.ga import new_population  # noqa: E402

KEYS = ("slot", "room", "hcv", "scv", "feasible", "penalty")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="comp01")
    ap.add_argument("--pop", type=int, default=65536)
    ap.add_argument("--children", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=str(REPO / "profiles" / "unique_bench.json"))
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.lib:
        native._lib = native.load(pathlib.Path(a.lib).resolve())
    inst = ttga.config_instance(a.config)
    dp = native.DeviceProblem(inst)
    N, C, E = a.pop, a.children, inst.E
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream()

    # N + C random individuals in one allocation (tt_eval's rows), evaluated
    rows = new_population(N + C, E, dev)
    seeds = torch.from_numpy(ttga.population_seeds(12345, N + C)).cuda()
    dp.random_init(seeds, rows["slot"], rows["room"])
    ev = (rows["hcv"], rows["scv"], rows["feasible"], rows["penalty"])
    dp.eval(rows["slot"], rows["room"], out=ev)
    saved = {k: rows[k][:N].clone() for k in KEYS}
    dp.ga_replace(saved, None, dp.ga_work(N))                    # sorted: the survivors are in order
    nodup = {k: rows[k][N:].clone() for k in KEYS}
    halfdup = {k: v.clone() for k, v in nodup.items()}
    src = torch.from_numpy(np.random.default_rng(7).permutation(N)[:(C + 1) // 2]).cuda()
    for k in KEYS:                                               # every second child: a member, anywhere in pop
        halfdup[k][0::2] = saved[k][src]
    pop = {k: v.clone() for k, v in saved.items()}
    work, uwork = dp.ga_work(N), dp.ga_unique_work(N, C)
    keep = torch.empty(C, dtype=torch.uint8, device=dev)
    n_kept = torch.empty(1, dtype=torch.int32, device=dev)
    identical = {k: saved[k][:1].expand(N, E).contiguous() for k in ("slot", "room")}

    def restore():
        for k in KEYS:
            pop[k].copy_(saved[k])

    def run(fn, *args, **kw):
        restore()
        fn(*args, **kw)

    calls = {
        "replace": lambda: run(dp.ga_replace, pop, nodup, work),
        "unique_nodup": lambda: run(dp.ga_replace_unique, pop, nodup, uwork, keep, n_kept),
        "unique_halfdup": lambda: run(dp.ga_replace_unique, pop, halfdup, uwork, keep, n_kept),
        "restore": restore,
        "eval": lambda: dp.eval(rows["slot"], rows["room"], out=ev),
        "first_random": lambda: dp.genome_first(saved["slot"], saved["room"]),
        "first_identical": lambda: dp.genome_first(identical["slot"], identical["room"]),
    }
    # the results before they are timed
    calls["replace"]()
    want = {k: v.clone() for k, v in pop.items()}
    calls["unique_nodup"]()
    agree = all(torch.equal(pop[k], want[k]) for k in KEYS) and int(n_kept.item()) == C and bool(keep.all())
    calls["unique_halfdup"]()
    agree = agree and int(n_kept.item()) == C // 2 and not bool(keep[0::2].any()) and bool(keep[1::2].all())
    first = calls["first_random"]()
    agree = agree and torch.equal(first, torch.arange(N, dtype=torch.int32, device=dev))
    agree = agree and not bool(calls["first_identical"]().any())
    if not agree:
        raise SystemExit("bench_unique: the calls' results are not what they must be")
    dropped_half = C - int(n_kept.item())

    def timed(fn):
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record(st)
        for _ in range(a.launches):
            fn()
        e.record(st)
        e.synchronize()
        return b.elapsed_time(e) * 1e3 / a.launches

    for fn in calls.values():                     # warm-up: code objects, the allocator, clocks
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for group in (("replace", "unique_nodup", "unique_halfdup", "restore", "eval"), ("first_random", "first_identical")):
        for _ in range(a.repeats):
            for k in group:
                times[k].append(timed(calls[k]))
    us = {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()}
    extra = {k: us[k]["median"] - us["replace"]["median"] for k in ("unique_nodup", "unique_halfdup")}
    res = {"config": a.config, "N": N, "C": C, "E": E, "launches": a.launches, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(0), "agree": agree, "dropped_halfdup": dropped_half,
           "row_bytes": 2 * E * (N + C), "us_per_launch": us, "extra_us_over_replace": extra,
           "extra_over_eval": {k: v / us["eval"]["median"] for k, v in extra.items()},
           "extra_le_eval": all(v <= us["eval"]["median"] for v in extra.values())}
    line = json.dumps(res)
    print(line)
    path = pathlib.Path(a.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(line + "\n")
    return 0 if res["extra_le_eval"] else 1


if __name__ == "__main__":
    sys.exit(main())
