"""Statistical comparison of whole-GA trajectories: the device GA against the
reference's own GA, same parameters, fixed seeds.

The device engine's random streams differ from the reference's (SURVEY F6:
one Park-Miller stream per individual instead of one shared stream), and it
crosses into a fresh child (no F2), so single trajectories cannot be compared
bit for bit (the per-operator kernels are: tests/test_gpu_parity.py). What is
compared is the distribution of outcomes over K fixed seeds:

* reference: ga.cpp with one MPI rank and one OpenMP thread (-c 1), i.e. the
  steady-state GA of pop_size members with one child per generation, run by
  oracle/_ref's ref_ga_run around the reference's own Solution objects, as is
  (F2 included) and with the crossover child fresh (as_is = 0);
* device: ttga.ga.Island(pop_size, children=1), the same generation count.

Per run the outcome is the value ga.cpp's setGlobalCost reports for pop[0]
(scv if feasible, else hcv*1e6 + scv, ga.cpp:234-257). Reported: feasibility
rate (Fisher exact test), best-scv distribution (Mann-Whitney U, two-sided),
medians of the logged best at generation checkpoints, and wall time per run.

    python tools/ga_quality.py [--config sm] [--seeds 16] [--gens 2001] [--steps 200] [--pop 10]

--unique compares the device GA with itself instead: Island(unique=True)
(duplicate-free replacement) against the plain island, same seeds and
parameters, no reference run: final values (Mann-Whitney U, two-sided), their
medians, the children dropped and the distinct genomes left per run.

--init greedy does the same for the initial population: Island(init="greedy")
(tt_greedy_init, include/ttga_greedy.h) against the plain island, same seeds
and parameters, no reference run: final values (Mann-Whitney U, two-sided),
their medians, and the medians of the logged best at generation checkpoints.

--kempe P [--kempe-max-chain N] does the same for the Kempe-chain move:
Island(kempe=P, kempe_max_chain=N) (tt_kempe_move, include/ttga_kempe.h) against
the plain island, same seeds and parameters, no reference run: final values
(Mann-Whitney U, two-sided), their medians, the medians of the logged best at
generation checkpoints, and per run the chains moved, rejected and their mean
length.

--slot-swap N does the same for the timeslot-swap descent: Island(slot_swap=N)
(tt_slot_swap, include/ttga_slotswap.h, max_passes N behind every search)
against the plain island, same seeds and parameters, no reference run: final
values (Mann-Whitney U, two-sided), their medians, the medians of the logged
best at generation checkpoints, and per run the rows, the rows improved, the
swaps applied and the scv gained.

--lahc N (with --lahc-history L, --lahc-swap P) does the same for the
late-acceptance search: Island(lahc=N, lahc_history=L, lahc_swap=P) (tt_lahc,
include/ttga_lahc.h, N steps behind every search) against the island without
it, same seeds and parameters, no reference run; per run the rows, the rows
searched and improved, the candidates accepted and the scv gained. Together
with --slot-swap M both islands run Island(slot_swap=M) and only the lahc
differs.

--crossover guided [--crossover-repair] does the same for the conflict-guided
crossover: Island(crossover="guided", crossover_repair=...) (tt_ga_breed_guided,
include/ttga_cx.h) against the island without it, same seeds and parameters, no
reference run; per run the children, how many crossed, how many of those at
cost 0, the cost and the events repaired. With --lahc N / --slot-swap M both
islands run them and only the crossover differs.
"""
import argparse
import json
import os
import pathlib
import sys
import time

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "timetabling-ga-mpi-openmp_amd"))
sys.path.insert(0, str(REPO / "tests"))
import numpy as np  # noqa: E402

import ttga  # noqa: E402


def summarize(final, feas, trace, checkpoints):
    fs = final[feas.astype(bool)]
    return {
        "feasible_rate": float(feas.mean()),
        "best_scv_feasible": {"median": float(np.median(fs)) if fs.size else None,
                              "mean": float(fs.mean()) if fs.size else None,
                              "min": int(fs.min()) if fs.size else None, "max": int(fs.max()) if fs.size else None},
        "final_log_value": [int(v) for v in final],
        "median_logged_best_at_generation": {str(g): float(np.median(trace[:, g])) for g in checkpoints},
    }


def device_runs(inst, seeds, pop, gens, steps, children=1, schedule="batch", unique=False, stats_out=None,
                init="random", kempe=0.0, kempe_max_chain=0, slot_swap=0, lahc=0, lahc_history=500,
                lahc_swap=0.5, crossover="uniform", crossover_repair=False):
    import torch

    from ttga import native
    from ttga.ga import Island
    dp = native.DeviceProblem(inst)
    final = np.zeros(len(seeds), np.int64)
    feas = np.zeros(len(seeds), np.uint8)
    trace = np.zeros((len(seeds), gens + 1), np.int64)
    secs = []
    for k, s in enumerate(seeds):
        isl = Island(dp, pop_size=pop, children=children, max_steps=steps, seed=int(s), schedule=schedule,
                     unique=unique, init=init, kempe=kempe, kempe_max_chain=kempe_max_chain,
                     slot_swap=slot_swap, lahc=lahc, lahc_history=lahc_history, lahc_swap=lahc_swap,
                     crossover=crossover, crossover_repair=crossover_repair)
        tr = torch.zeros(gens + 1, dtype=torch.int64, device="cuda")
        p = isl.pop

        def log(g):      # setCurrentCost's value for pop[0], kept on the device (no per-generation sync)
            h, c = p["hcv"][0].to(torch.int64), p["scv"][0].to(torch.int64)
            tr[g] = torch.where(p["feasible"][0] != 0, c, h * 1000000 + c)

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        isl.initialize()
        log(0)
        for g in range(gens):
            isl.step()
            log(g + 1)
        isl.flush()                      # staggered: the pending sub-batches replaced
        log(gens)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
        trace[k] = tr.cpu().numpy()
        feas[k] = 1 if isl.member_meta(0)[0] else 0
        final[k] = trace[k, -1]
        if stats_out is not None:
            if crossover == "guided":
                stats_out.append(isl.cx_stats())
            elif lahc > 0:
                stats_out.append(isl.lahc_stats())
            elif slot_swap > 0:
                stats_out.append(isl.slot_swap_stats())
            elif kempe > 0:
                stats_out.append(isl.kempe_stats())
            elif unique:
                stats_out.append(isl.unique_stats())
            else:            # the plain island's distinct genomes, for the comparison
                first = dp.genome_first(isl.pop["slot"], isl.pop["room"])
                stats_out.append({"distinct": int((first == torch.arange(pop, dtype=torch.int32, device="cuda")).sum())})
    return final, feas, trace, float(np.mean(secs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="sm")
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--first-seed", type=int, default=1)
    ap.add_argument("--gens", type=int, default=2001, help="ga.cpp runs generations 0..2000")
    ap.add_argument("--steps", type=int, default=200, help="maxSteps (-p 1: 200, -p 2: 1000, else 2000)")
    ap.add_argument("--pop", type=int, default=10)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--device-children", type=int, default=1, help="children per device generation")
    ap.add_argument("--device-gens", type=int, default=0, help="device generations (0: --gens)")
    ap.add_argument("--device-schedule", choices=["batch", "staggered"], default="batch")
    ap.add_argument("--no-ref-as-is", action="store_true", help="skip the reference run with F2")
    ap.add_argument("--unique", action="store_true",
                    help="compare Island(unique=True) with the plain island (no reference run)")
    ap.add_argument("--init", choices=["random", "greedy"], default="random",
                    help="greedy: compare Island(init='greedy') with the plain island (no reference run)")
    ap.add_argument("--kempe", type=float, default=0.0,
                    help="P > 0: compare Island(kempe=P) with the plain island (no reference run)")
    ap.add_argument("--kempe-max-chain", type=int, default=0, help="the cap on a chain's length (0: none)")
    ap.add_argument("--slot-swap", type=int, default=0,
                    help="N > 0: compare Island(slot_swap=N) with the plain island (no reference run)")
    ap.add_argument("--lahc", type=int, default=0,
                    help="N > 0: compare Island(lahc=N) with the island without it (no reference run)")
    ap.add_argument("--lahc-history", type=int, default=500)
    ap.add_argument("--lahc-swap", type=float, default=0.5)
    ap.add_argument("--crossover", choices=["uniform", "guided"], default="uniform",
                    help="guided: compare Island(crossover='guided') with the island without it (no reference run)")
    ap.add_argument("--crossover-repair", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scipy import stats

    import threading
    t_start = time.perf_counter()

    def heartbeat():                     # the long reference runs print nothing for minutes
        while True:
            time.sleep(30)
            print(f"[ga_quality] running {time.perf_counter() - t_start:.0f} s", file=sys.stderr, flush=True)
    threading.Thread(target=heartbeat, daemon=True).start()

    from oracle_lib import ref
    inst = ttga.config_instance(a.config)
    seeds = list(range(a.first_seed, a.first_seed + a.seeds))
    threads = a.threads or int(os.environ.get("OMP_NUM_THREADS", "0")) or min(16, os.cpu_count() or 1)
    checkpoints = sorted({0, 100, 500, 1000, a.gens // 2, a.gens} & set(range(a.gens + 1)))
    res = {"config": a.config, "E": inst.E, "R": inst.R, "F": inst.F, "S": inst.S, "pop_size": a.pop,
           "children_per_generation": 1, "generations": a.gens, "max_steps": a.steps, "seeds": seeds,
           "runs": {}}
    if a.crossover_repair and a.crossover != "guided":
        raise SystemExit("--crossover-repair needs --crossover guided")
    if a.crossover == "guided":
        dg = a.device_gens or a.gens
        res["children_per_generation"], res["generations"] = a.device_children, dg
        res["crossover"], res["crossover_repair"] = a.crossover, bool(a.crossover_repair)
        res["lahc"], res["lahc_history"], res["lahc_swap"], res["slot_swap"] = a.lahc, a.lahc_history, a.lahc_swap, a.slot_swap
        cps = sorted({0, 1, 10, 100, dg // 2, dg} & set(range(dg + 1)))
        for name, cx in (("device", "uniform"), ("device_guided", "guided")):
            st = [] if cx == "guided" else None
            final, feas, trace, secs = device_runs(inst, seeds, a.pop, dg, a.steps, a.device_children,
                                                   a.device_schedule, stats_out=st, slot_swap=a.slot_swap, lahc=a.lahc,
                                                   lahc_history=a.lahc_history, lahc_swap=a.lahc_swap, crossover=cx,
                                                   crossover_repair=a.crossover_repair and cx == "guided")
            res["runs"][name] = summarize(final, feas, trace, cps)
            res["runs"][name]["seconds_per_run"] = secs
            if st:
                res["runs"][name]["cx_stats"] = st
                crossed = sum(s["crossed"] for s in st)
                res["runs"][name]["clean_share"] = sum(s["clean"] for s in st) / max(1, crossed)
                res["runs"][name]["mean_cost"] = sum(s["cost"] for s in st) / max(1, crossed)
                res["runs"][name]["mean_repaired"] = sum(s["repaired"] for s in st) / max(1, crossed)
        vp, vg = (np.array(res["runs"][n]["final_log_value"]) for n in ("device", "device_guided"))
        same = bool(np.array_equal(vp, vg))
        res["tests"] = {"guided_vs_uniform": {
            "final_value_mannwhitney_p": 1.0 if same else float(stats.mannwhitneyu(vg, vp, alternative="two-sided").pvalue),
            "median_guided": float(np.median(vg)), "median_uniform": float(np.median(vp))}}
        print(json.dumps(res), flush=True)
        if a.out:
            pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
        return
    if a.unique:
        dg = a.device_gens or a.gens
        res["children_per_generation"], res["generations"] = a.device_children, dg
        for name, uniq in (("device", False), ("device_unique", True)):
            st = []
            final, feas, trace, secs = device_runs(inst, seeds, a.pop, dg, a.steps, a.device_children,
                                                   a.device_schedule, uniq, st)
            res["runs"][name] = summarize(final, feas, trace, sorted({0, dg // 2, dg}))
            res["runs"][name]["seconds_per_run"] = secs
            res["runs"][name]["distinct"] = [s["distinct"] for s in st]
            if uniq:
                res["runs"][name]["dropped"] = [s["dropped"] for s in st]
                res["runs"][name]["children"] = st[0]["children"]
        vp, vu = (np.array(res["runs"][n]["final_log_value"]) for n in ("device", "device_unique"))
        same = bool(np.array_equal(vp, vu))
        res["tests"] = {"unique_vs_plain": {
            "final_value_mannwhitney_p": 1.0 if same else float(stats.mannwhitneyu(vu, vp, alternative="two-sided").pvalue),
            "median_unique": float(np.median(vu)), "median_plain": float(np.median(vp))}}
        print(json.dumps(res), flush=True)
        if a.out:
            pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
        return
    if a.init == "greedy":
        dg = a.device_gens or a.gens
        res["children_per_generation"], res["generations"] = a.device_children, dg
        cps = sorted({0, 1, 10, 100, dg // 2, dg} & set(range(dg + 1)))
        for name, init in (("device", "random"), ("device_greedy", "greedy")):
            final, feas, trace, secs = device_runs(inst, seeds, a.pop, dg, a.steps, a.device_children,
                                                   a.device_schedule, init=init)
            res["runs"][name] = summarize(final, feas, trace, cps)
            res["runs"][name]["seconds_per_run"] = secs
        vp, vg = (np.array(res["runs"][n]["final_log_value"]) for n in ("device", "device_greedy"))
        same = bool(np.array_equal(vp, vg))
        res["tests"] = {"greedy_vs_random": {
            "final_value_mannwhitney_p": 1.0 if same else float(stats.mannwhitneyu(vg, vp, alternative="two-sided").pvalue),
            "median_greedy": float(np.median(vg)), "median_random": float(np.median(vp))}}
        print(json.dumps(res), flush=True)
        if a.out:
            pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
        return
    if a.kempe > 0:
        dg = a.device_gens or a.gens
        res["children_per_generation"], res["generations"] = a.device_children, dg
        res["kempe"], res["kempe_max_chain"] = a.kempe, a.kempe_max_chain
        cps = sorted({0, 1, 10, 100, dg // 2, dg} & set(range(dg + 1)))
        for name, prob in (("device", 0.0), ("device_kempe", a.kempe)):
            st = [] if prob > 0 else None
            final, feas, trace, secs = device_runs(inst, seeds, a.pop, dg, a.steps, a.device_children,
                                                   a.device_schedule, stats_out=st, kempe=prob,
                                                   kempe_max_chain=a.kempe_max_chain)
            res["runs"][name] = summarize(final, feas, trace, cps)
            res["runs"][name]["seconds_per_run"] = secs
            if st:
                res["runs"][name]["kempe_stats"] = st
                moved, events = sum(s["moved"] for s in st), sum(s["chain_events"] for s in st)
                res["runs"][name]["mean_chain"] = events / moved if moved else 0.0
        vp, vk = (np.array(res["runs"][n]["final_log_value"]) for n in ("device", "device_kempe"))
        same = bool(np.array_equal(vp, vk))
        res["tests"] = {"kempe_vs_plain": {
            "final_value_mannwhitney_p": 1.0 if same else float(stats.mannwhitneyu(vk, vp, alternative="two-sided").pvalue),
            "median_kempe": float(np.median(vk)), "median_plain": float(np.median(vp))}}
        print(json.dumps(res), flush=True)
        if a.out:
            pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
        return
    if a.lahc > 0:
        dg = a.device_gens or a.gens
        res["children_per_generation"], res["generations"] = a.device_children, dg
        res["lahc"], res["lahc_history"], res["lahc_swap"], res["slot_swap"] = a.lahc, a.lahc_history, a.lahc_swap, a.slot_swap
        cps = sorted({0, 1, 10, 100, dg // 2, dg} & set(range(dg + 1)))
        for name, n in (("device", 0), ("device_lahc", a.lahc)):
            st = [] if n > 0 else None
            final, feas, trace, secs = device_runs(inst, seeds, a.pop, dg, a.steps, a.device_children,
                                                   a.device_schedule, stats_out=st, slot_swap=a.slot_swap, lahc=n,
                                                   lahc_history=a.lahc_history, lahc_swap=a.lahc_swap)
            res["runs"][name] = summarize(final, feas, trace, cps)
            res["runs"][name]["seconds_per_run"] = secs
            if st:
                res["runs"][name]["lahc_stats"] = st
                res["runs"][name]["searched_share"] = sum(s["searched"] for s in st) / max(1, sum(s["rows"] for s in st))
                res["runs"][name]["improved_share"] = sum(s["improved"] for s in st) / max(1, sum(s["rows"] for s in st))
        vp, vs = (np.array(res["runs"][n]["final_log_value"]) for n in ("device", "device_lahc"))
        same = bool(np.array_equal(vp, vs))
        res["tests"] = {"lahc_vs_without": {
            "final_value_mannwhitney_p": 1.0 if same else float(stats.mannwhitneyu(vs, vp, alternative="two-sided").pvalue),
            "median_lahc": float(np.median(vs)), "median_without": float(np.median(vp))}}
        print(json.dumps(res), flush=True)
        if a.out:
            pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
        return
    if a.slot_swap > 0:
        dg = a.device_gens or a.gens
        res["children_per_generation"], res["generations"] = a.device_children, dg
        res["slot_swap"] = a.slot_swap
        cps = sorted({0, 1, 10, 100, dg // 2, dg} & set(range(dg + 1)))
        for name, n in (("device", 0), ("device_slot_swap", a.slot_swap)):
            st = [] if n > 0 else None
            final, feas, trace, secs = device_runs(inst, seeds, a.pop, dg, a.steps, a.device_children,
                                                   a.device_schedule, stats_out=st, slot_swap=n)
            res["runs"][name] = summarize(final, feas, trace, cps)
            res["runs"][name]["seconds_per_run"] = secs
            if st:
                res["runs"][name]["slot_swap_stats"] = st
                improved, passes = sum(s["improved"] for s in st), sum(s["passes"] for s in st)
                res["runs"][name]["mean_passes"] = passes / improved if improved else 0.0
                res["runs"][name]["improved_share"] = improved / max(1, sum(s["rows"] for s in st))
        vp, vs = (np.array(res["runs"][n]["final_log_value"]) for n in ("device", "device_slot_swap"))
        same = bool(np.array_equal(vp, vs))
        res["tests"] = {"slot_swap_vs_plain": {
            "final_value_mannwhitney_p": 1.0 if same else float(stats.mannwhitneyu(vs, vp, alternative="two-sided").pvalue),
            "median_slot_swap": float(np.median(vs)), "median_plain": float(np.median(vp))}}
        print(json.dumps(res), flush=True)
        if a.out:
            pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
        return
    R = ref()
    if R is None:
        raise SystemExit("oracle/_ref/libttref.so is missing (build it where /root/reference exists)")
    h = R.problem(inst)
    for name, as_is in ((("reference_as_is", 1),) if not a.no_ref_as_is else ()) + (("reference_fresh_child", 0),):
        hcv, scv, feas, pen, trace, secs = h.ga_run(seeds, a.pop, a.gens, a.steps, as_is, threads)
        final = trace[:, -1]
        res["runs"][name] = summarize(final, feas, trace, checkpoints)
        res["runs"][name]["seconds_per_run"] = secs * threads / len(seeds) if len(seeds) >= threads else secs
        res["runs"][name]["note"] = ("ref_ga_run, OpenMP over seeds (%d threads); seconds_per_run = wall x "
                                     "threads / runs" % threads)
    if not a.no_device:
        dg = a.device_gens or a.gens
        final, feas, trace, secs = device_runs(inst, seeds, a.pop, dg, a.steps, a.device_children, a.device_schedule)
        res["runs"]["device"] = summarize(final, feas, trace, sorted({0, dg // 2, dg}))
        res["runs"]["device"]["seconds_per_run"] = secs
        res["runs"]["device"]["note"] = (f"ttga.ga.Island(pop_size, children={a.device_children}, schedule="
                                         f"{a.device_schedule}), {dg} generations ({dg * a.device_children} children; "
                                         f"the reference: {a.gens}), one island at a time on cuda:0")
        tests = {}
        for name in [n for n in ("reference_as_is", "reference_fresh_child") if n in res["runs"]]:
            r = res["runs"][name]
            fa = np.array([v < 1000000 for v in r["final_log_value"]])
            fd = feas.astype(bool)
            table = [[int(fd.sum()), int((~fd).sum())], [int(fa.sum()), int((~fa).sum())]]
            fisher_p = float(stats.fisher_exact(table)[1])
            vd = np.array(res["runs"]["device"]["final_log_value"])
            vr = np.array(r["final_log_value"])
            mw = stats.mannwhitneyu(vd, vr, alternative="two-sided")
            tests["device_vs_" + name] = {"feasibility_fisher_p": fisher_p, "final_value_mannwhitney_p": float(mw.pvalue),
                                          "median_device": float(np.median(vd)), "median_reference": float(np.median(vr))}
        res["tests"] = tests
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
