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

--lahc N --lahc-kempe P (with --lahc-swap Q, --lahc-kempe-max-chain M) compares
the walk with Kempe-chain candidates, Island(lahc=N, lahc_swap=Q, lahc_kempe=P,
lahc_kempe_max_chain=M) (tt_lahc_kempe, include/ttga_lahc_kempe.h), against
Island(lahc=N) with Island's own lahc_swap, same seeds, history and
parameters, no reference run; per run the walk's counts and the chains tried,
capped, without a room and accepted, and their mean length.

--lahc N --lahc-kempe P --lahc-kempe-rooms augment compares the room rules of
those chains: Island(lahc_kempe_rooms="augment") (tt_lahc_kempe_aug,
include/ttga_lahc_kempe_aug.h: rooms by augmenting paths) against the same
island with the direct rule, same seeds, flags and parameters, no reference
run; per run the walk's counts and the chains' (with the rule also those a
path rescued and the bystanders displaced).

--lahc N --lahc-walkers K (with any of the walk's other flags) compares the
walk's parallel walkers: Island(lahc_walkers=K) (tt_lahc_multi,
include/ttga_lahc_multi.h: K walks from every row, the best one kept) against
the same island with the single walk, same seeds, flags and parameters, no
reference run; per run the walk's counts, and with the walkers the winners'
gain next to walker 0's on the same rows (`gain`, `gain_first`) and the share
of rows another walker won.

--crossover guided [--crossover-repair] does the same for the conflict-guided
crossover: Island(crossover="guided", crossover_repair=...) (tt_ga_breed_guided,
include/ttga_cx.h) against the island without it, same seeds and parameters, no
reference run; per run the children, how many crossed, how many of those at
cost 0, the cost and the events repaired. With --lahc N / --slot-swap M both
islands run them and only the crossover differs.
"""
import argparse
import functools
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
from ttga import stages  # noqa: E402


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
                lahc_swap=0.5, crossover="uniform", crossover_repair=False, lahc_kempe=0.0,
                lahc_kempe_max_chain=0, lahc_kempe_rooms="direct", lahc_walkers=1, move1_descent=0):
    import torch

    from ttga import native, stages
    from ttga.ga import Island
    stage_kw = {k: v for k, v in locals().items() if k in stages.KEYS}
    dp = native.DeviceProblem(inst)
    final = np.zeros(len(seeds), np.int64)
    feas = np.zeros(len(seeds), np.uint8)
    trace = np.zeros((len(seeds), gens + 1), np.int64)
    secs = []
    for k, s in enumerate(seeds):
        isl = Island(dp, pop_size=pop, children=children, max_steps=steps, seed=int(s), schedule=schedule, **stage_kw)
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
            stage = next((s for s in ("move1_descent", "cx", "lahc", "slot_swap", "kempe", "unique") if s in isl.on), None)
            if stage:        # the first of these that is on
                stats_out.append(getattr(isl, stage + "_stats")())
                if stage == "lahc" and "lahc_kempe" in isl.on:
                    stats_out[-1] = dict(stats_out[-1], kempe=isl.lahc_kempe_stats())
                if stage == "lahc" and "lahc_walkers" in isl.on:
                    stats_out[-1] = dict(stats_out[-1], walkers=isl.lahc_walkers_stats())
            else:            # the plain island's distinct genomes, for the comparison
                first = dp.genome_first(isl.pop["slot"], isl.pop["room"])
                stats_out.append({"distinct": int((first == torch.arange(pop, dtype=torch.int32, device="cuda")).sum())})
    return final, feas, trace, float(np.mean(secs))


def ab_compare(a, res, inst, seeds, names, kws, test, medians, extras=None, plain_stats=False, early=(1, 10, 100)):
    """The device GA against itself, same seeds and parameters, no reference
    run: res["runs"][names[0]] without a stage (Island keywords kws[0]) and
    res["runs"][names[1]] with it (kws[1]), then res["tests"][test]: the final
    values' Mann-Whitney U (two-sided) and their medians under the names
    medians = (with, without). extras(stats, with_stage) turns a run's per-seed
    stats into further keys of its record: asked for the run with the stage, and
    with plain_stats for the other too. The logged best is kept at generations
    0, `early`, half way and at the end. Prints the record and writes --out."""
    from scipy import stats
    dg = a.device_gens or a.gens
    res["children_per_generation"], res["generations"] = a.device_children, dg
    cps = sorted({0, *early, dg // 2, dg} & set(range(dg + 1)))
    for name, kw, with_stage in zip(names, kws, (False, True)):
        st = [] if extras and (with_stage or plain_stats) else None
        final, feas, trace, secs = device_runs(inst, seeds, a.pop, dg, a.steps, a.device_children, a.device_schedule,
                                               stats_out=st, **kw)
        res["runs"][name] = summarize(final, feas, trace, cps)
        res["runs"][name]["seconds_per_run"] = secs
        if st:
            res["runs"][name].update(extras(st, with_stage))
    vp, vw = (np.array(res["runs"][n]["final_log_value"]) for n in names)
    same = bool(np.array_equal(vp, vw))
    res["tests"] = {test: {
        "final_value_mannwhitney_p": 1.0 if same else float(stats.mannwhitneyu(vw, vp, alternative="two-sided").pvalue),
        medians[0]: float(np.median(vw)), medians[1]: float(np.median(vp))}}
    print(json.dumps(res), flush=True)
    if a.out:
        pathlib.Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


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
    plain, without = "with the plain island (no reference run)", "with the island without it (no reference run)"
    stages.add_arguments(ap, help={
        "unique": f"compare Island(unique=True) {plain}",
        "init": f"greedy: compare Island(init='greedy') {plain}",
        "kempe": f"P > 0: compare Island(kempe=P) {plain}",
        "slot_swap": f"N > 0: compare Island(slot_swap=N) {plain}",
        "lahc": f"N > 0: compare Island(lahc=N) {without}",
        "crossover": f"guided: compare Island(crossover='guided') {without}",
        "lahc_kempe": f"P > 0 (with --lahc N): compare Island(lahc=N, lahc_kempe=P) with Island(lahc=N)",
        "lahc_kempe_rooms": "augment (with --lahc N --lahc-kempe P): compare the room rules, same flags otherwise",
        "lahc_walkers": "K > 1 (with --lahc N): compare Island(lahc_walkers=K) with the single walk, same flags otherwise",
        "move1_descent": "N > 0: compare Island(move1_descent=N) with the same flags without it "
                         "(every other stage flag goes to both sides as given; no reference run)",
        "lahc_history": None, "lahc_swap": None, "crossover_repair": None, "lahc_kempe_max_chain": None})
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
    run = functools.partial(ab_compare, a, res, inst, seeds)
    rest = {"lahc": a.lahc, "lahc_history": a.lahc_history, "lahc_swap": a.lahc_swap, "slot_swap": a.slot_swap}
    if a.move1_descent > 0:                          # every other stage flag goes to both arms as it was given
        rest = {k: v for k, v in stages.island_kwargs(a).items() if k != "move1_descent"}
        stages.validate(**{k: v for k, v in rest.items() if k != "unique"})      # what Island would refuse, before any run
        res.update(rest, move1_descent=a.move1_descent)

        def extras(st, with_stage):
            if not with_stage:
                return {}
            improved = sum(s["improved"] for s in st)
            return {"move1_descent_stats": st, "improved_share": improved / max(1, sum(s["rows"] for s in st)),
                    "mean_passes": sum(s["meanPasses"] * s["improved"] for s in st) / improved if improved else 0.0}
        return run(("device", "device_move1_descent"), (rest, dict(rest, move1_descent=a.move1_descent)),
                   "move1_descent_vs_without", ("median_move1_descent", "median_without"), extras)
    if a.crossover == "guided":
        res["crossover"], res["crossover_repair"] = a.crossover, bool(a.crossover_repair)
        res.update(rest)

        def extras(st, _):
            crossed = max(1, sum(s["crossed"] for s in st))
            return {"cx_stats": st, "clean_share": sum(s["clean"] for s in st) / crossed,
                    "mean_cost": sum(s["cost"] for s in st) / crossed,
                    "mean_repaired": sum(s["repaired"] for s in st) / crossed}
        return run(("device", "device_guided"),
                   (rest, dict(rest, crossover="guided", crossover_repair=a.crossover_repair)),
                   "guided_vs_uniform", ("median_guided", "median_uniform"), extras)
    if a.unique:
        def extras(st, with_stage):
            d = {"distinct": [s["distinct"] for s in st]}
            return dict(d, dropped=[s["dropped"] for s in st], children=st[0]["children"]) if with_stage else d
        return run(("device", "device_unique"), ({"unique": False}, {"unique": True}), "unique_vs_plain",
                   ("median_unique", "median_plain"), extras, plain_stats=True, early=())
    if a.init == "greedy":
        return run(("device", "device_greedy"), ({"init": "random"}, {"init": "greedy"}), "greedy_vs_random",
                   ("median_greedy", "median_random"))
    if a.kempe > 0:
        res["kempe"], res["kempe_max_chain"] = a.kempe, a.kempe_max_chain

        def extras(st, _):
            moved, events = sum(s["moved"] for s in st), sum(s["chain_events"] for s in st)
            return {"kempe_stats": st, "mean_chain": events / moved if moved else 0.0}
        cap = {"kempe_max_chain": a.kempe_max_chain}
        return run(("device", "device_kempe"), (dict(cap, kempe=0.0), dict(cap, kempe=a.kempe)), "kempe_vs_plain",
                   ("median_kempe", "median_plain"), extras)
    if a.lahc_kempe_rooms == "augment" and not a.lahc_kempe > 0:
        raise SystemExit(stages.LAHC_KEMPE_ROOMS_NEEDS_KEMPE)
    if a.lahc_walkers > 1:                           # K walkers against the single walk, everything else alike
        message = stages.LAHC_WALKERS_NEEDS_LAHC if not a.lahc > 0 else (
            stages.lahc_kempe_error(a.lahc, a.lahc_swap, a.lahc_kempe) if a.lahc_kempe > 0 else None)
        if message:
            raise SystemExit(message)
        walk = dict(rest, lahc_kempe=a.lahc_kempe, lahc_kempe_max_chain=a.lahc_kempe_max_chain,
                    lahc_kempe_rooms=a.lahc_kempe_rooms)
        res.update(walk, lahc_walkers=a.lahc_walkers)

        def extras(st, with_stage):
            out = {"lahc_stats": st}
            if with_stage:
                w = [s["walkers"] for s in st]
                out.update(gain=sum(x["gain"] for x in w), gain_first=sum(x["gainFirst"] for x in w),
                           later_winner_share=sum(x["winnerLater"] for x in w) / max(1, sum(x["rows"] for x in w)))
            return out
        return run(("device_single", "device_walkers"), (walk, dict(walk, lahc_walkers=a.lahc_walkers)),
                   "walkers_vs_single", ("median_walkers", "median_single"), extras, plain_stats=True)
    if a.lahc_kempe > 0:
        message = stages.lahc_kempe_error(a.lahc, a.lahc_swap, a.lahc_kempe)
        if message:
            raise SystemExit(message)
        res.update(rest, lahc_kempe=a.lahc_kempe, lahc_kempe_max_chain=a.lahc_kempe_max_chain)
        default_swap = ap.get_default("lahc_swap")
        res["lahc_swap_without"] = default_swap

        def extras(st, with_stage):
            out = {"lahc_stats": st}
            if with_stage:
                k = [s["kempe"] for s in st]
                tried, acc = max(1, sum(x["tried"] for x in k)), sum(x["accepted"] for x in k)
                out.update(no_room_share=sum(x["no_room"] for x in k) / tried,
                           capped_share=sum(x["capped"] for x in k) / tried, accepted_share=acc / tried,
                           mean_chain=sum(x["chain_events"] for x in k) / acc if acc else 0.0)
                if "rescued" in k[0]:
                    out.update(rescued_share=sum(x["rescued"] for x in k) / tried,
                               displaced_per_accepted=sum(x["displaced"] for x in k) / acc if acc else 0.0)
            return out
        if a.lahc_kempe_rooms == "augment":          # the two room rules, everything else alike
            res["lahc_kempe_rooms"] = a.lahc_kempe_rooms
            chains = dict(rest, lahc_kempe=a.lahc_kempe, lahc_kempe_max_chain=a.lahc_kempe_max_chain)
            return run(("device_direct", "device_augment"), (chains, dict(chains, lahc_kempe_rooms="augment")),
                       "augment_vs_direct", ("median_augment", "median_direct"),
                       lambda st, _: extras(st, True), plain_stats=True)
        return run(("device_lahc", "device_lahc_kempe"),
                   (dict(rest, lahc_swap=default_swap),
                    dict(rest, lahc_kempe=a.lahc_kempe, lahc_kempe_max_chain=a.lahc_kempe_max_chain)),
                   "lahc_kempe_vs_lahc", ("median_lahc_kempe", "median_lahc"), extras, plain_stats=True)
    if a.lahc > 0:
        res.update(rest)

        def extras(st, _):
            rows = max(1, sum(s["rows"] for s in st))
            return {"lahc_stats": st, "searched_share": sum(s["searched"] for s in st) / rows,
                    "improved_share": sum(s["improved"] for s in st) / rows}
        return run(("device", "device_lahc"), (dict(rest, lahc=0), rest), "lahc_vs_without",
                   ("median_lahc", "median_without"), extras)
    if a.slot_swap > 0:
        res["slot_swap"] = a.slot_swap

        def extras(st, _):
            improved, passes = sum(s["improved"] for s in st), sum(s["passes"] for s in st)
            return {"slot_swap_stats": st, "mean_passes": passes / improved if improved else 0.0,
                    "improved_share": improved / max(1, sum(s["rows"] for s in st))}
        return run(("device", "device_slot_swap"), ({"slot_swap": 0}, {"slot_swap": a.slot_swap}),
                   "slot_swap_vs_plain", ("median_slot_swap", "median_plain"), extras)
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
