"""The CPU restatement (oracle/) is pinned against the reference's own outputs.

Golden vectors in tests/golden/ come from the reference's Problem/Solution
objects (oracle/gen_golden.py). Where oracle/_ref/libttref.so exists, the
restatement is additionally cross-checked on fresh random inputs.
"""
import numpy as np
import pytest

import move3_cases as mc
import ttga
from oracle_lib import oracle, ref, split_rows

NAMES = ["sm", "med", "tight"]


def load(golden_dir, name):
    z = np.load(golden_dir / f"{name}.npz")
    E, R, F, S = (int(x) for x in z["dims"])
    inst = ttga.Instance(E, R, F, S, z["room_size"], z["student_events"], z["room_features"], z["event_features"])
    return inst, z


@pytest.fixture(scope="module")
def orc():
    return oracle()


def test_rng_known_answers(golden_dir, orc):
    z = np.load(golden_dir / "rng.npz")
    for seed, draws, final in zip(z["seeds"], z["draws"], z["finals"]):
        d, f = orc.rand(int(seed), draws.size)
        assert np.array_equal(d, draws) and f == final
        r = ttga.ParkMiller(int(seed))
        py = np.array([r.next() for _ in range(draws.size)])
        assert np.array_equal(py, draws) and r.seed == final


def test_random_slots_vectorised_matches_stream(golden_dir):
    seeds = ttga.population_seeds(12345, 5)
    slots, finals = ttga.random_slots(seeds, 50)
    for i, s in enumerate(seeds):
        r = ttga.ParkMiller(int(s))
        assert [r.pick(45) for _ in range(50)] == slots[i].tolist()
        assert r.seed == finals[i]


def test_tim_roundtrip_and_derived(golden_dir, orc):
    inst = ttga.read_tim(golden_dir / "sm.tim")
    _, z = load(golden_dir, "sm")
    assert np.array_equal(inst.student_events, z["student_events"])
    assert inst.to_tim() == (golden_dir / "sm.tim").read_text()
    sn, corr, poss = orc.problem(inst).derived()
    assert np.array_equal(sn, z["ref_student_number"])
    assert np.array_equal(np.packbits(corr.astype(np.uint8), axis=1), z["ref_corr_bits"])
    assert np.array_equal(poss, z["ref_possible"])
    # numpy restatement too
    assert np.array_equal(inst.student_number(), sn)
    assert np.array_equal(inst.correlations(), corr)
    assert np.array_equal(inst.possible_rooms(), poss)


def test_tim_parser_rejects_truncated():
    with pytest.raises(ValueError):
        ttga.parse_tim("3 1 0 2\n5\n1 0")


@pytest.mark.parametrize("name", NAMES)
def test_derived(golden_dir, orc, name):
    inst, z = load(golden_dir, name)
    sn, corr, poss = orc.problem(inst).derived()
    assert np.array_equal(sn, z["ref_student_number"])
    assert np.array_equal(np.packbits(corr.astype(np.uint8), axis=1), z["ref_corr_bits"])
    assert np.array_equal(poss, z["ref_possible"])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("tag,sk,rk", [("canon", "slots", "rooms"), ("rand", "slots", "rand_rooms"),
                                       ("skew", "skew_slots", "skew_rooms"), ("edge", "edge_slots", "edge_rooms"),
                                       ("ls3", "ls3_slots", "ls3_rooms")])
def test_eval(golden_dir, orc, name, tag, sk, rk):
    inst, z = load(golden_dir, name)
    h = orc.problem(inst)
    hcv, scv, feas, pen = h.eval(z[sk], z[rk])
    assert np.array_equal(hcv, z[f"eval_{tag}_hcv"])
    assert np.array_equal(scv, z[f"eval_{tag}_scv"])
    assert np.array_equal(feas, z[f"eval_{tag}_feasible"])
    assert np.array_equal(pen, z[f"eval_{tag}_penalty"])


@pytest.mark.parametrize("name", NAMES)
def test_assign_rooms(golden_dir, orc, name):
    inst, z = load(golden_dir, name)
    h = orc.problem(inst)
    assert np.array_equal(h.assign_rooms(z["slots"]), z["rooms"])
    assert np.array_equal(h.assign_rooms(z["skew_slots"]), z["skew_rooms"])


@pytest.mark.parametrize("name", NAMES)
def test_variation(golden_dir, orc, name):
    inst, z = load(golden_dir, name)
    h = orc.problem(inst)
    s, r, g = h.random_init(z["init_seeds"])
    assert np.array_equal(s, z["init_slots"]) and np.array_equal(r, z["init_rooms"])
    assert np.array_equal(g, z["init_rng"])
    n = z["init_slots"].shape[0] // 2
    s, r, g = h.crossover(z["init_slots"][:n], z["init_slots"][n:], z["xover_seeds"])
    assert np.array_equal(s, z["xover_slots"]) and np.array_equal(r, z["xover_rooms"])
    assert np.array_equal(g, z["xover_rng"])
    s, r, g = h.mutation(z["init_slots"], z["init_rooms"], z["mut_seeds"])
    assert np.array_equal(s, z["mut_slots"]) and np.array_equal(r, z["mut_rooms"])
    assert np.array_equal(g, z["mut_rng"])


@pytest.mark.parametrize("name", NAMES)
def test_local_search(golden_dir, orc, name):
    inst, z = load(golden_dir, name)
    h = orc.problem(inst)
    n = z["ls_seeds"].size
    s, r, g = h.local_search(z["init_slots"][:n], z["init_rooms"][:n], z["ls_seeds"], 200)
    assert np.array_equal(s, z["ls_slots"]) and np.array_equal(r, z["ls_rooms"]) and np.array_equal(g, z["ls_rng"])
    s, r, g = h.local_search(s, r, g, 1000)
    assert np.array_equal(s, z["ls2_slots"]) and np.array_equal(r, z["ls2_rooms"]) and np.array_equal(g, z["ls2_rng"])
    s, r, g = h.local_search(s, r, g, 2000)
    assert np.array_equal(s, z["ls3_slots"]) and np.array_equal(r, z["ls3_rooms"]) and np.array_equal(g, z["ls3_rng"])
    s, r, g = h.local_search(z["init_slots"][:4], z["init_rooms"][:4], ttga.population_seeds(9500, 4), 60, 1, 1, 1)
    assert np.array_equal(s, z["lsp3_slots"]) and np.array_equal(r, z["lsp3_rooms"])
    assert np.array_equal(g, z["lsp3_rng"])


@pytest.mark.parametrize("tag", list(mc.GOLDEN_SHAPES))
def test_local_search_move3_golden(golden_dir, orc, tag):
    """Move3 (prob3 > 0) of the oracle against the reference's own localSearch
    (tests/golden/move3.npz): 8 phase-1 and 8 feasible rows of two instances,
    Move3 alone for 64 steps, every move for 300, a mix for 300. The fixture
    holds accepted Move3s of both phases (rows changed with prob1 = prob2 = 0;
    from the feasible rows on the 300-event instance)."""
    z = np.load(golden_dir / "move3.npz")
    inst = mc.golden_instance(z, tag)
    assert inst.to_tim() == mc.instance(mc.GOLDEN_SHAPES[tag]).to_tim()
    changed = mc.check_golden(z, tag, orc.problem(inst).local_search)
    assert changed["a", 0] == mc.GOLDEN_ROWS
    if tag == "e300":
        assert changed["b", 0] >= 1
    assert changed["b", 1] >= 1 and changed["b", 2] >= 1


# ---- live cross-checks against the reference build (skipped where it was never built)
REF = ref()
needs_ref = pytest.mark.skipif(REF is None, reason="oracle/_ref not built (no /root/reference)")


@needs_ref
@pytest.mark.parametrize("seed", [3, 4])
def test_oracle_vs_reference_random(orc, seed):
    inst = ttga.generate(150, 6, 4, 120, seed=seed)
    ho, hr = orc.problem(inst), REF.problem(inst)
    slots, _ = ttga.random_slots(ttga.population_seeds(seed * 1000, 40), inst.E)
    ro, rr = ho.assign_rooms(slots), hr.assign_rooms(slots)
    assert np.array_equal(ro, rr)
    for a, b in zip(ho.eval(slots, ro), hr.eval(slots, rr)):
        assert np.array_equal(a, b)
    seeds = ttga.population_seeds(seed * 77, 6)
    for a, b in zip(ho.local_search(slots[:6], ro[:6], seeds, 300), hr.local_search(slots[:6], rr[:6], seeds, 300)):
        assert np.array_equal(a, b)


@needs_ref
def test_oracle_vs_reference_med_ls_chain(orc):
    """The chain of tests/test_gpu_parity.py::test_local_search_med_population_vs_oracle
    (med, 96 individuals, localSearch 200 -> 1000 -> 3000 into phase 2), run by the
    reference's own Solution code: the oracle that checks the GPU there equals it
    here, so the GPU result is pinned to the reference on that population."""
    inst = ttga.config_instance("med")
    ho, hr = orc.problem(inst), REF.problem(inst)
    P = 96
    s0, r0, _ = ho.random_init(ttga.population_seeds(4242, P))
    seeds = ttga.population_seeds(4343, P)
    a, b = (s0, r0, seeds), (s0, r0, seeds)
    for steps in (200, 1000, 3000):
        a = ho.local_search(*a, steps)
        b = hr.local_search(*b, steps)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), steps
    for x, y in zip(ho.eval(a[0], a[1]), hr.eval(b[0], b[1])):
        assert np.array_equal(x, y)


@needs_ref
@pytest.mark.parametrize("name,steps", [("sm", 200), ("comp01", 200)])
def test_oracle_children_vs_reference_per_child_path(orc, name, steps):
    """The oracle's generation primitives (ga_breed with the 3E discarded draws,
    local_search, eval) equal the reference's own per-child path of
    ga.cpp:543-577 (oracle/_ref ref_ga_children: three RandomInitialSolution,
    two selection5, copies, crossover into a fresh child or copy, mutation,
    localSearch, computePenalty) child for child on the same streams."""
    from ttga.ga import stream_seeds
    inst = ttga.config_instance(name)
    ho, hr = orc.problem(inst), REF.problem(inst)
    N, C = 24, 24
    s, r, g = ho.random_init(stream_seeds(11, 0, N))
    s, r, g = ho.local_search(s, r, g, 100)
    h, sc, f, pen = ho.eval(s, r)
    seeds = stream_seeds(11, N, C)
    cs, cr, fl, rng = ho.ga_breed(s, r, pen, seeds, C, 0.8, 0.5, 1)
    assert (fl & 1).any() and (fl & 1 == 0).any() and (fl & 2).any()     # both crossover and copy children
    cs, cr, rng = ho.local_search(cs, cr, rng, steps)
    exp = dict(zip(("hcv", "scv", "feasible", "penalty"), ho.eval(cs, cr)), slot=cs, room=cr)
    got, grng, _ = hr.ga_children(s, r, pen, seeds, steps, threads=4)
    for k, v in exp.items():
        assert np.array_equal(got[k], v), k
    assert np.array_equal(grng, rng)


@needs_ref
@pytest.mark.parametrize("key", mc.SMALL)
def test_oracle_vs_reference_move3_matrix(orc, key):
    """The Move3 matrix of tests/test_gpu_ls_move3.py on its two small shapes,
    run by the reference's own Solution code: phase-1 and feasible starts, the
    four probability triples. The oracle that checks the GPU there equals the
    reference here."""
    inst = mc.instance(key)
    ho, hr = orc.problem(inst), REF.problem(inst)
    st = mc.starts(ho, key)
    for w in "ab":
        s0, r0 = st[w]
        seeds = mc.run_seeds(key, w, s0.shape[0])
        for p, steps in mc.TRIPLES:
            a = split_rows(ho.local_search, (s0, r0, seeds), steps, *p)
            b = split_rows(hr.local_search, (s0, r0, seeds), steps, *p)
            for x, y in zip(a, b):
                assert np.array_equal(x, y), (w, p)
            assert mc.changed_rows(s0, r0, a[0], a[1]) > 0, (w, p)
