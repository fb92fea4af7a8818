"""What a call of the C ABI may write, and where its buffers may lie.

Every entry point of include/*.h that takes a device buffer runs with all its
arguments carved from one guarded arena (tests/arena.py): payloads of exactly
the documented byte size -- P * E, 4 * P, 8 * P, 4 * P * 7, 4 * E * 45, the
tt_*_work_bytes value, tt_lpt_order's 8 * (n rounded up to a power of two) --
between guards of at least 64 rows, int32 payloads 4-byte aligned and no
better, rng and work payloads 8-byte aligned and no better, uint8 payloads at
a byte skew. After the call every guard and every input equals its snapshot,
the outputs equal the CPU reference the other GPU tests use for that call (the
oracle for the ttga.h calls, the Python models or numpy for the additions) and
the same call on ordinary tensors, and the device status is 0. A call the
header refuses at a shape is in the table with its code and must leave the
whole arena untouched.

Skews (slot, room): the pairs of SKEWS for tt_eval_variant, tt_genome_first
and tt_ga_replace_unique, whose kernels branch on the address (eval_tile5's
LDS-DMA needs 4-byte aligned rows, its and eval_lanes' 16-byte copies 16-byte
aligned ones, eval_corr's two-event loads 2-byte aligned slot and room rows,
row_hash_part splits a row by its address); (0, 0) and (1, 3) for every other
call."""
import ctypes

import numpy as np
import pytest

import ttga
import arena as ar
import cx_model as cm
import greedy_model as gm
import kempe_model as km
import lahc_kempe_model as lkm
import lahc_model as lm
import lahc_multi_model as lmm
import slotswap_model as ssm
from helpers import dev, host
from oracle_lib import oracle

pytestmark = pytest.mark.gpu

import torch  # noqa: E402
from ttga import native  # noqa: E402
from test_gpu_report import ref_event_hcv, ref_parts  # noqa: E402
from test_gpu_unique import build_case, np_first, np_keep, np_source, planted_rows, rand_pop  # noqa: E402

OK, INVALID, LIMIT = native.TT_OK, native.TT_ERR_INVALID, native.TT_ERR_LIMIT

# A: E a multiple of 16 (the DMA, 16-byte and two-event sides exist), two event words with a
#    packed tail, E > 64 (the local search's per-stream redo list);
# B: odd E, rows at every address residue; C: the wide eval path, eight event words;
# D: the 20-event instance of tests/test_gpu_unique.py; W: the walks' models' own "sm" (A has no
#    feasible row: its students make nearly every pair of events clash)
DIMS = {"A": (80, 10, 5, 120), "B": (269, 9, 5, 120), "C": (449, 24, 5, 220), "D": (20, 5, 2, 10)}
GEN_SEED = {"A": 101, "B": 102, "C": 103, "D": 3}
P1, P2 = 131, 67                 # one-pass calls: two full tiles and a tile of 3; searches and walks
SKEWS = [(0, 0), (1, 0), (0, 1), (2, 2), (4, 8), (3, 5)]
TWO_SKEWS = [(0, 0), (1, 3)]
DT = {"uint8": torch.uint8, "int32": torch.int32, "int64": torch.int64, "work": torch.uint8}
KIND = {np.dtype(np.uint8): "uint8", np.dtype(np.int32): "int32", np.dtype(np.int64): "int64"}


# ---------------------------------------------------------------- instances
class Ctx:
    def __init__(self, name):
        self.name = name
        self.inst = lm.SHAPES["sm"]() if name == "W" else ttga.generate(*DIMS[name], seed=GEN_SEED[name])
        self.o = oracle().problem(self.inst)
        self._dp = None
        self.memo = {}

    @property
    def dp(self):
        if self._dp is None:
            self._dp = native.DeviceProblem(self.inst)
        return self._dp


_CTX = {}


def ctx_of(name):
    if name not in _CTX:
        _CTX[name] = Ctx(name)
    return _CTX[name]


# ---------------------------------------------------------------- describing a call
def IN(name, a, group=None):
    a = np.ascontiguousarray(a)
    return (name, "in", KIND[a.dtype], tuple(a.shape), a, group)


def IO(name, a, group=None):
    a = np.ascontiguousarray(a)
    return (name, "inout", KIND[a.dtype], tuple(a.shape), a, group)


def OUT(name, kind, shape, group=None):
    return (name, "out", kind, tuple(shape) if not np.isscalar(shape) else (int(shape),), None, group)


def WORK(name, nbytes):
    """nbytes: the exact size, or a function of the DeviceProblem that gives it."""
    return (name, "work", "work", nbytes, None, None)


class Case:
    """args: the buffers; call(lib, handle, p, stream) -> code, p[name] the buffer's
    address (None for a name that is no buffer); want: {name: expected numpy};
    rc: the code the header promises; extra(tensors, dp): further assertions."""

    def __init__(self, args, call, want, rc=OK, extra=None, needs=None):
        self.args, self.call, self.want, self.rc, self.extra, self.needs = args, call, want, rc, extra, needs


class Ptrs(dict):
    def __missing__(self, key):
        return None


def ptrs(tensors):
    return Ptrs({k: ctypes.c_void_p(t.data_ptr()) for k, t in tensors.items()})


def run(cx, case, skews):
    dp = cx.dp
    lib, h = dp.lib, dp.handle
    if case.needs:
        case.needs(cx.inst, skews)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = [(n, role, kind, (size(dp),) if callable(size) else (size if isinstance(size, tuple) else (int(size),)),
             init, g) for n, role, kind, size, init, g in case.args]
    # the call on ordinary tensors
    plain = {n: (dev(init) if init is not None else torch.full(shape, 0x5B, dtype=DT[kind], device="cuda"))
             for n, role, kind, shape, init, g in args}
    rc = case.call(lib, h, ptrs(plain), st)
    torch.cuda.synchronize()
    assert rc == case.rc, (rc, lib.tt_last_error())
    # the call in the arena
    a = ar.Arena("cuda")
    for n, role, kind, shape, init, g in args:
        skew = 0
        if kind == "uint8":
            skew = skews[0] if (g or ("s" if "slot" in n else "r")) == "s" else skews[1]
        a.add(n, role, kind, shape, init, skew=skew)
    views = a.build()
    for n, role, kind, shape, init, g in args:
        r = a[n]
        assert r.end - r.start == int(np.prod(shape, dtype=np.int64)) * views[n].element_size()
    a.snapshot()
    rc = case.call(lib, h, ptrs(views), st)
    torch.cuda.synchronize()
    assert rc == case.rc, (rc, lib.tt_last_error())
    a.check(untouched=case.rc != OK)
    for n, exp in case.want.items():
        got = host(views[n])
        assert got.shape == exp.shape and got.dtype == exp.dtype, n
        bad = np.flatnonzero((got != exp).reshape(got.shape[0], -1).any(axis=1)) if got.size else []
        assert len(bad) == 0, f"{n} differs from the reference in rows {bad[:8]} (skews {skews})"
        assert np.array_equal(host(plain[n]), exp), f"{n} differs from the reference on ordinary tensors"
    for n, role, kind, shape, init, g in args:
        if role in ("inout", "out") and case.rc == OK:
            assert torch.equal(views[n], plain[n]), f"{n}: the arena's and the ordinary tensors' results differ"
    if case.extra:
        case.extra(views, dp)
        case.extra(plain, dp)
    assert dp.status() == 0


# ---------------------------------------------------------------- inputs shared by the cases of an instance
def memo(cx, key, fn):
    if key not in cx.memo:
        cx.memo[key] = fn()
    return cx.memo[key]


def crowd(cx, slot):
    """On A one row gets a slot of more than 64 events: the searches' redo launch runs."""
    if cx.name == "A":
        idx = np.random.default_rng(5).choice(cx.inst.E, size=70, replace=False)
        slot[3, idx] = 11
    return slot


def rows_p1(cx):
    """P1 rows: random slots, rooms half random, half the oracle's assignRooms."""
    def make():
        inst = cx.inst
        slots, _ = ttga.random_slots(ttga.population_seeds(4242, P1), inst.E)
        slots = crowd(cx, slots)
        rooms = np.random.default_rng(7).integers(0, inst.R, size=(P1, inst.E), dtype=np.uint8)
        rooms[::2] = cx.o.assign_rooms(slots[::2])
        return slots, rooms
    return memo(cx, "rows_p1", make)


def rows_p2(cx):
    """P2 rows from RandomInitialSolution with the oracle's rooms, and their streams."""
    def make():
        s0, _, _ = cx.o.random_init(ttga.population_seeds(606, P2))
        s0 = crowd(cx, s0)
        return s0, cx.o.assign_rooms(s0), ttga.population_seeds(707, P2)
    return memo(cx, "rows_p2", make)


def evaluated(cx, slot, room):
    h, s, f, p = cx.o.eval(slot, room)
    return dict(hcv=h, scv=s, feasible=f, penalty=p)


# ---------------------------------------------------------------- ttga.h
def eval_case(cx, variant):
    """variant None: tt_eval."""
    slot, room = rows_p1(cx)
    E = cx.inst.E
    args = [IN("slot", slot), IN("room", room), OUT("hcv", "int32", P1), OUT("scv", "int32", P1),
            OUT("feasible", "uint8", P1), OUT("penalty", "int32", P1)]
    if variant is None:
        def call(lib, h, p, st):
            return lib.tt_eval(h, p["slot"], p["room"], P1, p["hcv"], p["scv"], p["feasible"], p["penalty"], st)
    else:
        def call(lib, h, p, st):
            return lib.tt_eval_variant(h, p["slot"], p["room"], P1, p["hcv"], p["scv"], p["feasible"], p["penalty"],
                                       variant, st)
    # ttga.h: 7/8 = eval_tile5, E <= 448; 13 = the wide path, E <= 2491; 2 = any E
    refused = variant is not None and (variant & 15) in (7, 8) and E > 448
    want = {} if refused else memo(cx, "eval", lambda: evaluated(cx, slot, room))

    def needs(inst, skews):
        # the sides of the address branches these skews reach at this instance
        if cx.name == "A":
            assert inst.E % 16 == 0 and inst.E % 4 == 0 and inst.E % 2 == 0
        if cx.name == "B":
            assert inst.E % 2 == 1
    return Case(args, call, want, rc=LIMIT if refused else OK, needs=needs)


def assign_rooms_case(cx):
    slot, _ = rows_p1(cx)
    return Case([IN("slot", slot), OUT("room", "uint8", slot.shape)],
                lambda lib, h, p, st: lib.tt_assign_rooms(h, p["slot"], p["room"], P1, st),
                {"room": memo(cx, "assign", lambda: cx.o.assign_rooms(slot))})


def random_init_case(cx):
    seeds = ttga.population_seeds(1234, P1)
    s, r, g = memo(cx, "random_init", lambda: cx.o.random_init(seeds))
    E = cx.inst.E
    return Case([IO("rng", seeds), OUT("slot", "uint8", (P1, E)), OUT("room", "uint8", (P1, E))],
                lambda lib, h, p, st: lib.tt_random_init(h, p["rng"], p["slot"], p["room"], P1, st),
                {"slot": s, "room": r, "rng": g})


def crossover_case(cx):
    E = cx.inst.E
    s1, _ = ttga.random_slots(ttga.population_seeds(11, P1), E)
    s2, _ = ttga.random_slots(ttga.population_seeds(12, P1), E)
    seeds = ttga.population_seeds(13, P1)
    s, r, g = memo(cx, "crossover", lambda: cx.o.crossover(s1, s2, seeds))
    return Case([IN("slot1", s1), IN("slot2", s2), IO("rng", seeds), OUT("slot", "uint8", (P1, E)),
                 OUT("room", "uint8", (P1, E))],
                lambda lib, h, p, st: lib.tt_crossover(h, p["slot1"], p["slot2"], p["rng"], p["slot"], p["room"], P1, st),
                {"slot": s, "room": r, "rng": g})


def mutation_case(cx):
    slot, _ = rows_p1(cx)
    room = memo(cx, "assign", lambda: cx.o.assign_rooms(slot))
    seeds = ttga.population_seeds(14, P1)
    s, r, g = memo(cx, "mutation", lambda: cx.o.mutation(slot, room, seeds))
    return Case([IO("slot", slot), IO("room", room), IO("rng", seeds)],
                lambda lib, h, p, st: lib.tt_mutation(h, p["slot"], p["room"], p["rng"], P1, st),
                {"slot": s, "room": r, "rng": g})


LS_STEPS = 300


def local_search_case(cx, form):
    """form: "plain" tt_local_search, "ordered" tt_local_search_ordered, "eval" and
    "eval_order" tt_local_search_eval without and with an order."""
    s0, r0, seeds = rows_p2(cx)
    if cx.name == "A":
        assert cx.inst.E > 64 and np.bincount(s0[3], minlength=45).max() > 64      # the redo launch runs

    def ref():
        s, r, g = cx.o.local_search(s0, r0, seeds, LS_STEPS)
        return dict(slot=s, room=r, rng=g, **evaluated(cx, s, r))
    want = memo(cx, "local_search", ref)
    args = [IO("slot", s0), IO("room", r0), IO("rng", seeds)]
    order = np.random.default_rng(3).permutation(P2).astype(np.int32)
    if form in ("ordered", "eval_order"):
        args.append(IN("order", order))
    if form in ("eval", "eval_order"):
        args += [OUT("hcv", "int32", P2), OUT("scv", "int32", P2), OUT("feasible", "uint8", P2),
                 OUT("penalty", "int32", P2)]
    else:
        want = {k: want[k] for k in ("slot", "room", "rng")}

    def call(lib, h, p, st):
        if form == "plain":
            return lib.tt_local_search(h, p["slot"], p["room"], p["rng"], P2, LS_STEPS, 1.0, 1.0, 0.0, st)
        if form == "ordered":
            return lib.tt_local_search_ordered(h, p["slot"], p["room"], p["rng"], P2, LS_STEPS, 1.0, 1.0, 0.0,
                                               p["order"], st)
        return lib.tt_local_search_eval(h, p["slot"], p["room"], p["rng"], P2, LS_STEPS, 1.0, 1.0, 0.0, p["order"],
                                        p["hcv"], p["scv"], p["feasible"], p["penalty"], st)
    return Case(args, call, want)


def parents(cx):
    """A population of P2 evaluated random rows."""
    def make():
        s, r, _ = cx.o.random_init(ttga.population_seeds(21, P2))
        return s, r, cx.o.eval(s, r)[3]
    return memo(cx, "parents", make)


def ga_breed_case(cx):
    ps, pr, pen = parents(cx)
    E, C = cx.inst.E, P1
    seeds = ttga.population_seeds(22, C)
    cs, cr, fl, g = memo(cx, "ga_breed", lambda: cx.o.ga_breed(ps, pr, pen, seeds, C, 0.8, 0.5, 1))
    assert (fl & 1).any() and (fl & 2).any() and not (fl & 2).all()
    return Case([IN("pop_slot", ps), IN("pop_room", pr), IN("pop_penalty", pen), IO("rng", seeds),
                 OUT("child_slot", "uint8", (C, E)), OUT("child_room", "uint8", (C, E)), OUT("child_flags", "uint8", C)],
                lambda lib, h, p, st: lib.tt_ga_breed(h, p["pop_slot"], p["pop_room"], p["pop_penalty"], P2, p["rng"], C,
                                                      0.8, 0.5, 1, p["child_slot"], p["child_room"], p["child_flags"],
                                                      st),
                {"child_slot": cs, "child_room": cr, "child_flags": fl, "rng": g})


def pow2_at_least(n):
    return 1 << max(int(n) - 1, 0).bit_length()


def lpt_order_case(cx, n):
    key = np.random.default_rng(n).integers(-1, 30, n).astype(np.int32)
    hi = np.where(key < 0, np.int64(2 ** 32), np.int64(2 ** 31 - 1) - key.astype(np.int64))
    exp = np.lexsort((np.arange(n), hi)).astype(np.int32)
    return Case([IN("key", key), OUT("order", "int32", n), WORK("work", 8 * pow2_at_least(n))],
                lambda lib, h, p, st: lib.tt_lpt_order(h, p["key"], n, p["order"], p["work"], st), {"order": exp})


KEYS = ("slot", "room", "hcv", "scv", "feasible", "penalty")
POP_KIND = {"slot": "s", "room": "r", "feasible": "r"}


def replace_inputs(cx, N, C):
    def make():
        rng = np.random.default_rng(N * 7 + C)
        if C == 0:                                       # no order to rely on: the initial sort
            pop = rand_pop(rng, N, cx.inst)
            return pop, {k: v[:0] for k, v in pop.items()}
        return build_case(rng, cx.inst, N, C, "best" if C <= 8192 else "childdup")
    return memo(cx, ("replace_inputs", N, C), make)


def source_word(cx, N, want):
    def extra(t, dp):
        off = int(dp.lib.tt_ga_work_source_offset(N, cx.inst.E))
        assert 0 < off and off + 4 <= t["work"].numel()
        assert int(host(t["work"][off:off + 4].clone().view(torch.int32))[0]) == want
    return extra


def ga_replace_case(cx, N, C):
    pop, ch = replace_inputs(cx, N, C)
    exp = memo(cx, ("replace", N, C), lambda: cx.o.ga_replace(pop, ch))
    pen = np.concatenate([pop["penalty"][:N - C], ch["penalty"]]).astype(np.uint32)
    src = int(np.lexsort((np.arange(N), pen))[0])                             # the merged position of the new pop[0]
    args = [IO("pop_" + k, pop[k], POP_KIND.get(k)) for k in KEYS] + [IN("child_" + k, ch[k], POP_KIND.get(k)) for k in KEYS]
    args.append(WORK("work", lambda dp: int(dp.lib.tt_ga_work_bytes(N, dp.E))))

    def call(lib, h, p, st):
        return lib.tt_ga_replace(h, *(p["pop_" + k] for k in KEYS), N, *(p["child_" + k] for k in KEYS), C, p["work"], st)
    return Case(args, call, {"pop_" + k: exp[k] for k in KEYS}, extra=source_word(cx, N, src))


def ga_replace_unique_case(cx, N, C):
    pop, ch = replace_inputs(cx, N, C)

    def ref():
        keep = np_keep(pop, ch) if C else np.zeros(0, bool)
        return keep, cx.o.ga_replace(pop, {k: v[keep] for k, v in ch.items()}), np_source(pop, ch, keep)
    keep, exp, src = memo(cx, ("replace_unique", N, C), ref)
    if C:
        assert 0 < keep.sum() < C                                            # children kept and children dropped
    args = [IO("pop_" + k, pop[k], POP_KIND.get(k)) for k in KEYS] + [IN("child_" + k, ch[k], POP_KIND.get(k)) for k in KEYS]
    if C:
        args.append(OUT("keep", "uint8", C, "r"))
    args += [OUT("n_kept", "int32", 1), WORK("work", lambda dp: int(dp.lib.tt_ga_unique_work_bytes(N, C, dp.E)))]

    def call(lib, h, p, st):
        return lib.tt_ga_replace_unique(h, *(p["pop_" + k] for k in KEYS), N, *(p["child_" + k] for k in KEYS), C,
                                        p["keep"], p["n_kept"], 0, p["work"], st)
    want = {"pop_" + k: exp[k] for k in KEYS}
    want["n_kept"] = np.array([int(keep.sum())], np.int32)
    if C:
        want["keep"] = keep.astype(np.uint8)
    return Case(args, call, want, extra=source_word(cx, N, src))


def genome_first_case(cx):
    P = 300
    slot, room, _ = memo(cx, "planted", lambda: planted_rows(np.random.default_rng(2003), P, cx.inst.E, cx.inst.R))
    exp = np_first(slot, room)
    assert 0 < (exp != np.arange(P)).sum()
    return Case([IN("slot", slot), IN("room", room), OUT("first", "int32", P),
                 WORK("work", lambda dp: int(dp.lib.tt_genome_work_bytes(P, dp.E)))],
                lambda lib, h, p, st: lib.tt_genome_first(h, p["slot"], p["room"], P, p["first"], 0, p["work"], st),
                {"first": exp})


# ---------------------------------------------------------------- ttga_report.h
def eval_parts_case(cx):
    """On the first P2 rows (one full tile and a tile of 3): the reference takes 50 ms a row at C."""
    slot, room = (x[:P2] for x in rows_p1(cx))
    E, P1 = cx.inst.E, P2
    parts = memo(cx, "parts", lambda: ref_parts(cx.inst, slot, room))
    eh = memo(cx, "event_hcv", lambda: ref_event_hcv(cx.inst, slot, room))
    return Case([IN("slot", slot), IN("room", room), OUT("parts", "int32", (P1, 6)), OUT("event_hcv", "int32", (P1, E))],
                lambda lib, h, p, st: lib.tt_eval_parts(h, p["slot"], p["room"], P1, p["parts"], p["event_hcv"], st),
                {"parts": parts, "event_hcv": eh})


def slot_histogram_case(cx):
    slot, _ = rows_p1(cx)
    E = cx.inst.E
    hist = np.stack([np.bincount(slot[:, e], minlength=45)[:45] for e in range(E)]).astype(np.int32)
    return Case([IN("slot", slot), OUT("hist", "int32", (E, 45))],
                lambda lib, h, p, st: lib.tt_slot_histogram(h, p["slot"], P1, p["hist"], st), {"hist": hist})


# ---------------------------------------------------------------- ttga_greedy.h, ttga_cx.h
def greedy_order_case(cx):
    E = cx.inst.E
    return Case([OUT("order", "int32", E), WORK("work", lambda dp: int(dp.lib.tt_greedy_work_bytes(dp.handle)))],
                lambda lib, h, p, st: lib.tt_greedy_order(h, p["order"], p["work"], st),
                {"order": memo(cx, "greedy_order", lambda: gm.greedy_order(cx.inst))})


def greedy_init_case(cx):
    E = cx.inst.E
    order = memo(cx, "greedy_order", lambda: gm.greedy_order(cx.inst))
    seeds = ttga.population_seeds(31, P1)

    def ref():
        s, g = gm.greedy_slots(cx.inst, order, seeds)
        return s, cx.o.assign_rooms(s), g
    s, r, g = memo(cx, "greedy_init", ref)
    return Case([IN("order", order), IO("rng", seeds), OUT("slot", "uint8", (P1, E)), OUT("room", "uint8", (P1, E))],
                lambda lib, h, p, st: lib.tt_greedy_init(h, p["order"], p["rng"], p["slot"], p["room"], P1, st),
                {"slot": s, "room": r, "rng": g})


def crossover_guided_case(cx):
    E = cx.inst.E
    order = memo(cx, "greedy_order", lambda: gm.greedy_order(cx.inst))
    s1, _ = ttga.random_slots(ttga.population_seeds(41, P1), E)
    s2, _ = ttga.random_slots(ttga.population_seeds(42, P1), E)
    seeds = ttga.population_seeds(43, P1)

    def ref():
        s, g, c, n = cm.guided_slots(cx.inst, order, s1, s2, seeds, 1)
        return s, cx.o.assign_rooms(s), g, c, n
    s, r, g, c, n = memo(cx, "crossover_guided", ref)
    assert n.any()
    return Case([IN("slot1", s1), IN("slot2", s2), IN("order", order), IO("rng", seeds), OUT("slot", "uint8", (P1, E)),
                 OUT("room", "uint8", (P1, E)), OUT("cost", "int32", P1), OUT("repaired", "int32", P1)],
                lambda lib, h, p, st: lib.tt_crossover_guided(h, p["slot1"], p["slot2"], p["order"], p["rng"], p["slot"],
                                                              p["room"], P1, 1, p["cost"], p["repaired"], st),
                {"slot": s, "room": r, "rng": g, "cost": c, "repaired": n})


def ga_breed_guided_case(cx):
    ps, pr, pen = parents(cx)
    E, C = cx.inst.E, P1
    order = memo(cx, "greedy_order", lambda: gm.greedy_order(cx.inst))
    seeds = ttga.population_seeds(44, C)
    cs, cr, fl, g, cost, rep = memo(cx, "ga_breed_guided",
                                    lambda: cm.breed(cx.inst, cx.o, order, ps, pr, pen, seeds, 0.8, 0.5, 1, 1))
    return Case([IN("pop_slot", ps), IN("pop_room", pr), IN("pop_penalty", pen), IN("order", order), IO("rng", seeds),
                 OUT("child_slot", "uint8", (C, E)), OUT("child_room", "uint8", (C, E)), OUT("child_flags", "uint8", C),
                 OUT("child_cost", "int32", C), OUT("child_repaired", "int32", C)],
                lambda lib, h, p, st: lib.tt_ga_breed_guided(h, p["pop_slot"], p["pop_room"], p["pop_penalty"], P2,
                                                             p["order"], p["rng"], C, 0.8, 0.5, 1, 1, p["child_slot"],
                                                             p["child_room"], p["child_flags"], p["child_cost"],
                                                             p["child_repaired"], st),
                {"child_slot": cs, "child_room": cr, "child_flags": fl, "rng": g, "child_cost": cost,
                 "child_repaired": rep})


# ---------------------------------------------------------------- ttga_kempe.h, ttga_slotswap.h
def kempe_move_case(cx):
    s0, r0, seeds = rows_p2(cx)

    def ref():
        ws, wg, wl, pairs = km.kempe_rows(cx.inst, s0, seeds, 1.0, 0, room=r0)
        return ws, km.expected_rooms(cx.o, ws, r0, wl, pairs), wg, wl
    s, r, g, cl = memo(cx, "kempe", ref)
    assert (cl >= 1).all()
    return Case([IO("slot", s0), IO("room", r0), IO("rng", seeds), OUT("chain_len", "int32", P2)],
                lambda lib, h, p, st: lib.tt_kempe_move(h, p["slot"], p["room"], p["rng"], P2, 1.0, 0, p["chain_len"], st),
                {"slot": s, "room": r, "rng": g, "chain_len": cl})


SWAP_PASSES = 3


def slot_swap_case(cx):
    s0, r0, _ = rows_p2(cx)
    before = evaluated(cx, s0, r0)

    def ref():
        rows, gain, passes, perm = ssm.descend_rows(cx.inst, s0, SWAP_PASSES, deltas=ssm.deltas_windows)
        return rows, gain, passes, perm, evaluated(cx, rows, r0)
    rows, gain, passes, perm, after = memo(cx, "slot_swap", ref)
    assert passes.max() == SWAP_PASSES and np.array_equal(after["scv"], before["scv"] - gain)
    return Case([IO("slot", s0), IO("scv", before["scv"]), IO("penalty", before["penalty"]), OUT("gain", "int32", P2),
                 OUT("passes", "int32", P2), OUT("perm", "uint8", (P2, 45), "s")],
                lambda lib, h, p, st: lib.tt_slot_swap(h, p["slot"], P2, SWAP_PASSES, p["scv"], p["penalty"], p["gain"],
                                                       p["passes"], p["perm"], st),
                {"slot": rows, "scv": after["scv"], "penalty": after["penalty"], "gain": gain.astype(np.int32),
                 "passes": passes.astype(np.int32), "perm": perm.astype(np.uint8)})


# ---------------------------------------------------------------- ttga_lahc*.h
WALK_STEPS, WALK_L = 300, 50
MULTI_STEPS = 150


def walk_rows(cx):
    def make():
        model = lmm.Model(cx.inst)                       # tt_lahc's, the augmenting walk's and the walkers' model
        slot, room, seeds = lm.population(cx.inst, P2, model)
        ev = evaluated(cx, slot, room)
        assert 2 * int((ev["hcv"] == 0).sum()) >= P2 and (ev["hcv"] != 0).any()      # open and closed rows
        return model, slot, room, seeds, ev
    return memo(cx, "walk_rows", make)


def walk_case(cx, kind, K=None):
    model, slot, room, seeds, ev = walk_rows(cx)
    names = ["slot", "room", "rng", "gain", "accepted", "best_step"]
    args = [IO("slot", slot), IO("room", room), IO("rng", seeds), IO("scv", ev["scv"]), IO("penalty", ev["penalty"]),
            OUT("gain", "int32", P2), OUT("accepted", "int32", P2), OUT("best_step", "int32", P2)]
    if kind == "lahc":
        ref = lambda: model.lahc_rows(slot, room, seeds, WALK_STEPS, WALK_L, 0.5)                        # noqa: E731

        def call(lib, h, p, st):
            return lib.tt_lahc(h, p["slot"], p["room"], p["rng"], P2, WALK_STEPS, WALK_L, 0.5, p["scv"], p["penalty"],
                               p["gain"], p["accepted"], p["best_step"], st)
    elif kind == "kempe":
        names.append("kempe_stats")
        args.append(OUT("kempe_stats", "int32", (P2, 5)))
        ref = lambda: lkm.Model(cx.inst).lahc_kempe_rows(slot, room, seeds, WALK_STEPS, WALK_L, 0.25, 0.5, 0)         # noqa: E731

        def call(lib, h, p, st):
            return lib.tt_lahc_kempe(h, p["slot"], p["room"], p["rng"], P2, WALK_STEPS, WALK_L, 0.25, 0.5, 0, p["scv"],
                                     p["penalty"], p["gain"], p["accepted"], p["best_step"], p["kempe_stats"], st)
    elif kind == "aug":
        names.append("kempe_stats")
        args.append(OUT("kempe_stats", "int32", (P2, 7)))
        ref = lambda: model.lahc_kempe_aug_rows(slot, room, seeds, WALK_STEPS, WALK_L, 0.25, 0.5, 0, 1)  # noqa: E731

        def call(lib, h, p, st):
            return lib.tt_lahc_kempe_aug(h, p["slot"], p["room"], p["rng"], P2, WALK_STEPS, WALK_L, 0.25, 0.5, 0, 1,
                                         p["scv"], p["penalty"], p["gain"], p["accepted"], p["best_step"],
                                         p["kempe_stats"], st)
    else:
        names += ["kempe_stats", "winner", "walker_gain"]
        args += [OUT("kempe_stats", "int32", (P2, 7)), OUT("winner", "int32", P2), OUT("walker_gain", "int32", (P2, K)),
                 WORK("work", lambda dp: int(dp.lib.tt_lahc_multi_work_bytes(dp.handle, P2, K)))]
        ref = lambda: model.lahc_multi_rows(slot, room, seeds, K, MULTI_STEPS, WALK_L, 0.25, 0.5, 0, 1)  # noqa: E731

        def call(lib, h, p, st):
            return lib.tt_lahc_multi(h, p["slot"], p["room"], p["rng"], P2, K, MULTI_STEPS, WALK_L, 0.25, 0.5, 0, 1,
                                     p["scv"], p["penalty"], p["gain"], p["accepted"], p["best_step"], p["kempe_stats"],
                                     p["winner"], p["walker_gain"], p["work"], st)
    out = memo(cx, ("walk", kind, K), ref)
    want = dict(zip(names, out))
    assert want["gain"].any()
    after = evaluated(cx, want["slot"], want["room"])
    assert np.array_equal(after["scv"], ev["scv"] - want["gain"])
    want["scv"], want["penalty"] = after["scv"], after["penalty"]
    return Case(args, call, want)


# ---------------------------------------------------------------- the table
EVAL_VARIANTS = {"v2": 2, "v7": 7, "v8": 8, "v8_one_tile": 8 | (128 << 4), "v8_persistent": 8 | (64 << 4), "v13": 13}

# call id -> (instances, builder); every one runs at TWO_SKEWS
CALLS = {
    "tt_eval": ("ABC", lambda cx: eval_case(cx, None)),
    "tt_assign_rooms": ("ABC", assign_rooms_case),
    "tt_random_init": ("ABC", random_init_case),
    "tt_crossover": ("ABC", crossover_case),
    "tt_mutation": ("ABC", mutation_case),
    "tt_local_search": ("ABC", lambda cx: local_search_case(cx, "plain")),
    "tt_local_search_ordered": ("ABC", lambda cx: local_search_case(cx, "ordered")),
    "tt_local_search_eval": ("ABC", lambda cx: local_search_case(cx, "eval")),
    "tt_local_search_eval-order": ("ABC", lambda cx: local_search_case(cx, "eval_order")),
    "tt_ga_breed": ("ABC", ga_breed_case),
    "tt_eval_parts": ("ABC", eval_parts_case),
    "tt_slot_histogram": ("ABC", slot_histogram_case),
    "tt_lpt_order-200": ("A", lambda cx: lpt_order_case(cx, 200)),          # one 256-key bitonic sort
    "tt_lpt_order-300": ("A", lambda cx: lpt_order_case(cx, 300)),          # 512 keys: two rank tiles
    "tt_lpt_order-600": ("A", lambda cx: lpt_order_case(cx, 600)),          # 1,024 keys: four rank tiles
    "tt_ga_replace-300-130": ("D", lambda cx: ga_replace_case(cx, 300, 130)),
    "tt_ga_replace-600-300": ("D", lambda cx: ga_replace_case(cx, 600, 300)),
    "tt_ga_replace-300-0": ("D", lambda cx: ga_replace_case(cx, 300, 0)),
    "tt_ga_replace-9000-8500": ("D", lambda cx: ga_replace_case(cx, 9000, 8500)),
    "tt_greedy_order": ("A", greedy_order_case),
    "tt_greedy_init": ("A", greedy_init_case),
    "tt_kempe_move": ("A", kempe_move_case),
    "tt_slot_swap": ("A", slot_swap_case),
    "tt_lahc": ("W", lambda cx: walk_case(cx, "lahc")),
    "tt_lahc_kempe": ("W", lambda cx: walk_case(cx, "kempe")),
    "tt_lahc_kempe_aug": ("W", lambda cx: walk_case(cx, "aug")),
    "tt_lahc_multi-K1": ("W", lambda cx: walk_case(cx, "multi", 1)),
    "tt_lahc_multi-K5": ("W", lambda cx: walk_case(cx, "multi", 5)),
    "tt_crossover_guided": ("A", crossover_guided_case),
    "tt_ga_breed_guided": ("A", ga_breed_guided_case),
}
# the calls whose kernels branch on the address: every pair of SKEWS
SKEWED = {f"tt_eval_variant-{k}": ("ABC", (lambda v: lambda cx: eval_case(cx, v))(v)) for k, v in EVAL_VARIANTS.items()}
SKEWED["tt_genome_first"] = ("D", genome_first_case)
for _n, _c in ((300, 130), (600, 300), (300, 0), (9000, 8500)):
    SKEWED[f"tt_ga_replace_unique-{_n}-{_c}"] = ("D", (lambda n, c: lambda cx: ga_replace_unique_case(cx, n, c))(_n, _c))


def expand(table, skews):
    return [pytest.param(i, cid, sk, id=f"{i}-{cid}-s{sk[0]}r{sk[1]}") for cid, (insts, _) in table.items()
            for i in insts for sk in skews]


def built(table, inst, cid):
    cx = ctx_of(inst)
    return cx, memo(cx, ("case", cid), lambda: table[cid][1](cx))


@pytest.mark.parametrize("inst,cid,skews", expand(SKEWED, SKEWS))
def test_address_branches(inst, cid, skews):
    cx, case = built(SKEWED, inst, cid)
    run(cx, case, skews)


@pytest.mark.parametrize("inst,cid,skews", expand(CALLS, TWO_SKEWS))
def test_footprint(inst, cid, skews):
    cx, case = built(CALLS, inst, cid)
    run(cx, case, skews)


def test_every_entry_point_is_in_the_table():
    """Every function of include/*.h with a device buffer among its arguments."""
    import pathlib
    import re
    inc = pathlib.Path(__file__).resolve().parent.parent / "include"
    names = set()
    for hdr in inc.glob("*.h"):
        names |= set(re.findall(r"^int (tt_\w+)\(", hdr.read_text(), flags=re.M))
    host_only = {"tt_problem_create", "tt_problem_destroy", "tt_problem_dims", "tt_problem_derived",
                 "tt_eval_auto_variant", "tt_local_search_stats", "tt_local_search_masks", "tt_device_status",
                 "tt_version"}
    listed = {cid.split("-")[0] for cid in list(CALLS) + list(SKEWED)}
    assert names - host_only == listed, (names - host_only) ^ listed
