"""Every entry point on populations whose [P][E] buffers pass 2^31 and 2^32
bytes, by the periodic check of tests/large_rows.py: the population repeats a
base block of M = 4,099 distinct rows (each with its own rng seed), so every
per-row output of the big call must have period M and equal the same entry
point's output at P = M on fresh small buffers -- and that small call is
compared here with the CPU oracle (257 rows) or the stage's Python model (16
rows). P = ceil(2^32 / E) + M + 3: one full period past the 2^32-byte line, a
partial last tile, the 2^31 line inside. Out-of-place outputs start as a
sentinel no call produces; inputs are checked to be unchanged.

Instances: L448 = generate(448, 10, 5, 150, seed=12) (eval_tile5 with 4 and 8
waves, second tile buffer, persistent grid; P = 9,591,083) and L2000 =
generate(2000, 24, 5, 300, seed=12) (the wide eval path, the bucket parts
kernel, the wide matcher; P = 2,151,586). The stages with one instance run on
L448, where a row costs least; L2000 has more events than cells, so no row of
it is feasible and the walks would meet their gate only. tt_crossover stops
at 1,280 events (ttga.h): on L2000 the large call must be TT_ERR_LIMIT and
touch nothing.

Entry points that look across rows have an exact expectation from the period:
tt_slot_histogram (k times the block's histogram plus that of its first rem
rows), tt_genome_first (first[i] = i mod M) and tt_ga_replace (ascending
penalties, the multiset ttga.h states -- the survivors 0 .. N-C-1 of a sorted
population and the children --, and a fresh tt_eval of every row).

The launch limit: HIP runs no launch of more than 2^32 - 1 threads in full.
It reports success and runs the count modulo 2^32 (or refuses an exact
multiple of 2^32), so a call that gives every row a workgroup refuses more
rows than fit with TT_ERR_LIMIT and touches nothing: test_launch_limit (256
threads a row), test_launch_limit_one_wave (64) and test_genome_first_bound
(16), all at E = 3, each at its bound and just past it.

Left out on purpose: tt_ga_breed* with N * E past 2^31 (a child depends on
indices drawn over N, which no small call reproduces; here N = 64 and C * E
passes 2^32) and tt_ga_replace_unique with large N (a periodic population is
all duplicates by construction).

Every case prints its instance, P, peak device memory and wall time
("LARGE_ROWS ..." lines, pytest -s)."""
import contextlib
import ctypes
import gc
import time
import types

import numpy as np
import pytest

import cx_model as cx
import greedy_model as gm
import kempe_model as km
import lahc_kempe_aug_model as am
import lahc_model as lm
import lahc_multi_model as mm
import large_rows as lr
import slotswap_model as sm
import ttga
from helpers import dev, host
from oracle_lib import oracle, split_rows
from ttga import validate

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from ttga import native  # noqa: E402

M = lr.M_ROWS
LINE = 1 << 32
U8_FILL, I32_FILL = 0xEE, -77                       # no slot, room, flag, count or score
ORACLE_ROWS = np.arange(0, M, 16)                   # 257 rows of the base block for the C++ oracle
MODEL_ROWS = np.linspace(0, M - 1, 16).astype(np.int64)     # 16 for the Python models
MAX_BYTES = 24 << 30
INSTANCES = {"L448": lambda: ttga.generate(448, 10, 5, 150, seed=12),
             "L2000": lambda: ttga.generate(2000, 24, 5, 300, seed=12)}
EVAL_NAMES = ("hcv", "scv", "feasible", "penalty")


# ---------------------------------------------------------------- buffers and the frame of a case
def u8(*shape):
    return torch.full(shape, U8_FILL, dtype=torch.uint8, device="cuda")


def i32(*shape):
    return torch.full(shape, I32_FILL, dtype=torch.int32, device="cuda")


def eval_out(n):
    return i32(n), i32(n), u8(n), i32(n)


def tile(base, P):
    return lr.tile_rows(base if torch.is_tensor(base) else dev(base), P)


def periodic(what, **pairs):
    """name=(big, base): every row of big equals its base row."""
    for name, (big, base) in pairs.items():
        lr.assert_periodic(big, base if torch.is_tensor(base) else dev(base), f"{what}: {name}")


def same(what, want, got, rows=None):
    """Device tensors (or arrays) against the judge's arrays, on `rows` of them."""
    for name, w in want.items():
        g = got[name]
        g = host(g) if torch.is_tensor(g) else g
        g = g if rows is None else g[rows]
        bad = np.flatnonzero((g.reshape(len(g), -1) != np.asarray(w).reshape(len(g), -1)).any(axis=1))
        assert bad.size == 0, f"{what}: {name} differs from the judge in {bad.size} rows, first {bad[:8]}"


@contextlib.contextmanager
def case(what, name, P, nbytes):
    """Skips without the memory, times the case and reports its peak."""
    lr.need_device_memory(nbytes)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    dt, peak = time.perf_counter() - t0, torch.cuda.max_memory_allocated()
    print(f"\nLARGE_ROWS case={what} instance={name} P={P} peak_GiB={peak / 2 ** 30:.2f} seconds={dt:.2f}")
    assert peak <= MAX_BYTES, f"{what}: {peak} bytes of device memory at once"


@pytest.fixture(autouse=True)
def free_between_cases():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                       # a device error is sticky: nothing more runs on this device
        pytest.exit(f"device error, the module stops here: {e}", returncode=3)
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def ctx():
    """Per instance: the handle, the oracle, the base block (random rows with
    assigned rooms from tt_random_init at P = M, their seeds and scores) and, on
    demand, the walk block (tt_greedy_init and 200 steps of local search)."""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        inst = INSTANCES[name]()
        c = types.SimpleNamespace(name=name, inst=inst, E=inst.E, dp=native.DeviceProblem(inst),
                                  o=oracle().problem(inst), seeds=mm_seeds(M))
        g, s, r = dev(c.seeds), u8(M, inst.E), u8(M, inst.E)
        c.dp.random_init(g, s, r)
        c.slot, c.room, c.rng = host(s), host(r), host(g)
        assert len({row.tobytes() for row in c.slot}) == M and len(set(c.seeds.tolist())) == M
        c.scores = [host(t) for t in c.dp.eval(s, r, out=eval_out(M))]
        same(f"{name} base eval", dict(zip(EVAL_NAMES, c.o.eval(c.slot[ORACLE_ROWS], c.room[ORACLE_ROWS]))),
             dict(zip(EVAL_NAMES, c.scores)), ORACLE_ROWS)
        c.P = lr.rows_past(LINE, inst.E)
        assert c.P * inst.E >= LINE + M * inst.E and c.P % 64 and (1 << 31) < c.P * inst.E
        cache[name] = c
        return c
    return get


def mm_seeds(n, base=1):
    from mutation_model import spread_seeds
    return spread_seeds(n, base)


def walk_block(c):
    """tt_greedy_init + 200 steps of tt_local_search at P = M: mostly feasible rows."""
    if not hasattr(c, "walk"):
        g, s, r = dev(mm_seeds(M, 7001)), u8(M, c.E), u8(M, c.E)
        c.dp.greedy_init(g, s, r)
        out = eval_out(M)
        c.dp.local_search(s, r, g, 200, out=out)
        c.walk = types.SimpleNamespace(slot=host(s), room=host(r), rng=host(g), scores=[host(t) for t in out])
        assert len({row.tobytes() for row in c.walk.slot}) == M
    return c.walk


both = pytest.mark.parametrize("name", ["L448", "L2000"])


# ---------------------------------------------------------------- tt_eval, tt_eval_parts
@pytest.mark.parametrize("name,variant", [("L448", v) for v in (0, 7, 8, 8 | 64 << 4, 8 | 128 << 4, 2)] +
                         [("L2000", 13), ("L2000", 2)])
def test_eval(ctx, name, variant):
    c = ctx(name)
    with case(f"tt_eval_variant_{variant}", name, c.P, 2 * c.P * c.E):
        bs, br = dev(c.slot), dev(c.room)
        base = c.dp.eval(bs, br, variant=variant, out=eval_out(M))
        same("base", dict(zip(EVAL_NAMES, c.scores)), dict(zip(EVAL_NAMES, base)))      # = the oracle-checked scores
        s, r = tile(bs, c.P), tile(br, c.P)
        assert s.numel() >= LINE and s.data_ptr() % 16 == 0
        out = c.dp.eval(s, r, variant=variant, out=eval_out(c.P))
        periodic("tt_eval", slot=(s, bs), room=(r, br), **{n: (g, b) for n, g, b in zip(EVAL_NAMES, out, base)})


def raw_parts(dp, s, r, parts, eh):
    native._check(dp.lib, dp.lib.tt_eval_parts(dp.handle, s.data_ptr(), r.data_ptr(), s.shape[0], parts.data_ptr(),
                                               ctypes.c_void_p(eh.data_ptr() if eh is not None else None),
                                               dp._stream(s)))


def ref_parts(inst, slots, rooms):
    """[rows, 6] in PART_NAMES' order, from the definitions ttga.validate states
    (validate.evaluate itself takes 8 s a row at 2,000 events: its int64 matrix
    products are done once here, in float32, exact at these counts). Row 0 is
    also asked of validate.evaluate where that is quick (E < 1,000)."""
    A = inst.student_events.astype(np.float32)
    E, R = inst.E, inst.R
    corr = np.triu((A.T @ A) > 0, k=1)
    sn, possible, ev = A.sum(axis=0).astype(np.int64), inst.possible_rooms(), np.arange(E)
    out = []
    for t, r in zip(np.asarray(slots, np.int64), np.asarray(rooms, np.int64)):
        cells = np.bincount(t * R + r, minlength=45 * R)
        X = np.zeros((E, 45), np.float32)
        X[ev, t] = 1
        days = ((A @ X) > 0).reshape(inst.S, 5, 9)
        out.append([int((cells * (cells - 1) // 2).sum()), int(((t[:, None] == t[None, :]) & corr).sum()),
                    int((possible[ev, r] == 0).sum()), int(sn[t % 9 == 8].sum()),
                    int((days[:, :, :-2] & days[:, :, 1:-1] & days[:, :, 2:]).sum()), int((days.sum(axis=2) == 1).sum())])
    if E < 1000 and len(out):
        assert out[0] == [validate.evaluate(inst, slots[0], rooms[0])[k] for k in native.PART_NAMES]
    return np.array(out, np.int32).reshape(-1, 6)


def ref_event_hcv(inst, slots, rooms):
    """Solution::eventHcv: the other events of e's slot in e's room + those correlated with e."""
    A = inst.student_events.astype(np.int64)
    corr = (A.T @ A) > 0
    out = np.zeros(slots.shape, np.int32)
    for i in range(slots.shape[0]):
        eq = slots[i][:, None] == slots[i][None, :]
        np.fill_diagonal(eq, False)
        out[i] = (eq & (rooms[i][:, None] == rooms[i][None, :])).sum(1) + (eq & corr).sum(1)
    return out


@both
@pytest.mark.parametrize("event_hcv", [False, True], ids=["parts", "event_hcv"])
def test_eval_parts(ctx, name, event_hcv):
    """Without event_hcv the rows pass 2^32 bytes; with it P = ceil(2^30 / E) + M + 3,
    so that the int32 [P][E] output does while the inputs stay near 1 GiB."""
    c = ctx(name)
    P = lr.rows_past(1 << 30, c.E) if event_hcv else c.P
    with case("tt_eval_parts" + ("_event_hcv" if event_hcv else ""), name, P, (6 if event_hcv else 2) * P * c.E):
        bs, br = dev(c.slot), dev(c.room)
        bparts, beh = i32(M, 6), i32(M, c.E) if event_hcv else None
        raw_parts(c.dp, bs, br, bparts, beh)
        hp = host(bparts)
        same("base parts", dict(parts=ref_parts(c.inst, c.slot[MODEL_ROWS], c.room[MODEL_ROWS])), dict(parts=hp), MODEL_ROWS)
        assert np.array_equal(hp[:, :3].sum(1), c.scores[0]) and np.array_equal(hp[:, 3:].sum(1), c.scores[1])
        s, r = tile(bs, P), tile(br, P)
        parts, eh = i32(P, 6), i32(P, c.E) if event_hcv else None
        raw_parts(c.dp, s, r, parts, eh)
        periodic("tt_eval_parts", slot=(s, bs), room=(r, br), parts=(parts, bparts))
        if event_hcv:
            assert eh.numel() * 4 >= LINE + 4 * M * c.E
            same("base event_hcv", dict(eh=ref_event_hcv(c.inst, c.slot[MODEL_ROWS], c.room[MODEL_ROWS])),
                 dict(eh=beh), MODEL_ROWS)
            periodic("tt_eval_parts", event_hcv=(eh, beh))


# ---------------------------------------------------------------- the reference's per-row operations
@both
def test_assign_rooms(ctx, name):
    c = ctx(name)
    with case("tt_assign_rooms", name, c.P, 2 * c.P * c.E):
        bs, br = dev(c.slot), u8(M, c.E)
        c.dp.assign_rooms(bs, br)
        same("base", dict(room=c.o.assign_rooms(c.slot[ORACLE_ROWS])), dict(room=br), ORACLE_ROWS)
        s, r = tile(bs, c.P), u8(c.P, c.E)
        c.dp.assign_rooms(s, r)
        periodic("tt_assign_rooms", slot=(s, bs), room=(r, br))


@both
def test_random_init(ctx, name):
    c = ctx(name)
    with case("tt_random_init", name, c.P, 2 * c.P * c.E):
        want = c.o.random_init(c.seeds[ORACLE_ROWS])
        same("base", dict(slot=want[0], room=want[1], rng=want[2]), dict(slot=c.slot, room=c.room, rng=c.rng), ORACLE_ROWS)
        g, s, r = tile(c.seeds, c.P), u8(c.P, c.E), u8(c.P, c.E)
        c.dp.random_init(g, s, r)
        periodic("tt_random_init", slot=(s, c.slot), room=(r, c.room), rng=(g, c.rng))


def parents(c):
    """Parent 2 of row i is the base block's row i + 1: periodic like parent 1."""
    return c.slot, np.roll(c.slot, -1, axis=0)


@both
def test_crossover(ctx, name):
    """L2000 is past tt_crossover's documented limit (64 rows of each parent in
    the LDS: E <= 1280), so there the call, on the large buffers, must be
    TT_ERR_LIMIT and leave every buffer as it was."""
    c = ctx(name)
    A, B = parents(c)
    with case("tt_crossover", name, c.P, 4 * c.P * c.E):
        ba, bb, bg, bs, br = dev(A), dev(B), dev(c.seeds), u8(M, c.E), u8(M, c.E)
        if c.E > 1280:
            a, b, g, s, r = tile(ba, c.P), tile(bb, c.P), tile(c.seeds, c.P), u8(c.P, c.E), u8(c.P, c.E)
            with pytest.raises(native.TTError, match="too large") as e:
                c.dp.crossover(a, b, g, s, r)
            assert e.value.code == native.TT_ERR_LIMIT
            periodic("refused tt_crossover", slot1=(a, ba), slot2=(b, bb), rng=(g, c.seeds), slot=(s, bs), room=(r, br))
            return                                              # (bs, br: still the sentinel, like s and r)
        c.dp.crossover(ba, bb, bg, bs, br)
        want = c.o.crossover(A[ORACLE_ROWS], B[ORACLE_ROWS], c.seeds[ORACLE_ROWS])
        same("base", dict(slot=want[0], room=want[1], rng=want[2]), dict(slot=bs, room=br, rng=bg), ORACLE_ROWS)
        a, b, g, s, r = tile(ba, c.P), tile(bb, c.P), tile(c.seeds, c.P), u8(c.P, c.E), u8(c.P, c.E)
        c.dp.crossover(a, b, g, s, r)
        periodic("tt_crossover", slot1=(a, ba), slot2=(b, bb), slot=(s, bs), room=(r, br), rng=(g, bg))


@both
@pytest.mark.parametrize("repair", [False, True], ids=["plain", "repair"])
def test_crossover_guided(ctx, name, repair):
    c = ctx(name)
    A, B = parents(c)
    with case("tt_crossover_guided" + ("_repair" if repair else ""), name, c.P, 4 * c.P * c.E):
        order = c.dp.greedy_order()
        ba, bb, bg, bs, br, bc, bp = dev(A), dev(B), dev(c.seeds), u8(M, c.E), u8(M, c.E), i32(M), i32(M)
        c.dp.crossover_guided(ba, bb, bg, bs, br, order, repair, bc, bp)
        J = MODEL_ROWS
        ws, wg, wc, wp = cx.guided_slots(c.inst, host(order), A[J], B[J], c.seeds[J], repair)
        same("base", dict(slot=ws, room=c.o.assign_rooms(ws), rng=wg, cost=wc, repaired=wp),
             dict(slot=bs, room=br, rng=bg, cost=bc, repaired=bp), J)
        a, b, g, s, r = tile(ba, c.P), tile(bb, c.P), tile(c.seeds, c.P), u8(c.P, c.E), u8(c.P, c.E)
        cost, rep = i32(c.P), i32(c.P)
        c.dp.crossover_guided(a, b, g, s, r, order, repair, cost, rep)
        periodic("tt_crossover_guided", slot1=(a, ba), slot2=(b, bb), slot=(s, bs), room=(r, br), rng=(g, bg),
                 cost=(cost, bc), repaired=(rep, bp))
        assert c.dp.status() & 512 == 0


@both
def test_mutation(ctx, name):
    c = ctx(name)
    with case("tt_mutation", name, c.P, 2 * c.P * c.E):
        bs, br, bg = dev(c.slot), dev(c.room), dev(c.seeds)
        c.dp.mutation(bs, br, bg)
        want = c.o.mutation(c.slot[ORACLE_ROWS], c.room[ORACLE_ROWS], c.seeds[ORACLE_ROWS])
        same("base", dict(slot=want[0], room=want[1], rng=want[2]), dict(slot=bs, room=br, rng=bg), ORACLE_ROWS)
        assert (host(bs) != c.slot).any(axis=1).sum() > M // 2
        s, r, g = tile(c.slot, c.P), tile(c.room, c.P), tile(c.seeds, c.P)
        c.dp.mutation(s, r, g)
        periodic("tt_mutation", slot=(s, bs), room=(r, br), rng=(g, bg))


# ---------------------------------------------------------------- the searches (L448)
@pytest.mark.parametrize("ordered", [False, True], ids=["identity", "ordered"])
def test_local_search_eval(ctx, ordered):
    """Five steps with (1, 1, 0); once dispatched in an order that is not the identity."""
    c = ctx("L448")
    steps = 5
    with case("tt_local_search_eval" + ("_ordered" if ordered else ""), c.name, c.P, 2 * c.P * c.E):
        bs, br, bg, bout = dev(c.slot), dev(c.room), dev(c.seeds), eval_out(M)
        c.dp.local_search(bs, br, bg, steps, out=bout)
        J = ORACLE_ROWS
        ws, wr, wg = split_rows(c.o.local_search, (c.slot[J], c.room[J], c.seeds[J]), steps)
        same("base", dict(slot=ws, room=wr, rng=wg, **dict(zip(EVAL_NAMES, c.o.eval(ws, wr)))),
             dict(slot=bs, room=br, rng=bg, **dict(zip(EVAL_NAMES, bout))), J)
        assert (host(bs) != c.slot).any(axis=1).sum() > M // 2
        order = None
        if ordered:
            stride = 7919                                                   # a prime that does not divide P
            assert c.P % stride
            order = ((torch.arange(c.P, dtype=torch.int64, device="cuda") * stride) % c.P).to(torch.int32)
        s, r, g, out = tile(c.slot, c.P), tile(c.room, c.P), tile(c.seeds, c.P), eval_out(c.P)
        c.dp.local_search(s, r, g, steps, order=order, out=out)
        periodic("tt_local_search_eval", slot=(s, bs), room=(r, br), rng=(g, bg),
                 **{n: (x, b) for n, x, b in zip(EVAL_NAMES, out, bout)})
        assert c.dp.status() == 0


def test_greedy_init(ctx):
    c = ctx("L448")
    with case("tt_greedy_init", c.name, c.P, 2 * c.P * c.E):
        order = c.dp.greedy_order()
        bg, bs, br = dev(c.seeds), u8(M, c.E), u8(M, c.E)
        c.dp.greedy_init(bg, bs, br, order)
        J = MODEL_ROWS
        assert np.array_equal(host(order), gm.greedy_order(c.inst))
        ws, wg = gm.greedy_slots(c.inst, host(order), c.seeds[J])
        same("base", dict(slot=ws, room=c.o.assign_rooms(ws), rng=wg), dict(slot=bs, room=br, rng=bg), J)
        g, s, r = tile(c.seeds, c.P), u8(c.P, c.E), u8(c.P, c.E)
        c.dp.greedy_init(g, s, r, order)
        periodic("tt_greedy_init", slot=(s, bs), room=(r, br), rng=(g, bg))
        assert c.dp.status() & 32 == 0


def test_kempe_move(ctx):
    c = ctx("L448")
    with case("tt_kempe_move", c.name, c.P, 2 * c.P * c.E):
        bs, br, bg, bl = dev(c.slot), dev(c.room), dev(c.seeds), i32(M)
        c.dp.kempe_move(bs, br, bg, 1.0, 0, bl)
        J = MODEL_ROWS
        ws, wg, wl, pairs = km.kempe_rows(c.inst, c.slot[J], c.seeds[J], 1.0, 0, c.room[J])
        wr = km.expected_rooms(c.o, ws, c.room[J], wl, pairs)
        same("base", dict(slot=ws, room=wr, rng=wg, chain_len=wl), dict(slot=bs, room=br, rng=bg, chain_len=bl), J)
        assert (host(bl) > 0).all()                                         # prob 1: every row moved a chain
        s, r, g, ln = tile(c.slot, c.P), tile(c.room, c.P), tile(c.seeds, c.P), i32(c.P)
        c.dp.kempe_move(s, r, g, 1.0, 0, ln)
        periodic("tt_kempe_move", slot=(s, bs), room=(r, br), rng=(g, bg), chain_len=(ln, bl))
        assert c.dp.status() & 64 == 0


def test_slot_swap(ctx):
    c = ctx("L448")
    with case("tt_slot_swap", c.name, c.P, c.P * (c.E + 45)):
        bs, bscv, bpen = dev(c.slot), dev(c.scores[1]), dev(c.scores[3])
        bgain, bpass, bperm = i32(M), i32(M), u8(M, 45)
        c.dp.slot_swap(bs, 1, bscv, bpen, bgain, bpass, bperm)
        J = MODEL_ROWS
        ws, wgain, wpass, wperm = sm.descend_rows(c.inst, c.slot[J], 1)
        same("base", dict(slot=ws, gain=wgain, passes=wpass, perm=wperm),
             dict(slot=bs, gain=bgain, passes=bpass, perm=bperm), J)
        assert np.array_equal(host(bscv), c.scores[1] - host(bgain)) and (host(bpass) == 1).any()
        s, scv, pen = tile(c.slot, c.P), tile(c.scores[1], c.P), tile(c.scores[3], c.P)
        gain, passes, perm = i32(c.P), i32(c.P), u8(c.P, 45)
        c.dp.slot_swap(s, 1, scv, pen, gain, passes, perm)
        periodic("tt_slot_swap", slot=(s, bs), scv=(scv, bscv), penalty=(pen, bpen), gain=(gain, bgain),
                 passes=(passes, bpass), perm=(perm, bperm))
        assert c.dp.status() & 128 == 0


WALK_STEPS, WALK_HISTORY = 20, 5


def walk_case(c, what, call, rows, width):
    """tt_lahc / tt_lahc_kempe_aug on the walk block: `call(s, r, g, **outputs)`,
    rows(model rows) -> the model's arrays in the outputs' order."""
    w = walk_block(c)
    with case(what, c.name, c.P, 2 * c.P * c.E):
        def outputs(n, scv, pen):
            o = dict(scv=scv, penalty=pen, gain=i32(n), accepted=i32(n), best_step=i32(n))
            if width:
                o["kempe_stats"] = i32(n, width)
            return o
        bs, br, bg = dev(w.slot), dev(w.room), dev(w.rng)
        bo = outputs(M, dev(w.scores[1]), dev(w.scores[3]))
        call(bs, br, bg, **bo)
        J = MODEL_ROWS
        want = rows(w.slot[J], w.room[J], w.rng[J])
        names = ("slot", "room", "rng", "gain", "accepted", "best_step", "kempe_stats")[:len(want)]
        same("base", dict(zip(names, want)), dict(slot=bs, room=br, rng=bg, **bo), J)
        walked = int((host(bo["accepted"]) > 0).sum())
        assert 8 * walked >= M, f"only {walked} of {M} rows of the base block walk"
        assert np.array_equal(host(bo["scv"]), w.scores[1] - host(bo["gain"]))
        s, r, g = tile(w.slot, c.P), tile(w.room, c.P), tile(w.rng, c.P)
        o = outputs(c.P, tile(w.scores[1], c.P), tile(w.scores[3], c.P))
        call(s, r, g, **o)
        periodic(what, slot=(s, bs), room=(r, br), rng=(g, bg), **{k: (o[k], bo[k]) for k in o})
        assert c.dp.status() & 256 == 0
        print(f"{what}: {walked} of {M} base rows walk")


def test_lahc(ctx):
    c = ctx("L448")
    model = lm.Model(c.inst)
    walk_case(c, "tt_lahc", lambda s, r, g, **o: c.dp.lahc(s, r, g, WALK_STEPS, WALK_HISTORY, 0.5, **o),
              lambda s, r, g: model.lahc_rows(s, r, g, WALK_STEPS, WALK_HISTORY, 0.5), None)


def test_lahc_kempe_aug(ctx):
    c = ctx("L448")
    model = am.Model(c.inst)
    walk_case(c, "tt_lahc_kempe_aug",
              lambda s, r, g, **o: c.dp.lahc_kempe_aug(s, r, g, WALK_STEPS, WALK_HISTORY, 0.25, 0.5, 0, 1, **o),
              lambda s, r, g: model.lahc_kempe_aug_rows(s, r, g, WALK_STEPS, WALK_HISTORY, 0.25, 0.5, 0, 1), 7)


@pytest.mark.parametrize("name,K", [("L2000", 1024), ("L448", 128)])
def test_lahc_multi(ctx, name, K):
    """Many walkers a row: the *work* buffer passes 2^32 bytes while the
    population is small (a period of 47 rows). L2000's rows, 1,024 walkers each,
    are all closed (more events than cells): the walkers meet the gate only, so
    that case reaches the small front of the buffer alone (the state and the
    per-walker numbers, some 54 MB), not the stored rows behind it. L448's
    walk, 128 to a row (the model takes 10 ms a walker): its improved rows are
    stored in and read back from the part past 2^32 bytes, and that is asserted."""
    c = ctx(name)
    steps, m = 3, 47
    P = lr.rows_past(LINE, 2 * c.E * K, m)
    nbytes = c.dp.lahc_multi_work_bytes(P, K)
    assert lr.is_prime(m) and nbytes >= LINE + m * 2 * c.E * K and P * K < 2 ** 31
    src = walk_block(c) if name == "L448" else types.SimpleNamespace(slot=c.slot, room=c.room, rng=c.seeds, scores=c.scores)
    with case("tt_lahc_multi", name, P, nbytes + 8 * P * K):
        def outputs(n, scv, pen):
            return dict(scv=scv, penalty=pen, gain=i32(n), accepted=i32(n), best_step=i32(n), kempe_stats=i32(n, 7),
                        winner=i32(n), walker_gain=i32(n, K))
        run = lambda s, r, g, o, work: c.dp.lahc_multi(s, r, g, K, steps, WALK_HISTORY, 0.25, 0.5, 0, 1, work=work, **o)  # noqa: E731
        bs, br, bg = dev(src.slot[:m]), dev(src.room[:m]), dev(src.rng[:m])
        bo = outputs(m, dev(src.scores[1][:m]), dev(src.scores[3][:m]))
        run(bs, br, bg, bo, None)
        # the model on 16 rows; on 2 where every row is closed (it takes 1.7 s a row of 1,024 walkers at
        # 2,000 events), and there ttga_lahc_multi.h's word on a closed row, on all 47: it comes back as
        # it is, rng included, with zeros
        J = np.arange(16 if name == "L448" else 2)
        want = mm.Model(c.inst).lahc_multi_rows(src.slot[J], src.room[J], src.rng[J], K, steps, WALK_HISTORY, 0.25, 0.5, 0, 1)
        names = ("slot", "room", "rng", "gain", "accepted", "best_step", "kempe_stats", "winner", "walker_gain")
        same("base", dict(zip(names, want)), dict(slot=bs, room=br, rng=bg, **bo), J)
        walked = int((host(bo["accepted"]) > 0).sum())
        if name == "L2000":
            assert walked == 0 and (src.scores[0][:m] > 0).all()
            same("closed rows", dict(slot=src.slot[:m], room=src.room[:m], rng=src.rng[:m], scv=src.scores[1][:m],
                                     penalty=src.scores[3][:m]), dict(slot=bs, room=br, rng=bg, **bo))
            assert not any(host(bo[k]).any() for k in names[3:])
        else:
            # the large part of `work` is rows[P * K][2][E]: a walker stores its row there only when it
            # improved, and the commit reads the winner's only when its gain is positive. So the base
            # block must hold such rows (an eighth of it, as for the walks): each repeats once among
            # the last m + 3 rows, whose walkers' rows all lie past the 2^32-byte line
            improved = (host(bo["gain"]) > 0) & (host(bo["best_step"]) > 0)
            assert 8 * walked >= m and 8 * int(improved.sum()) >= m, (walked, int(improved.sum()))
            assert (host(bs)[improved] != src.slot[:m][improved]).any(axis=1).all()       # the stored row came back
            assert (P - m - 3) * K * 2 * c.E >= LINE
            print(f"tt_lahc_multi {name}: {int(improved.sum())} of {m} base rows come back through rows[]")
        s, r, g = tile(src.slot[:m], P), tile(src.room[:m], P), tile(src.rng[:m], P)
        o = outputs(P, tile(src.scores[1][:m], P), tile(src.scores[3][:m], P))
        work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        run(s, r, g, o, work)
        periodic("tt_lahc_multi", slot=(s, bs), room=(r, br), rng=(g, bg), **{k: (o[k], bo[k]) for k in o})


# ---------------------------------------------------------------- tt_ga_breed, tt_ga_breed_guided (L448)
def members(c, n=64):
    """n members of the walk block, sorted by penalty (ties by position)."""
    w = walk_block(c)
    pick = np.argsort(w.scores[3].astype(np.uint32)[:4 * n], kind="stable")[::4][:n]
    return w.slot[pick], w.room[pick], w.scores[3][pick]


@pytest.mark.parametrize("guided", [False, True], ids=["tt_ga_breed", "tt_ga_breed_guided"])
def test_ga_breed(ctx, guided):
    """N = 64 members, C * E past 2^32, the children periodic in their seeds."""
    c = ctx("L448")
    ps, pr, pp = members(c)
    assert (np.diff(pp.astype(np.uint32).astype(np.int64)) >= 0).all()
    C = c.P
    with case("tt_ga_breed_guided" if guided else "tt_ga_breed", c.name, C, 2 * C * c.E):
        dps, dpr, dpp = dev(ps), dev(pr), dev(pp)
        order = c.dp.greedy_order() if guided else None

        def breed(g, s, r, fl, cost, rep):
            if guided:
                c.dp.ga_breed_guided(dps, dpr, dpp, g, s, r, fl, 0.8, 0.5, True, order, True, cost, rep)
            else:
                c.dp.ga_breed(dps, dpr, dpp, g, s, r, fl, 0.8, 0.5, True)
        bg, bs, br, bf, bc, bp = dev(c.seeds), u8(M, c.E), u8(M, c.E), u8(M), i32(M), i32(M)
        breed(bg, bs, br, bf, bc, bp)
        if guided:
            J = MODEL_ROWS
            ws, wr, wf, wg, wc, wp = cx.breed(c.inst, c.o, host(order), ps, pr, pp, c.seeds[J], 0.8, 0.5, 1, True)
            same("base", dict(slot=ws, room=wr, flags=wf, rng=wg, cost=wc, repaired=wp),
                 dict(slot=bs, room=br, flags=bf, rng=bg, cost=bc, repaired=bp), J)
        else:
            J = ORACLE_ROWS
            ws, wr, wf, wg = c.o.ga_breed(ps, pr, pp, c.seeds[J], len(J), 0.8, 0.5, 1)
            same("base", dict(slot=ws, room=wr, flags=wf, rng=wg), dict(slot=bs, room=br, flags=bf, rng=bg), J)
        assert set(np.unique(host(bf)).tolist()) == {0, 1, 2, 3}
        g, s, r, fl, cost, rep = tile(c.seeds, C), u8(C, c.E), u8(C, c.E), u8(C), i32(C), i32(C)
        breed(g, s, r, fl, cost, rep)
        periodic("breed", slot=(s, bs), room=(r, br), flags=(fl, bf), rng=(g, bg))
        if guided:
            periodic("breed", cost=(cost, bc), repaired=(rep, bp))
        for t, w in ((dps, ps), (dpr, pr), (dpp, pp)):
            assert np.array_equal(host(t), w)


# ---------------------------------------------------------------- the entry points that look across rows
@both
def test_slot_histogram(ctx, name):
    c = ctx(name)
    with case("tt_slot_histogram", name, c.P, c.P * c.E):
        k, rem = divmod(c.P, M)
        whole, part = host(c.dp.slot_histogram(dev(c.slot))), host(c.dp.slot_histogram(dev(c.slot[:rem])))
        ref = np.stack([np.bincount(c.slot[:, e], minlength=45)[:45] for e in range(c.E)])
        assert np.array_equal(whole, ref) and whole.sum() == M * c.E and part.sum() == rem * c.E
        s = tile(c.slot, c.P)
        hist = c.dp.slot_histogram(s)
        assert np.array_equal(host(hist).astype(np.int64), k * whole.astype(np.int64) + part)
        periodic("tt_slot_histogram", slot=(s, c.slot))


def test_genome_first(ctx):
    """first[i] is the base block's first[i mod M]; its rows are distinct, so that is i mod M."""
    c = ctx("L448")
    with case("tt_genome_first", c.name, c.P, 2 * c.P * c.E):
        bfirst = c.dp.genome_first(dev(c.slot), dev(c.room))
        assert np.array_equal(host(bfirst), np.arange(M))
        s, r, first = tile(c.slot, c.P), tile(c.room, c.P), i32(c.P)
        work = torch.empty(int(c.dp.lib.tt_genome_work_bytes(c.P, c.E)), dtype=torch.uint8, device="cuda")
        native._check(c.dp.lib, c.dp.lib.tt_genome_first(c.dp.handle, s.data_ptr(), r.data_ptr(), c.P, first.data_ptr(),
                                                         0, ctypes.c_void_p(work.data_ptr()), c.dp._stream(s)))
        periodic("tt_genome_first", first=(first, bfirst), slot=(s, c.slot), room=(r, c.room))


def test_ga_replace(ctx):
    """N * E past 2^32, 3,000 children, a work buffer of exactly tt_ga_work_bytes.
    First the sort of the unsorted periodic population (C = 0), then the
    replacement. After each: penalties ascending (as unsigned) and a fresh
    tt_eval of the new population reproduces hcv, scv, feasible and penalty row
    for row, so every row travelled with its own scores. After the replacement
    the penalties are the multiset ttga.h states: those of the sorted
    population's positions 0 .. N-C-1 and the children's (the children
    overwrite the last C positions, better or not), by a device sort."""
    c = ctx("L448")
    w = walk_block(c)
    N, C = c.P, 3000
    nwork = int(c.dp.lib.tt_ga_work_bytes(N, c.E))
    with case("tt_ga_replace", c.name, N, 2 * N * c.E + nwork):
        pop = dict(slot=tile(c.slot, N), room=tile(c.room, N))
        pop.update({k: tile(v, N) for k, v in zip(EVAL_NAMES, c.scores)})
        # children: 1,500 searched rows (better than every member) and 1,500 of the block's own (ties)
        rows = dict(slot=np.concatenate([w.slot[:1500], c.slot[1500:3000]]),
                    room=np.concatenate([w.room[:1500], c.room[1500:3000]]))
        rows.update({k: np.concatenate([a[:1500], b[1500:3000]]) for k, a, b in zip(EVAL_NAMES, w.scores, c.scores)})
        child = {k: dev(v) for k, v in rows.items()}
        work = torch.empty(nwork, dtype=torch.uint8, device="cuda")

        def check(what, want_pen):
            pen = pop["penalty"]
            assert bool((pen[1:] >= pen[:-1]).all()), f"{what}: penalties not ascending"      # all >= 0 here
            assert torch.equal(pen, want_pen), f"{what}: not the wanted multiset of penalties"
            fresh = c.dp.eval(pop["slot"], pop["room"], out=eval_out(N))
            for k, t in zip(EVAL_NAMES, fresh):
                bad = torch.nonzero(t != pop[k]).flatten()[:8].tolist()
                assert not bad, f"{what}: {k} of rows {bad} is not the row's own"
        assert (c.scores[3] >= 0).all() and (w.scores[3] >= 0).all()
        before = torch.sort(pop["penalty"]).values
        c.dp.ga_replace(pop, None, work)
        check("sort", before)
        union = torch.sort(torch.cat([pop["penalty"][:N - C], child["penalty"]])).values
        c.dp.ga_replace(pop, child, work)
        check("replace", union)
        assert int(pop["feasible"][:1500].sum()) > 0 and np.array_equal(host(child["slot"]), rows["slot"])
        src = c.dp.ga_work_source(work, N)
        assert N - C <= src < N - C + 1500                                  # the new best is a searched child


# ---------------------------------------------------------------- the launch limit
def test_launch_limit(ctx):
    """HIP runs no launch of more than 2^32 - 1 threads in full (it reports
    success and runs the count modulo 2^32, or refuses an exact multiple).
    eval_block and the parts kernels give a row 256 threads, assign_rooms_kernel
    too in the wide layout (R > 16): 2^24 + 3 rows and 2^24 rows (the first
    past the bound) are TT_ERR_LIMIT with every output left as it was, 2^24 - 1
    rows (the bound) match the oracle."""
    inst = ttga.generate(3, 17, 2, 5, seed=3)
    dp, o = native.DeviceProblem(inst), oracle().problem(inst)
    bound = (2 ** 32 - 1) // 256
    assert bound == 2 ** 24 - 1
    over = 2 ** 24 + 3
    with case("launch_limit", "E3_R17", over, 40 * over):
        seeds = mm_seeds(M, 31)
        bs, br, bg = u8(M, 3), u8(M, 3), dev(seeds)
        dp.random_init(bg, bs, br)
        s, r = tile(bs, over), tile(br, over)
        out, parts, room = eval_out(over), i32(over, 6), u8(over, 3)
        for n in (over, bound + 1):
            sn, rn = s[:n], r[:n]
            for what, call in (("tt_eval_variant 2", lambda: dp.eval(sn, rn, variant=2, out=tuple(t[:n] for t in out))),
                               ("tt_eval_parts", lambda: raw_parts(dp, sn, rn, parts[:n], None)),
                               ("tt_assign_rooms", lambda: dp.assign_rooms(sn, room[:n]))):
                with pytest.raises(native.TTError, match="too large for one launch") as e:
                    call()
                assert e.value.code == native.TT_ERR_LIMIT, (what, n)
        torch.cuda.synchronize()
        assert all(bool((t == I32_FILL).all()) for t in (out[0], out[1], out[3], parts))
        assert bool((out[2] == U8_FILL).all()) and bool((room == U8_FILL).all())
        periodic("refused calls", slot=(s, bs), room=(r, br))
        # one row under: the bound itself
        s, r = s[:bound], r[:bound]
        hs, hr = host(s), host(r)
        want = split_rows(o.eval, (hs, hr))
        got = dp.eval(s, r, variant=2, out=tuple(t[:bound] for t in out))
        same("tt_eval_variant 2 at the bound", dict(zip(EVAL_NAMES, want)), dict(zip(EVAL_NAMES, got)))
        raw_parts(dp, s, r, parts[:bound], None)
        hp = host(parts[:bound])
        assert np.array_equal(hp[:, :3].sum(1), want[0]) and np.array_equal(hp[:, 3:].sum(1), want[1])
        bparts = i32(M, 6)
        raw_parts(dp, bs, br, bparts, None)
        same("base parts", dict(parts=ref_parts(inst, host(bs), host(br))), dict(parts=bparts))
        periodic("tt_eval_parts at the bound", parts=(parts[:bound], bparts))
        dp.assign_rooms(s, room[:bound])
        same("tt_assign_rooms at the bound", dict(room=split_rows(lambda x: (o.assign_rooms(x),), (hs,))[0]),
             dict(room=room[:bound]))
        assert bool((parts[bound:] == I32_FILL).all()) and bool((room[bound:] == U8_FILL).all())
    dp.close()


def test_launch_limit_one_wave(ctx):
    """The kernels with one wave a row take 67,108,863 rows. With 16 rooms the
    matcher is one of them: tt_assign_rooms runs 2^24 + 3 rows, which 17 rooms
    refuse (test_launch_limit). tt_mutation at 2^26 rows is TT_ERR_LIMIT with
    slot, room and rng as they were; at 2^26 - 1 rows, the bound, it mutates
    every row as it does the base block's, which the oracle judges."""
    inst = ttga.generate(3, 16, 2, 5, seed=3)
    dp, o = native.DeviceProblem(inst), oracle().problem(inst)
    bound = (2 ** 32 - 1) // 64
    assert bound == 2 ** 26 - 1
    with case("launch_limit_one_wave", "E3_R16", bound + 1, 20 * (bound + 1)):
        seeds = mm_seeds(M, 41)
        bs, br, bg = u8(M, 3), u8(M, 3), dev(seeds)
        dp.random_init(bg, bs, br)
        hs, hr, hg = host(bs), host(br), host(bg)
        n = 2 ** 24 + 3
        s, room, broom = tile(bs, n), u8(n, 3), u8(M, 3)
        dp.assign_rooms(bs, broom)
        same("base rooms", dict(room=o.assign_rooms(hs)), dict(room=broom))
        dp.assign_rooms(s, room)
        periodic("tt_assign_rooms, 16 rooms", slot=(s, bs), room=(room, broom))
        del s, room
        s, r, g = tile(bs, bound + 1), tile(br, bound + 1), tile(bg, bound + 1)
        with pytest.raises(native.TTError, match="too large for one launch .*at most 67108863") as e:
            dp.mutation(s, r, g)
        assert e.value.code == native.TT_ERR_LIMIT
        periodic("refused tt_mutation", slot=(s, bs), room=(r, br), rng=(g, bg))
        dp.mutation(bs, br, bg)
        want = o.mutation(hs, hr, hg)
        same("base mutation", dict(slot=want[0], room=want[1], rng=want[2]), dict(slot=bs, room=br, rng=bg))
        dp.mutation(s[:bound], r[:bound], g[:bound])
        periodic("tt_mutation at the bound", slot=(s[:bound], bs), room=(r[:bound], br), rng=(g[:bound], bg))
        periodic("the row past the bound", slot=(s[bound:], dev(hs[bound % M:bound % M + 1])),
                 rng=(g[bound:], dev(hg[bound % M:bound % M + 1])))
    dp.close()


def test_genome_first_bound(ctx):
    """tt_genome_first's grid has 16 threads a row: 268,435,440 rows at most.
    At that bound (E = 3; past 2^27 rows the padding loop's thread index needs
    more than 31 bits) first[i] is the base block's first[i mod M], duplicates
    of the block included; one row more is TT_ERR_LIMIT and writes nothing."""
    inst = ttga.generate(3, 16, 2, 5, seed=3)
    dp = native.DeviceProblem(inst)
    bound = 16 * ((2 ** 32 - 1) // 256)
    assert bound == 268_435_440
    nwork = int(dp.lib.tt_genome_work_bytes(bound + 1, 3))
    with case("tt_genome_first_bound", "E3_R16", bound, 10 * (bound + 1) + nwork):
        bs, br, bg = u8(M, 3), u8(M, 3), dev(mm_seeds(M, 43))
        dp.random_init(bg, bs, br)
        bfirst = dp.genome_first(bs, br)
        seen, want = {}, np.zeros(M, np.int32)
        for i, key in enumerate(a.tobytes() + b.tobytes() for a, b in zip(host(bs), host(br))):
            want[i] = seen.setdefault(key, i)
        assert np.array_equal(host(bfirst), want) and (want != np.arange(M)).any()
        s, r, first = tile(bs, bound + 1), tile(br, bound + 1), i32(bound + 1)
        work = torch.empty(nwork, dtype=torch.uint8, device="cuda")

        def call(n):
            native._check(dp.lib, dp.lib.tt_genome_first(dp.handle, s.data_ptr(), r.data_ptr(), n, first.data_ptr(), 0,
                                                         ctypes.c_void_p(work.data_ptr()), dp._stream(s)))
        with pytest.raises(native.TTError, match="too large for one launch") as e:
            call(bound + 1)
        assert e.value.code == native.TT_ERR_LIMIT
        periodic("refused tt_genome_first", first=(first, i32(M)))
        call(bound)
        periodic("tt_genome_first at the bound", first=(first[:bound], bfirst), slot=(s, bs), room=(r, br))
        assert int(first[bound]) == I32_FILL
    dp.close()
