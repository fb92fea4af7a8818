"""What the GPU tests of the four late-acceptance entry points share
(tests/test_gpu_lahc.py, _kempe, _kempe_aug, _multi): one call on numpy rows
with tt_eval around it, the post-conditions every such call must meet, the
stream's advance, and the three frames for invalid genes, refused arguments
and the LDS limit. torch and the library are imported where they are used, so
check_rows runs on canned arrays without a device."""
import numpy as np
import pytest

import lahc_model as lm
from helpers import dev, host

BAD_GENE = 256                                   # tt_device_status bit 8
FILL = 12345
NAMES = ("slot", "room", "rng", "gain", "accepted", "best_step", "kempe_stats", "winner", "walker_gain")
LDS_BYTES = 65536


def filled(*shape):
    import torch
    return torch.full(shape, FILL, dtype=torch.int32, device="cuda")


def run(dp, call, slot, room, seeds, width=None, with_eval=True, **extra):
    """One call on numpy rows: call(s, r, g, scv=, penalty=, gain=, accepted=,
    best_step=[, kempe_stats=][, extra...]) on sentinel-filled outputs. width:
    the columns of kempe_stats (None: the call has none); extra: further
    per-row outputs by keyword, each the shape behind P. Returns the outputs
    (NAMES' order), tt_eval before and after, and scv / penalty in place."""
    P = slot.shape[0]
    s, r, g = dev(slot), dev(room), dev(seeds)
    before = [host(t) for t in dp.eval(s, r)] if with_eval else None
    scv = dev(before[1]) if with_eval else None
    pen = dev(before[3]) if with_eval else None
    out = dict(gain=filled(P), accepted=filled(P), best_step=filled(P))
    if width is not None:
        out["kempe_stats"] = filled(P, width)
    for name, shape in extra.items():
        out[name] = filled(P, *shape)
    call(s, r, g, scv=scv, penalty=pen, **out)
    got = (host(s), host(r), host(g), *(host(t) for t in out.values()))
    after = [host(t) for t in dp.eval(s, r)] if with_eval else None
    return got, before, after, (host(scv), host(pen)) if with_eval else None


def same(got, want, names=NAMES):
    P = got[0].shape[0]
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape, name
        diff = np.flatnonzero((g.reshape(P, -1) != w.reshape(P, -1)).any(axis=1))
        assert diff.size == 0, f"{name} differs in rows {diff[:8]}: gpu {g[diff[:2]]} want {w[diff[:2]]}"


def check_rows(got, want, before, after, inplace, slot, room, seeds, steps):
    """What every call of the family must meet: the wanted rows bit for bit
    (want None: not compared), and around it tt_eval: hcv and feasible
    unchanged, scv lower by exactly the gain, scv / penalty in place equal to a
    fresh evaluation; the rows the gate keeps out byte-identical, their rng
    untouched and every output 0; the bounds on accepted, best_step and the
    Kempe counts. Returns the closed rows' mask."""
    if want is not None:
        same(got, want)
    hcv0, scv0, feas0, pen0 = before
    hcv1, scv1, feas1, pen1 = after
    assert np.array_equal(hcv1, hcv0) and np.array_equal(feas1, feas0)
    assert np.array_equal(scv1, scv0 - got[3]) and (got[3] >= 0).all()
    assert np.array_equal(inplace[0], scv1) and np.array_equal(inplace[1], pen1)      # in place = a fresh tt_eval
    closed = hcv0 != 0                                                               # rows the gate keeps out
    assert np.array_equal(got[0][closed], slot[closed]) and np.array_equal(got[1][closed], room[closed])
    assert np.array_equal(got[2][closed], seeds[closed])
    for k in range(3, len(got)):
        assert not got[k][closed].any(), NAMES[k]
    assert (got[5] <= steps).all() and (got[4] <= steps).all()
    if len(got) > 6:
        st = got[6].astype(np.int64)                    # tried, capped, no room, accepted, events[, rescued, displaced]
        assert (st[:, 3] <= st[:, 0] - st[:, 1] - st[:, 2]).all() and (st[:, 3] <= got[4]).all()
        if st.shape[1] > 5:
            assert (st[:, 5] <= st[:, 0] - st[:, 1] - st[:, 2]).all()
    return closed


def check_stream_advance(got, seeds, closed, draws):
    """The first searched row's stream advanced by exactly `draws` draws. Returns the row."""
    from ttga.rng import step
    i = int(np.flatnonzero(~closed)[0])
    s = int(seeds[i])
    for _ in range(draws):
        s = step(s)
    assert got[2][i] == s
    return i


# ---------------------------------------------------------------- the three frames
# call(dp, a) -> the function run() calls, for the arguments in the dict a;
# rows(model, slot, room, seeds, a) -> the model's rows for the same arguments.
def invalid_genes(Model, call, rows, a, width=None, closed=(1, 4), **extra):
    """Rows with slot gene 45 / room gene R between valid ones: untouched, rng
    included, outputs 0, status bit 8; their neighbours walk as the model has
    them. Own handle: the status word is sticky."""
    from ttga import native
    inst = lm.SHAPES["sm"]()
    dp, model = native.DeviceProblem(inst), Model(inst)
    slot, room, seeds = lm.population(inst, 6, model)
    slot[1, 7] = 45
    room[4, 3] = inst.R
    assert dp.status() == 0
    want = rows(model, slot, room, seeds, a)
    got, _, _, _ = run(dp, call(dp, a), slot, room, seeds, width, with_eval=False, **extra)
    same(got, want)
    for i in closed:
        assert np.array_equal(got[0][i], slot[i]) and np.array_equal(got[1][i], room[i]) and got[2][i] == seeds[i]
        assert not any(np.asarray(got[k][i]).any() for k in range(3, len(got)))
    assert got[4][0] > 0 and got[4][3] > 0 and got[4][5] > 0
    assert dp.status() & BAD_GENE == BAD_GENE
    dp.close()


def _refused(problem, width):
    inst, dp, model = problem
    slot, room, seeds = lm.population(inst, 4, model)
    bufs = (dev(slot), dev(room), dev(seeds))
    out = dict(scv=filled(4), penalty=filled(4), gain=filled(4), accepted=filled(4), best_step=filled(4))
    if width is not None:
        out["kempe_stats"] = filled(4, width)

    def untouched():
        assert all(np.array_equal(host(t), w) for t, w in zip(bufs, (slot, room, seeds)))
        assert all((host(t) == FILL).all() for t in out.values())
    return dp, model, (slot, room, seeds), bufs, out, untouched


def invalid_arguments_launch_nothing(problem, call, rows, ok, bad, null_call, width=None):
    """Every dict of `bad` over `ok` is TT_ERR_INVALID and leaves every buffer as
    it was; then null_call(dp, s, r, g), 200 steps on a history of 20 with every
    output NULL, walks as the model has it."""
    from ttga import native
    dp, model, host_rows, bufs, out, untouched = _refused(problem, width)
    for kw in bad:
        with pytest.raises(native.TTError) as ei:
            call(dp, {**ok, **kw})(*bufs, **out)
        assert ei.value.code == native.TT_ERR_INVALID, kw
    untouched()
    null_call(dp, *bufs)
    want = rows(model, *host_rows, {**ok, "steps": 200, "history": 20})
    assert all(np.array_equal(host(t), w) for t, w in zip(bufs, want))


def lds_limit(problem, call, rows, ok, fixed, width=None):
    """A history too long for the LDS (`fixed` bytes go to the rest of the
    image): TT_ERR_LIMIT, every buffer untouched; the largest history that fits
    walks as the model has it. Returns that call's slot, room and the model's rows."""
    from ttga import native
    dp, model, host_rows, bufs, out, untouched = _refused(problem, width)
    fits = (LDS_BYTES - fixed) // 4
    with pytest.raises(native.TTError, match="too large") as ei:
        call(dp, {**ok, "history": fits + 1})(*bufs, **out)
    assert ei.value.code == native.TT_ERR_LIMIT
    untouched()
    some = {k: out[k] for k in ("gain", "kempe_stats") if k in out}
    call(dp, {**ok, "history": fits})(*bufs, **some)
    want = rows(model, *host_rows, {**ok, "history": fits})
    assert np.array_equal(host(out["gain"]), want[3])
    assert width is None or np.array_equal(host(out["kempe_stats"]), want[6])
    return host(bufs[0]), host(bufs[1]), want
