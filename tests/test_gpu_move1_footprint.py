"""What tt_move1_scan and tt_move1_descent may write, and where their buffers
may lie: tests/test_gpu_footprint.py's frame (every argument carved from one
guarded arena, tests/arena.py; payloads of exactly the documented size between
guards; int32 payloads 4-byte aligned and no better, uint8 payloads at a byte
skew, to_room's included) on that module's "W" instance, with the outputs
equal to tests/move1_model.py. The header sits in include/ttga/, which the
older module's completeness test does not scan, so this module has its own."""
import pathlib
import re
import types

import numpy as np
import pytest

import ttga
import move1_model as mm

pytestmark = pytest.mark.gpu

import torch  # noqa: E402,F401
from ttga import native  # noqa: E402
from test_gpu_footprint import IN, IO, LIMIT, OUT, P2, TWO_SKEWS, Case, built, ctx_of, evaluated, expand, memo, run  # noqa: E402

DESCENT_PASSES = 6


def move1_rows(cx):
    def make():
        model = mm.Model(cx.inst)
        slot, room = mm.population(cx.inst, P2, model)
        ev = evaluated(cx, slot, room)
        assert 2 * int((ev["hcv"] == 0).sum()) >= P2 and (ev["hcv"] != 0).any()      # scanned and unscanned rows
        return model, slot, room, ev
    return memo(cx, "move1_rows", make)


def scan_case(cx, outputs=("summary", "d_scv", "to_room")):
    model, slot, room, _ = move1_rows(cx)
    E = cx.inst.E
    want = dict(zip(("summary", "d_scv", "to_room"), memo(cx, "move1_scan", lambda: model.scan_rows(slot, room))))
    assert want["summary"][:, 2].any() and (want["to_room"] == mm.UNSCANNED).any()
    shapes = {"summary": ("int32", (P2, 6)), "d_scv": ("int32", (P2, E, 45)), "to_room": ("uint8", (P2, E, 45))}
    args = [IN("slot", slot), IN("room", room)] + [OUT(n, *shapes[n]) for n in outputs]
    return Case(args, lambda lib, h, p, st: lib.tt_move1_scan(h, p["slot"], p["room"], P2, p["summary"], p["d_scv"],
                                                              p["to_room"], st),
                {n: want[n] for n in outputs})


def descent_case(cx):
    model, slot, room, ev = move1_rows(cx)
    s, r, gain, passes = memo(cx, "move1_descent", lambda: model.descent_rows(slot, room, DESCENT_PASSES))
    after = evaluated(cx, s, r)
    assert passes.max() == DESCENT_PASSES and np.array_equal(after["scv"], ev["scv"] - gain)
    return Case([IO("slot", slot), IO("room", room), IO("scv", ev["scv"]), IO("penalty", ev["penalty"]),
                 OUT("gain", "int32", P2), OUT("passes", "int32", P2)],
                lambda lib, h, p, st: lib.tt_move1_descent(h, p["slot"], p["room"], P2, DESCENT_PASSES, p["scv"],
                                                           p["penalty"], p["gain"], p["passes"], st),
                {"slot": s, "room": r, "scv": after["scv"], "penalty": after["penalty"], "gain": gain, "passes": passes})


# call id -> (instances, builder); every one runs at TWO_SKEWS
CALLS = {
    "tt_move1_scan": ("W", scan_case),
    "tt_move1_scan-summary": ("W", lambda cx: scan_case(cx, ("summary",))),
    "tt_move1_scan-tables": ("W", lambda cx: scan_case(cx, ("d_scv", "to_room"))),
    "tt_move1_descent": ("W", descent_case),
}


@pytest.mark.parametrize("inst,cid,skews", expand(CALLS, TWO_SKEWS))
def test_footprint(inst, cid, skews):
    cx, case = built(CALLS, inst, cid)
    run(cx, case, skews)


def test_payloads_are_the_documented_sizes():
    """4 P 6, 4 P E 45, P E 45, P E and 4 P bytes: run() carves exactly the shapes given here."""
    cx = ctx_of("W")
    E = cx.inst.E
    sizes = {}
    for cid in ("tt_move1_scan", "tt_move1_descent"):
        for n, role, kind, shape, init, g in built(CALLS, "W", cid)[1].args:
            sizes[cid, n] = int(np.prod(shape)) * (1 if kind == "uint8" else 4)
    assert sizes["tt_move1_scan", "summary"] == 4 * P2 * 6 and sizes["tt_move1_scan", "d_scv"] == 4 * P2 * E * 45
    assert sizes["tt_move1_scan", "to_room"] == P2 * E * 45
    assert sizes["tt_move1_scan", "slot"] == sizes["tt_move1_descent", "room"] == P2 * E
    assert all(sizes["tt_move1_descent", n] == 4 * P2 for n in ("scv", "penalty", "gain", "passes"))


@pytest.mark.parametrize("skews", TWO_SKEWS, ids=lambda s: f"s{s[0]}r{s[1]}")
@pytest.mark.parametrize("call", ["scan", "descent"])
def test_limit_leaves_the_arena_untouched(call, skews):
    """8,200 students: the masks alone pass 64 KB, TT_ERR_LIMIT, and no byte of the arena changes."""
    cx = memo(ctx_of("W"), "move1_limit_ctx", lambda: types.SimpleNamespace(
        inst=ttga.generate(40, 3, 2, 8200), memo={}, dp=native.DeviceProblem(ttga.generate(40, 3, 2, 8200))))
    g = np.random.default_rng(11)
    P, E = 5, 40
    slot, room = g.integers(0, 45, (P, E)).astype(np.uint8), g.integers(0, 3, (P, E)).astype(np.uint8)
    if call == "scan":
        case = Case([IN("slot", slot), IN("room", room), OUT("summary", "int32", (P, 6)), OUT("d_scv", "int32", (P, E, 45)),
                     OUT("to_room", "uint8", (P, E, 45))],
                    lambda lib, h, p, st: lib.tt_move1_scan(h, p["slot"], p["room"], P, p["summary"], p["d_scv"],
                                                            p["to_room"], st), {}, rc=LIMIT)
    else:
        four = np.arange(P, dtype=np.int32)
        case = Case([IO("slot", slot), IO("room", room), IO("scv", four), IO("penalty", four), OUT("gain", "int32", P),
                     OUT("passes", "int32", P)],
                    lambda lib, h, p, st: lib.tt_move1_descent(h, p["slot"], p["room"], P, 3, p["scv"], p["penalty"],
                                                               p["gain"], p["passes"], st), {}, rc=LIMIT)
    run(cx, case, skews)


def test_every_entry_point_of_include_ttga_is_in_the_table():
    """Every function of include/ttga/*.h with a device buffer among its arguments."""
    inc = pathlib.Path(__file__).resolve().parent.parent / "include" / "ttga"
    names = set()
    for hdr in inc.glob("*.h"):
        names |= set(re.findall(r"^int (tt_\w+)\(", hdr.read_text(), flags=re.M))
    assert names and names == {cid.split("-")[0] for cid in CALLS}, names
