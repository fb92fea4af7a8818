"""tests/arena.py on CPU tensors with a fake "call": the region geometry
(sizes, alignment, skew), a clean call passes, and each planted defect -- a
byte just past or just before a payload, a write 63 rows away, a changed input,
a byte past a work buffer of exactly work_bytes -- makes check() fail with a
message that names the region and the side."""
import numpy as np
import pytest

import arena as ar

P, E = 67, 81
WORK_BYTES = 5 * 256 + 24


def carve(slot_skew=0, room_skew=0):
    rng = np.random.default_rng(1)
    a = ar.Arena("cpu")
    a.add("slot", "in", "uint8", (P, E), rng.integers(0, 45, (P, E), dtype=np.uint8), skew=slot_skew)
    a.add("room", "inout", "uint8", (P, E), rng.integers(0, 9, (P, E), dtype=np.uint8), skew=room_skew)
    a.add("rng", "inout", "int64", (P,), rng.integers(1, 2 ** 31 - 1, P, dtype=np.int64))
    a.add("order", "in", "int32", (P,), rng.permutation(P).astype(np.int32))
    a.add("hcv", "out", "int32", (P,))
    a.add("stats", "out", "int32", (P, 7))
    a.add("work", "work", "work", (WORK_BYTES,))
    views = a.build()
    a.snapshot()
    return a, views


def clean_call(v):
    """Writes every writable payload in full, reads the inputs."""
    v["room"][:] = (v["slot"] % 7)
    v["rng"] += 1
    v["hcv"][:] = v["order"] * 2
    v["stats"][:] = 5
    v["work"][:] = 0xAB


@pytest.mark.parametrize("skews", [(0, 0), (1, 0), (0, 1), (2, 2), (4, 8), (3, 5), (1, 3), (15, 255)])
def test_geometry(skews):
    a, v = carve(*skews)
    sizes = {"slot": P * E, "room": P * E, "rng": 8 * P, "order": 4 * P, "hcv": 4 * P, "stats": 4 * P * 7,
             "work": WORK_BYTES}
    base = a.buf.data_ptr()
    prev_hi = 0
    for r in a.regions:
        assert r.end - r.start == sizes[r.name] == r.view.numel() * r.view.element_size()
        assert r.view.is_contiguous() and r.view.data_ptr() == base + r.start
        assert tuple(r.view.shape) == r.shape
        # guards: >= 4,096 bytes and >= 64 rows on both sides, inside the one allocation, regions disjoint
        g = max(4096, 64 * r.row_bytes)
        assert r.start - r.lo >= g and r.hi - r.end >= g
        assert r.lo == prev_hi and r.hi <= a.buf.numel()
        prev_hi = r.hi
    assert a["stats"].row_bytes == 28 and a["slot"].row_bytes == E and a["slot"].guard == 64 * E
    addr = {r.name: r.view.data_ptr() for r in a.regions}
    assert addr["slot"] % 256 == skews[0] and addr["room"] % 256 == skews[1]
    for name in ("order", "hcv", "stats"):
        assert addr[name] % 8 == 4                       # int32: 4-byte aligned and no better
    assert addr["rng"] % 16 == 8 and addr["work"] % 16 == 8
    assert v["rng"].dtype == ar.torch.int64 and v["hcv"].dtype == ar.torch.int32 and v["work"].dtype == ar.torch.uint8
    # inputs hold their initial value, outputs the random prefill (position-dependent, not a constant)
    assert np.array_equal(v["slot"].numpy(), a["slot"].init) and np.array_equal(v["rng"].numpy(), a["rng"].init)
    for name in ("hcv", "work"):
        raw = a.buf[a[name].start:a[name].end].numpy()
        assert len(np.unique(raw)) > 16
    guard = a.buf[a["slot"].lo:a["slot"].start].numpy()
    assert len(np.unique(guard)) > 200


def test_fill_is_reproducible():
    """Two arenas of one description are byte for byte the same, layout included,
    wherever the allocator puts them (held together, so their addresses differ)."""
    keep = [carve(3, 5) for _ in range(4)]
    a = keep[0][0]
    assert len({x.buf.data_ptr() for x, _ in keep}) == 4 and a.buf.data_ptr() % 256 == 0
    for b, _ in keep[1:]:
        assert [(r.lo, r.start, r.end, r.hi) for r in b.regions] == [(r.lo, r.start, r.end, r.hi) for r in a.regions]
        assert np.array_equal(a.buf.numpy(), b.buf.numpy())


def test_clean_call_passes():
    a, v = carve(1, 3)
    clean_call(v)
    a.check()
    with pytest.raises(AssertionError):
        a.check(untouched=True)                          # a refused call must not have written even its outputs


def test_untouched_arena_passes_both_checks():
    a, _ = carve(3, 5)
    a.check()
    a.check(untouched=True)


def flip(a, pos):
    a.buf[pos] = a.buf[pos] ^ 0x5A


DEFECTS = {
    # name: (region, position of the planted byte, words the message must hold)
    "one_past_payload": ("hcv", lambda r: r.end, ("hcv [out] guard after", "[0]")),
    "one_before_payload": ("room", lambda r: r.start - 1, ("room [inout] guard before", "[-1]")),
    "63_rows_past": ("room", lambda r: r.end + 62 * E + (E - 1), ("room [inout] guard after", f"[{63 * E - 1}]")),
    "63_rows_before": ("stats", lambda r: r.start - 63 * 28, ("stats [out] guard before", f"[{-63 * 28}]")),
    "input_changed": ("slot", lambda r: r.start + 5 * E + 7, ("slot [in] payload", f"[{5 * E + 7}]")),
    "int_input_changed": ("order", lambda r: r.start + 9, ("order [in] payload", "[9]")),
    "one_past_work": ("work", lambda r: r.start + WORK_BYTES, ("work [work] guard after", "[0]")),
}


@pytest.mark.parametrize("skews", [(0, 0), (3, 5)])
@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_fails(defect, skews):
    a, v = carve(*skews)
    clean_call(v)
    region, where, words = DEFECTS[defect]
    flip(a, where(a[region]))
    with pytest.raises(AssertionError) as e:
        a.check()
    for w in words:
        assert w in str(e.value), str(e.value)
    assert str(e.value).count("bytes changed") == 1      # nothing else reported


def test_a_write_of_the_same_value_is_the_only_blind_spot():
    """The prefill is random so that a stray store of a constant (0, 63, 255)
    meets a different byte almost everywhere: a row of 64 zeros past a payload
    is seen even where one of its bytes happens to equal the prefill."""
    a, v = carve()
    clean_call(v)
    r = a["hcv"]
    a.buf[r.end:r.end + 64] = 0
    with pytest.raises(AssertionError, match="hcv .out. guard after"):
        a.check()


def test_empty_payload():
    """A [0][E] array (no children): no bytes, guards of 64 rows all the same."""
    a = ar.Arena("cpu")
    a.add("child_slot", "in", "uint8", (0, E), np.zeros((0, E), np.uint8), skew=3)
    a.add("keep", "out", "uint8", (5,))
    v = a.build()
    a.snapshot()
    assert tuple(v["child_slot"].shape) == (0, E) and a["child_slot"].end == a["child_slot"].start
    assert a["child_slot"].guard == 64 * E
    v["keep"][:] = 1
    a.check()
    flip(a, a["child_slot"].start)
    with pytest.raises(AssertionError, match="child_slot"):
        a.check()


def test_misuse():
    a = ar.Arena("cpu")
    with pytest.raises(ValueError):
        a.add("x", "out", "int32", (4,), skew=1)         # only uint8 payloads take a skew
    with pytest.raises(ValueError):
        a.add("x", "in", "int32", (4,))                  # an input needs its value
    with pytest.raises(ValueError):
        a.add("x", "out", "int32", (4,), np.zeros(4, np.int32))
    with pytest.raises(ValueError):
        a.add("x", "in", "int32", (4,), np.zeros(4, np.int64))
    a.add("x", "out", "int32", (4,))
    a.build()
    with pytest.raises(RuntimeError):
        a.check()                                        # no snapshot
