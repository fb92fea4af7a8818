"""tests/large_rows.py on CPU tensors with a numpy stand-in for a per-row
kernel whose offset arithmetic is done modulo 2^w with w small, so that a
buffer of a few hundred kilobytes "wraps" the way a [P][E] population does at
2^31 or 2^32 bytes. The periodic check must report each planted defect -- a
wrapped read offset, a wrapped write offset, a signed wrap (a negative offset
clamped into the buffer), a [P] output index truncated to w bits, a wrap that is
a whole number of rows (E a power of two) -- with exactly the rows a row-by-row
comparison against the correct stand-in finds, and nothing for the correct
stand-in. Also the formula for P and the helpers' slab arithmetic."""
import numpy as np
import pytest
import torch

import large_rows as lr

M = 131                            # the base block of these tests: a prime
W = 18                             # the "line": offsets wrap at 2^18 bytes
LINE = 1 << W


def base_block(E, seed=5):
    """M pairwise distinct random rows and a seed for each."""
    g = np.random.default_rng(seed)
    rows = g.integers(0, 45, (M, E), dtype=np.uint8)
    assert len({r.tobytes() for r in rows}) == M
    return rows, g.permutation(1 << 20)[:M].astype(np.int64) + 1


def standin(rows, seeds, read_bits=None, write_bits=None, vec_bits=None, signed=False):
    """A per-row "kernel" over flat buffers: out[i] = (7 * in[i] + 3) % 251 (never
    the sentinel 255) and tot[i] = sum(in[i]) + seeds[i] (never the sentinel -1),
    row i at byte offset i * E of the [P][E] buffers and 4 * i of tot. Each
    offset is reduced to the given number of bits before use (None: not at all);
    with `signed` the reduced value is read as a two's-complement number and a
    negative one is clamped to 0. Stores happen in row order."""
    P, E = rows.shape
    flat = rows.reshape(-1)
    out = np.full(P * E, 255, np.uint8)
    tot = np.full(P, -1, np.int32)

    def reduce(off, bits, last):
        if bits is None:
            return off
        off = off & ((1 << bits) - 1)
        if signed:
            off = np.where(off >= 1 << (bits - 1), off - (1 << bits), off)
        return np.clip(off, 0, last)

    off = np.arange(P, dtype=np.int64) * E
    cols = np.arange(E, dtype=np.int64)
    src = flat[reduce(off, read_bits, (P - 1) * E)[:, None] + cols]
    val = ((src.astype(np.int64) * 7 + 3) % 251).astype(np.uint8)
    sums = (src.sum(axis=1) + seeds).astype(np.int32)
    dst = reduce(off, write_bits, (P - 1) * E)
    vec = reduce(4 * np.arange(P, dtype=np.int64), vec_bits, 4 * (P - 1)) // 4
    for i in range(P):                                         # row order: a later store wins
        out[dst[i]:dst[i] + E] = val[i]
        tot[vec[i]] = sums[i]
    return out.reshape(P, E), tot


DEFECTS = {
    # name: (E, the stand-in's defect, must a row below the line fail too)
    "wrapped_read": (61, dict(read_bits=W), False),
    "wrapped_write": (61, dict(write_bits=W), True),
    "signed_read_clamped": (61, dict(read_bits=W + 1, signed=True), False),
    "signed_write_clamped": (61, dict(write_bits=W + 1, signed=True), True),
    "truncated_vector_index": (61, dict(vec_bits=14), True),
    "whole_rows_read": (64, dict(read_bits=W), False),
    "whole_rows_write": (64, dict(write_bits=W), True),
}


def periodic_case(E):
    rows, seeds = base_block(E)
    P = lr.rows_past(LINE, E, M)
    big_rows = lr.tile_rows(torch.from_numpy(rows), P).numpy()
    big_seeds = lr.tile_rows(torch.from_numpy(seeds), P).numpy()
    assert np.array_equal(big_rows, rows[np.arange(P) % M]) and np.array_equal(big_seeds, seeds[np.arange(P) % M])
    return rows, seeds, big_rows, big_seeds, P


def failing(big, base):
    return lr.mismatched_rows(torch.from_numpy(big), torch.from_numpy(base)).numpy()


@pytest.mark.parametrize("E", [61, 64])
def test_correct_standin_passes(E):
    rows, seeds, big_rows, big_seeds, P = periodic_case(E)
    base_out, base_tot = standin(rows, seeds)
    out, tot = standin(big_rows, big_seeds)
    assert P * E >= LINE + M * E and (out != 255).all() and (tot != -1).all()
    assert failing(out, base_out).size == 0 and failing(tot, base_tot).size == 0
    lr.assert_periodic(torch.from_numpy(out), torch.from_numpy(base_out), "out")


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_is_reported(defect):
    E, how, low_row_too = DEFECTS[defect]
    rows, seeds, big_rows, big_seeds, P = periodic_case(E)
    base_out, base_tot = standin(rows, seeds)                  # the small call: nothing wraps at M rows
    assert all(np.array_equal(a, b) for a, b in zip(standin(rows, seeds, **how), (base_out, base_tot)))
    right_out, right_tot = standin(big_rows, big_seeds)
    out, tot = standin(big_rows, big_seeds, **how)
    got = np.union1d(failing(out, base_out), failing(tot, base_tot))
    want = np.flatnonzero((out != right_out).any(axis=1) | (tot != right_tot))
    assert np.array_equal(got, want)                           # every wrong row, no other
    # the first row whose offset needs bit W (signed: W is the sign bit), or whose 4 * i needs bit 14
    first_past = -(-LINE // E) if "vec_bits" not in how else (1 << 14) // 4
    assert (got >= first_past).sum() >= M - 1                  # a whole period past the line, bar a coincidence
    assert ((got < first_past).any()) == low_row_too
    if E == 64:
        assert LINE % E == 0 and (LINE // E) % M != 0          # a whole number of rows, never of periods
    # assert_periodic raises for each output that is wrong, and only for that one
    for name, big, base, right in (("out", out, base_out, right_out), ("tot", tot, base_tot, right_tot)):
        if np.array_equal(big, right):
            lr.assert_periodic(torch.from_numpy(big), torch.from_numpy(base), f"{defect}: {name}")
        else:
            with pytest.raises(AssertionError, match=f"{defect}: {name}: .* rows differ from the base block"):
                lr.assert_periodic(torch.from_numpy(big), torch.from_numpy(base), f"{defect}: {name}")


def test_a_missed_store_shows_through_the_sentinel():
    """A wrapped write leaves the rows past the line as they were filled: the
    sentinel, which no call produces, so the row fails whatever it should hold."""
    rows, seeds, big_rows, big_seeds, P = periodic_case(61)
    out, _ = standin(big_rows, big_seeds, write_bits=W)
    past = np.arange(-(-LINE // 61), P)
    assert (out[past] == 255).all() and np.isin(past, failing(out, standin(rows, seeds)[0])).all()


@pytest.mark.parametrize("line", [1 << 30, 1 << 31, 1 << 32])
def test_rows_past_the_line(line):
    bumped = 0
    for E in list(range(1, 3000)) + [4096, 65535]:
        P = lr.rows_past(line, E)
        assert (P - lr.M_ROWS) * E >= line                     # one full period lies past the line
        assert (P - lr.M_ROWS - 5) * E < line                  # and not much more than one
        assert P % 64 != 0                                     # the last 64-row tile is partial
        assert P * E > line // 2                               # the line at half of it lies inside
        plain = -(-line // E) + lr.M_ROWS + 3
        assert P == plain + (plain % 64 == 0)
        bumped += plain % 64 == 0
    assert bumped > 10                                         # the one-more-row rule was exercised
    assert lr.is_prime(lr.M_ROWS) and lr.is_prime(M)
    assert lr.rows_past(1 << 32, 448) == 9_591_083 and lr.rows_past(1 << 32, 2000) == 2_151_586


@pytest.mark.parametrize("shape", [(), (7,), (6, 3)])
@pytest.mark.parametrize("slab", [1, 1000, 1 << 28])
def test_slabs_cover_every_row(shape, slab):
    """tile_rows and mismatched_rows with slabs of less than a period, of a few
    and of all of them: a single changed element is found in the first row, at
    every slab border and in the partial last period, and nowhere else."""
    m, P = 13, 13 * 9 + 5
    base = torch.arange(m * int(np.prod(shape, dtype=np.int64)), dtype=torch.int32).reshape((m,) + shape)
    big = lr.tile_rows(base, P, slab_bytes=slab)
    assert torch.equal(big, base[torch.arange(P) % m])
    assert lr.mismatched_rows(big, base, slab_bytes=slab).numel() == 0
    for row in (0, 12, 13, 64, P - 6, P - 5, P - 1):
        x = big.clone()
        x[row].reshape(-1)[-1] += 1
        assert lr.mismatched_rows(x, base, slab_bytes=slab).tolist() == [row]
    x = big.clone()
    x += 1
    assert lr.mismatched_rows(x, base, slab_bytes=slab).tolist() == list(range(P))
