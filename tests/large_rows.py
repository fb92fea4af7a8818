"""The periodic-population check for buffers past 2^31 and 2^32 bytes.

No CPU model evaluates ten million rows, and none has to. A *base block* of M
pairwise distinct rows (M prime) is repeated down a big population: row i of
every [P][E] and [P] input is base row i mod M. An entry point that gives row i
a result that depends on row i's inputs alone must then return outputs of
period M that equal its own outputs from a call with P = M on fresh small
buffers, and that small call is what the oracle and the Python models judge.

A row address that wraps at 2^k bytes reads or writes row i - 2^k / E: another
base row (M is prime, so no power-of-two distance is a multiple of it), or the
middle of one where E does not divide 2^k. Out-of-place outputs start as a
sentinel no call produces, so a store that went elsewhere shows at the row it
missed as well as at the row it hit.

mismatched_rows() compares the whole buffer, slab by slab, where the buffer
lives (torch CPU or CUDA tensors), and returns every failing row: it never
samples. Nothing here needs a GPU; tests/test_large_rows_cpu.py plants the
defects it must catch.
"""
import torch

M_ROWS = 4099                      # rows of the base block: a prime
SLAB_BYTES = 1 << 28               # bytes of the big buffer compared (or filled) at a time
HEADROOM = 4 << 30                 # device memory a case leaves free (GPU tests)


def is_prime(n):
    return n >= 2 and all(n % d for d in range(2, int(n ** 0.5) + 1))


def rows_past(line_bytes, row_bytes, M=M_ROWS):
    """The rows of a population whose [P][row_bytes] buffer passes `line_bytes`
    by at least one full period: ceil(line / row_bytes) + M + 3, and one more
    where that is a multiple of 64 (so that the last 64-row tile is partial)."""
    P = -(-line_bytes // row_bytes) + M + 3
    return P + 1 if P % 64 == 0 else P


def _periods(base, slab_bytes):
    """Whole periods per slab: at least one."""
    per = base.numel() * base.element_size()
    return max(1, slab_bytes // max(per, 1))


def tile_rows(base, P, out=None, slab_bytes=SLAB_BYTES):
    """A [P, ...] tensor on base's device whose row i is base[i % M], written
    into `out` if given."""
    M = base.shape[0]
    if out is None:
        out = torch.empty((P,) + tuple(base.shape[1:]), dtype=base.dtype, device=base.device)
    assert out.shape[0] == P and out.shape[1:] == base.shape[1:] and out.is_contiguous()
    n = _periods(base, slab_bytes)
    j = 0
    while j < P:
        k = min(n, (P - j) // M)
        if k == 0:                                             # the partial last period
            out[j:].copy_(base[:P - j])
            break
        out[j:j + k * M].view((k, M) + tuple(base.shape[1:])).copy_(base.unsqueeze(0).expand(k, *base.shape))
        j += k * M
    return out


def mismatched_rows(big, base, slab_bytes=SLAB_BYTES):
    """The rows i of `big` ([P, ...]) that differ from base[i % M] ([M, ...]),
    ascending, as an int64 tensor on the host. Every row is compared; a slab of
    whole periods at a time is broadcast against the base block on big's
    device, so there is no full-size temporary and no synchronisation per row
    (one, for the result)."""
    P, M = big.shape[0], base.shape[0]
    assert big.shape[1:] == base.shape[1:] and big.dtype == base.dtype and big.device == base.device, \
        (big.shape, base.shape, big.dtype, base.dtype)
    assert big.is_contiguous()
    bad = torch.zeros(P, dtype=torch.bool, device=big.device)
    n = _periods(base, slab_bytes)
    j = 0
    while j < P:
        k = min(n, (P - j) // M)
        if k == 0:
            ne, k_rows = big[j:] != base[:P - j], P - j
            bad[j:] = ne.reshape(k_rows, -1).any(dim=1)
            break
        ne = big[j:j + k * M].view((k, M) + tuple(base.shape[1:])) != base.unsqueeze(0)
        bad[j:j + k * M] = ne.reshape(k * M, -1).any(dim=1)
        j += k * M
    return torch.nonzero(bad).flatten().cpu()


def describe(rows, M, limit=8):
    """The first few failing rows in words, each with its base row."""
    return ", ".join(f"{int(r)} (base {int(r) % M})" for r in rows[:limit]) + (", ..." if len(rows) > limit else "")


def assert_periodic(big, base, what):
    rows = mismatched_rows(big, base)
    assert rows.numel() == 0, f"{what}: {rows.numel()} of {big.shape[0]} rows differ from the base block's: " \
                              f"{describe(rows, base.shape[0])}"


def need_device_memory(nbytes):
    """Skips the calling test where the device has less free memory than the
    case's `nbytes` plus the headroom; the reason says so."""
    import pytest
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + HEADROOM:
        pytest.skip(f"torch.cuda.mem_get_info() reports {free / 2 ** 30:.1f} GiB free; the case needs "
                    f"{nbytes / 2 ** 30:.1f} GiB plus {HEADROOM / 2 ** 30:.0f} GiB of headroom")
