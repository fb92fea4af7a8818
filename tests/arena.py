"""A guarded arena for the buffer contracts of the C ABI (imported like helpers;
no fixtures). Works on CPU and on CUDA tensors.

An Arena is ONE uint8 tensor filled with position-dependent bytes from a
fixed-seed generator. The arguments of one library call are carved from it as
regions: guard, payload of exactly the documented byte size, guard. A guard is
at least 4,096 bytes and at least 64 rows of its buffer, so a whole stray tile
of rows stays inside the allocation: the checker never depends on a fault and
cannot cause one. (Read overruns are invisible to guards and out of scope.)

Placement: a payload starts at its element type's alignment and no better --
an int32 payload at an address that is 4 (mod 8), an int64 or work payload at
8 (mod 16) -- and a uint8 payload at 0 (mod 256) plus a `skew` in bytes set
per region, so skew 0 is what torch's allocator gives and every other residue
can be asked for.

Roles: "in" (read-only), "inout", "out", "work". An "out" or "work" payload
keeps the arena's random prefill, so an output that was never written shows;
"in" and "inout" payloads take their initial value. snapshot() is taken before
the call; check() after it asserts that every byte outside the inout, out and
work payloads -- every guard and every "in" payload -- equals the snapshot.
"""
from __future__ import annotations

import numpy as np
import torch

MIN_GUARD = 4096
GUARD_ROWS = 64
ROLES = ("in", "inout", "out", "work")
_WRITABLE = ("inout", "out", "work")
_SEED = 0x7A11_0C8D

_DTYPES = {"uint8": torch.uint8, "int32": torch.int32, "int64": torch.int64}
# (modulus, residue) of a payload's first byte: the type's alignment and no better
_PLACE = {"uint8": (256, 0), "int32": (8, 4), "int64": (16, 8), "work": (16, 8)}


class Region:
    """One carved argument. lo..start: guard before; start..end: payload;
    end..hi: guard after (absolute byte offsets into the arena)."""

    def __init__(self, name, role, kind, shape, skew, init):
        self.name, self.role, self.kind, self.shape, self.skew, self.init = name, role, kind, shape, skew, init
        item = {"uint8": 1, "int32": 4, "int64": 8, "work": 1}[kind]
        self.itemsize = item
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * item
        self.row_bytes = (int(np.prod(shape[1:], dtype=np.int64)) if len(shape) > 1 else 1) * item
        self.guard = max(MIN_GUARD, GUARD_ROWS * self.row_bytes)
        self.lo = self.start = self.end = self.hi = -1
        self.view = None

    def __repr__(self):
        return f"Region({self.name!r}, {self.role}, {self.kind}{list(self.shape)}, payload {self.start}..{self.end})"


class Arena:
    def __init__(self, device="cpu"):
        self.device = torch.device(device)
        self.regions: list[Region] = []
        self.buf = None
        self.snap = None

    # -- describing the call ---------------------------------------------------
    def add(self, name, role, kind, shape, init=None, skew=0):
        """kind: "uint8", "int32", "int64" (typed views) or "work" (a uint8 view of
        `shape` = (bytes,), 8-byte placed). init: a numpy array for "in" and
        "inout" payloads (required there), none for "out" and "work"."""
        if self.buf is not None:
            raise RuntimeError("the arena is built: add every region first")
        if role not in ROLES or kind not in _PLACE:
            raise ValueError(f"unknown role {role!r} or kind {kind!r}")
        if any(r.name == name for r in self.regions):
            raise ValueError(f"region {name!r} twice")
        shape = (int(shape),) if np.isscalar(shape) else tuple(int(x) for x in shape)
        if skew and kind != "uint8":
            raise ValueError("only uint8 payloads take a skew")
        if (init is None) != (role in ("out", "work")):
            raise ValueError(f"{name}: 'in' and 'inout' regions take an initial value, 'out' and 'work' none")
        if init is not None:
            init = np.ascontiguousarray(init)
            if tuple(init.shape) != shape or init.dtype != np.dtype(kind):
                raise ValueError(f"{name}: init is {init.dtype}{list(init.shape)}, region {kind}{list(shape)}")
        self.regions.append(Region(name, role, kind, shape, int(skew), init))
        return self

    # -- carving ---------------------------------------------------------------
    def build(self):
        """Lays the regions out, allocates and fills the arena, writes the initial
        values and returns {name: typed contiguous view}."""
        pos = 0
        slack = 512                                     # the allocation's own base is not known yet
        for r in self.regions:
            r.lo = pos
            pos += r.guard + 512 + r.nbytes + r.guard   # room for the placement inside [lo, hi)
            r.hi = pos
        total = pos + slack
        g = torch.Generator(device="cpu").manual_seed(_SEED)
        fill = torch.randint(0, 256, (total,), dtype=torch.uint8, generator=g)
        # the arena starts at a multiple of 256 inside its allocation, so the layout (and with it
        # every byte of the arena) is the same whatever address the allocator gives
        raw = torch.empty(total + 256, dtype=torch.uint8, device=self.device)
        off = -raw.data_ptr() % 256
        self.buf = raw[off:off + total]
        self.buf.copy_(fill)
        base = self.buf.data_ptr()
        assert base % 256 == 0
        for r in self.regions:
            mod, res = _PLACE[r.kind]
            a = base + r.lo + r.guard
            a = (a + mod - 1) // mod * mod + res + r.skew
            r.start = a - base
            r.end = r.start + r.nbytes
            assert r.lo + r.guard <= r.start and r.end + r.guard <= r.hi
            raw = self.buf[r.start:r.end]
            v = raw if r.kind in ("uint8", "work") else raw.view(_DTYPES[r.kind])
            r.view = v.view(r.shape)
            # (an empty payload, a [0][E] array, has no address of its own)
            assert r.view.is_contiguous() and (r.nbytes == 0 or r.view.data_ptr() == base + r.start)
            if r.init is not None:
                r.view.copy_(torch.from_numpy(r.init).to(self.device))
        return {r.name: r.view for r in self.regions}

    def __getitem__(self, name):
        return next(r for r in self.regions if r.name == name)

    # -- checking ----------------------------------------------------------------
    def snapshot(self):
        self._sync()
        self.snap = self.buf.clone()

    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def check(self, untouched=False):
        """Every byte outside the inout, out and work payloads equals the
        snapshot (untouched=True: every byte of the arena, for a refused call)."""
        if self.snap is None:
            raise RuntimeError("snapshot() before the call, check() after it")
        self._sync()
        diff = self.buf != self.snap
        if not untouched:
            for r in self.regions:
                if r.role in _WRITABLE:
                    diff[r.start:r.end] = False
        bad = torch.nonzero(diff).flatten().cpu().numpy()
        if bad.size == 0:
            return
        lines = []
        for r in self.regions:
            for side, lo, hi, origin in (("guard before", r.lo, r.start, r.start), ("payload", r.start, r.end, r.start),
                                         ("guard after", r.end, r.hi, r.end)):
                hit = bad[(bad >= lo) & (bad < hi)]
                if hit.size:
                    rel = (hit[:8] - origin).tolist()
                    unit = f" (rows of {r.row_bytes} B)" if r.row_bytes > 1 else ""
                    lines.append(f"{r.name} [{r.role}] {side}: {hit.size} bytes changed, first offsets {rel} from the "
                                 f"{'end' if side == 'guard after' else 'start'} of the payload{unit}")
        tail = bad[bad >= (self.regions[-1].hi if self.regions else 0)]
        if tail.size:
            lines.append(f"arena tail: {tail.size} bytes changed, first at {tail[:8].tolist()}")
        raise AssertionError("bytes outside the writable payloads changed:\n  " + "\n  ".join(lines))
