"""ctypes binding of libttga.so (include/ttga.h) for device-resident populations.

There is no CPU fallback anywhere in this module: if the HIP library is missing
or the device calls fail, every entry point raises. Tensors are torch CUDA
(=HIP) tensors; calls are enqueued on torch's current stream of the tensor's
device.
"""
from __future__ import annotations

import ctypes
import os
import pathlib

import numpy as np

PKG_DIR = pathlib.Path(__file__).resolve().parent.parent
LIB_PATH = PKG_DIR / "libttga.so"

TT_OK, TT_ERR_INVALID, TT_ERR_DEVICE, TT_ERR_LIMIT = 0, 1, 2, 3
NUM_SLOTS = 45

EXPORTS = (
    "tt_problem_create", "tt_problem_destroy", "tt_problem_dims", "tt_problem_derived", "tt_eval",
    "tt_eval_variant", "tt_assign_rooms", "tt_random_init", "tt_crossover", "tt_mutation", "tt_local_search",
    "tt_device_status", "tt_last_error", "tt_version", "tt_ga_breed", "tt_ga_work_bytes", "tt_ga_replace",
    "tt_eval_auto_variant", "tt_local_search_ordered", "tt_lpt_order", "tt_ga_work_source_offset",
    "tt_local_search_stats", "tt_local_search_masks", "tt_local_search_eval",
)

# include/ttga_report.h
REPORT_EXPORTS = ("tt_eval_parts", "tt_slot_histogram")
PART_NAMES = ("room_pairs", "corr_pairs", "unsuitable", "last_slot", "consecutive", "single_class")

# include/ttga_unique.h
UNIQUE_EXPORTS = ("tt_genome_work_bytes", "tt_genome_first", "tt_ga_unique_work_bytes", "tt_ga_replace_unique")

# include/ttga_greedy.h
GREEDY_EXPORTS = ("tt_greedy_work_bytes", "tt_greedy_order", "tt_greedy_init")

# include/ttga_kempe.h
KEMPE_EXPORTS = ("tt_kempe_move",)

# include/ttga_slotswap.h
SLOTSWAP_EXPORTS = ("tt_slot_swap",)

# include/ttga_lahc.h
LAHC_EXPORTS = ("tt_lahc",)

# include/ttga_lahc_kempe.h (brought in by ttga_lahc.h)
LAHC_KEMPE_EXPORTS = ("tt_lahc_kempe",)

# include/ttga_lahc_kempe_aug.h (brought in by ttga_lahc.h)
LAHC_KEMPE_AUG_EXPORTS = ("tt_lahc_kempe_aug",)
ROOM_RULES = ("direct", "augment")          # tt_lahc_kempe_aug's room_rule 0 and 1

# include/ttga_lahc_multi.h (brought in by ttga_lahc.h)
LAHC_MULTI_EXPORTS = ("tt_lahc_multi_work_bytes", "tt_lahc_multi")
MAX_WALKERS = 1024                          # tt_lahc_multi's walkers: 1 .. 1024

# include/ttga_cx.h
CX_EXPORTS = ("tt_crossover_guided", "tt_ga_breed_guided")

# include/ttga/move1.h
MOVE1_EXPORTS = ("tt_move1_scan", "tt_move1_descent")
MOVE1_CLASH, MOVE1_NO_ROOM, MOVE1_UNSCANNED, MOVE1_NONE = 255, 254, 253, 0x7FFFFFFF

_lib = None


class TTError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"ttga error {code}: {msg}")
        self.code = code


def load(path: os.PathLike | str | None = None) -> ctypes.CDLL:
    """Load libttga.so (built in-tree by `make -C timetabling-ga-mpi-openmp_amd`)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = pathlib.Path(path) if path else LIB_PATH
    if not p.exists():
        raise FileNotFoundError(f"{p} not built: run `make -C {PKG_DIR}` (hipcc --offload-arch=gfx950)")
    lib = ctypes.CDLL(str(p))
    vp, i32, dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    P = ctypes.POINTER
    lib.tt_problem_create.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, i32, P(vp)]
    lib.tt_problem_destroy.argtypes = [vp]
    lib.tt_problem_dims.argtypes = [vp, vp]
    lib.tt_problem_derived.argtypes = [vp, vp, vp, vp]
    lib.tt_eval.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.tt_eval_variant.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, i32, vp]
    lib.tt_assign_rooms.argtypes = [vp, vp, vp, i32, vp]
    lib.tt_random_init.argtypes = [vp, vp, vp, vp, i32, vp]
    lib.tt_crossover.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp]
    lib.tt_mutation.argtypes = [vp, vp, vp, vp, i32, vp]
    lib.tt_local_search.argtypes = [vp, vp, vp, vp, i32, i32, dbl, dbl, dbl, vp]
    lib.tt_local_search_ordered.argtypes = [vp, vp, vp, vp, i32, i32, dbl, dbl, dbl, vp, vp]
    lib.tt_lpt_order.argtypes = [vp, vp, i32, vp, vp, vp]
    lib.tt_local_search_stats.argtypes = [vp, vp, vp]
    lib.tt_local_search_masks.argtypes = [vp, vp, vp]
    lib.tt_local_search_eval.argtypes = [vp, vp, vp, vp, i32, i32, dbl, dbl, dbl, vp, vp, vp, vp, vp, vp]
    lib.tt_device_status.argtypes = [vp, vp]
    lib.tt_eval_auto_variant.argtypes = [vp]
    lib.tt_ga_breed.argtypes = [vp, vp, vp, vp, i32, vp, i32, dbl, dbl, i32, vp, vp, vp, vp]
    lib.tt_ga_work_bytes.argtypes = [i32, i32]
    lib.tt_ga_work_bytes.restype = ctypes.c_size_t
    lib.tt_ga_work_source_offset.argtypes = [i32, i32]
    lib.tt_ga_work_source_offset.restype = ctypes.c_size_t
    lib.tt_ga_replace.argtypes = [vp] * 7 + [i32] + [vp] * 6 + [i32, vp, vp]
    lib.tt_last_error.restype = ctypes.c_char_p
    lib.tt_last_error.argtypes = []
    lib.tt_version.argtypes = []
    lib.tt_eval_parts.argtypes = [vp, vp, vp, i32, vp, vp, vp]
    lib.tt_slot_histogram.argtypes = [vp, vp, i32, vp, vp]
    for name in REPORT_EXPORTS:
        getattr(lib, name).restype = ctypes.c_int
    lib.tt_genome_work_bytes.argtypes = [i32, i32]
    lib.tt_genome_work_bytes.restype = ctypes.c_size_t
    lib.tt_genome_first.argtypes = [vp, vp, vp, i32, vp, i32, vp, vp]
    lib.tt_genome_first.restype = ctypes.c_int
    lib.tt_ga_unique_work_bytes.argtypes = [i32, i32, i32]
    lib.tt_ga_unique_work_bytes.restype = ctypes.c_size_t
    lib.tt_ga_replace_unique.argtypes = [vp] * 7 + [i32] + [vp] * 6 + [i32, vp, vp, i32, vp, vp]
    lib.tt_ga_replace_unique.restype = ctypes.c_int
    lib.tt_greedy_work_bytes.argtypes = [vp]
    lib.tt_greedy_work_bytes.restype = ctypes.c_size_t
    lib.tt_greedy_order.argtypes = [vp, vp, vp, vp]
    lib.tt_greedy_order.restype = ctypes.c_int
    lib.tt_greedy_init.argtypes = [vp, vp, vp, vp, vp, i32, vp]
    lib.tt_greedy_init.restype = ctypes.c_int
    lib.tt_kempe_move.argtypes = [vp, vp, vp, vp, i32, dbl, i32, vp, vp]
    lib.tt_kempe_move.restype = ctypes.c_int
    lib.tt_slot_swap.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.tt_slot_swap.restype = ctypes.c_int
    lib.tt_lahc.argtypes = [vp, vp, vp, vp, i32, i32, i32, dbl, vp, vp, vp, vp, vp, vp]
    lib.tt_lahc.restype = ctypes.c_int
    lib.tt_lahc_kempe.argtypes = [vp, vp, vp, vp, i32, i32, i32, dbl, dbl, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.tt_lahc_kempe.restype = ctypes.c_int
    lib.tt_lahc_kempe_aug.argtypes = [vp, vp, vp, vp, i32, i32, i32, dbl, dbl, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.tt_lahc_kempe_aug.restype = ctypes.c_int
    lib.tt_lahc_multi_work_bytes.argtypes = [vp, i32, i32]
    lib.tt_lahc_multi_work_bytes.restype = ctypes.c_size_t
    lib.tt_lahc_multi.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, dbl, dbl, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp,
                                  vp, vp]
    lib.tt_lahc_multi.restype = ctypes.c_int
    lib.tt_crossover_guided.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp]
    lib.tt_crossover_guided.restype = ctypes.c_int
    lib.tt_ga_breed_guided.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, dbl, dbl, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.tt_ga_breed_guided.restype = ctypes.c_int
    lib.tt_move1_scan.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp]
    lib.tt_move1_scan.restype = ctypes.c_int
    lib.tt_move1_descent.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]
    lib.tt_move1_descent.restype = ctypes.c_int
    for name in EXPORTS:
        if name not in ("tt_last_error", "tt_ga_work_bytes", "tt_ga_work_source_offset"):
            getattr(lib, name).restype = ctypes.c_int
    if path is None:
        _lib = lib
    return lib


def _check(lib, rc: int):
    if rc != TT_OK:
        raise TTError(rc, lib.tt_last_error().decode(errors="replace"))


def _np_ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def _ptr(t):
    """The address of an optional tensor: NULL for None."""
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def _opt_i32(name, t, n, what, device):
    """An optional int32 output of n entries (`what` in words) on the population's device."""
    import torch
    if t is not None and not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n
                              and t.device == device):
        raise ValueError(f"{name} must be a contiguous int32 CUDA tensor of {what} entries on the population's device")


class DeviceProblem:
    """A tt_problem handle: the Problem image resident on one GPU."""

    def __init__(self, inst, device: int = 0):
        self.lib = load()
        self.inst = inst
        self.device = device
        self.E, self.R, self.F, self.S = inst.E, inst.R, inst.F, inst.S
        h = ctypes.c_void_p()
        rs, A = inst.room_size, inst.student_events
        rf, ef = inst.room_features, inst.event_features
        _check(self.lib, self.lib.tt_problem_create(self.E, self.R, self.F, self.S, _np_ptr(rs), _np_ptr(A),
                                                    _np_ptr(rf), _np_ptr(ef), device, ctypes.byref(h)))
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.lib.tt_problem_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def derived(self):
        sn = np.zeros(self.E, np.int32)
        corr = np.zeros((self.E, self.E), np.int32)
        poss = np.zeros((self.E, self.R), np.int32)
        _check(self.lib, self.lib.tt_problem_derived(self.handle, _np_ptr(sn), _np_ptr(corr), _np_ptr(poss)))
        return sn, corr, poss

    def eval_variant(self) -> int:
        """The kernel tt_eval runs for this instance (tt_eval_variant numbering)."""
        return int(self.lib.tt_eval_auto_variant(self.handle))

    def status(self) -> int:
        v = ctypes.c_int32(0)
        _check(self.lib, self.lib.tt_device_status(self.handle, ctypes.byref(v)))
        return int(v.value)

    # -- population operations (torch tensors on this device) -------------------
    @staticmethod
    def _stream(t, stream=None):
        # note: every library call makes the handle's device current (hipSetDevice)
        # and leaves it so; tensors of another device are rejected by _pop/_rng
        import torch
        st = torch.cuda.current_stream(t.device) if stream is None else stream
        return ctypes.c_void_p(st.cuda_stream)

    def _pop(self, slot, room=None):
        import torch
        for t in (slot, room):
            if t is None:
                continue
            if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == self.E):
                raise ValueError("population tensors must be contiguous uint8 CUDA tensors of shape [P, E]")
            if t.device.index != self.device:
                raise ValueError(f"tensor on cuda:{t.device.index}, problem handle on cuda:{self.device}")
        return slot.shape[0]

    def eval(self, slot, room, variant: int = 0, out=None):
        import torch
        P = self._pop(slot, room)
        if out is None:
            dev = slot.device
            out = (torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev),
                   torch.empty(P, dtype=torch.uint8, device=dev), torch.empty(P, dtype=torch.int32, device=dev))
        hcv, scv, feas, pen = out
        _check(self.lib, self.lib.tt_eval_variant(self.handle, slot.data_ptr(), room.data_ptr(), P, hcv.data_ptr(),
                                                  scv.data_ptr(), feas.data_ptr(), pen.data_ptr(), variant,
                                                  self._stream(slot)))
        return out

    def eval_parts(self, slot, room, event_hcv: bool = False, out=None):
        """tt_eval_parts: the six constraint parts (PART_NAMES order) of every
        individual as an int32 [P, 6] tensor (`out`, if given); with event_hcv
        also Solution::eventHcv of every event, int32 [P, E]."""
        import torch
        P = self._pop(slot, room)
        if out is None:
            out = torch.empty((P, len(PART_NAMES)), dtype=torch.int32, device=slot.device)
        elif not (out.is_cuda and out.dtype == torch.int32 and out.is_contiguous()
                  and tuple(out.shape) == (P, len(PART_NAMES)) and out.device == slot.device):
            raise ValueError("out must be a contiguous int32 CUDA tensor of shape [P, 6] on the population's device")
        eh = torch.empty((P, self.E), dtype=torch.int32, device=slot.device) if event_hcv else None
        _check(self.lib, self.lib.tt_eval_parts(self.handle, slot.data_ptr(), room.data_ptr(), P, out.data_ptr(),
                                                ctypes.c_void_p(eh.data_ptr() if event_hcv else None),
                                                self._stream(slot)))
        return (out, eh) if event_hcv else out

    def slot_histogram(self, slot):
        """tt_slot_histogram: int32 [E, 45], the individuals with each event in each slot."""
        import torch
        P = self._pop(slot)
        hist = torch.empty((self.E, NUM_SLOTS), dtype=torch.int32, device=slot.device)
        _check(self.lib, self.lib.tt_slot_histogram(self.handle, slot.data_ptr(), P, hist.data_ptr(),
                                                    self._stream(slot)))
        return hist

    def assign_rooms(self, slot, room=None):
        import torch
        P = self._pop(slot, room)
        if room is None:
            room = torch.empty_like(slot)
        _check(self.lib, self.lib.tt_assign_rooms(self.handle, slot.data_ptr(), room.data_ptr(), P, self._stream(slot)))
        return room

    def random_init(self, rng, slot, room):
        P = self._pop(slot, room)
        self._rng(rng, P)
        _check(self.lib, self.lib.tt_random_init(self.handle, rng.data_ptr(), slot.data_ptr(), room.data_ptr(), P,
                                                 self._stream(slot)))

    def crossover(self, slot1, slot2, rng, slot, room):
        P = self._pop(slot, room)
        self._pop(slot1, slot2)
        self._rng(rng, P)
        _check(self.lib, self.lib.tt_crossover(self.handle, slot1.data_ptr(), slot2.data_ptr(), rng.data_ptr(),
                                               slot.data_ptr(), room.data_ptr(), P, self._stream(slot)))

    def mutation(self, slot, room, rng):
        P = self._pop(slot, room)
        self._rng(rng, P)
        _check(self.lib, self.lib.tt_mutation(self.handle, slot.data_ptr(), room.data_ptr(), rng.data_ptr(), P,
                                              self._stream(slot)))

    def local_search(self, slot, room, rng, max_steps: int, p1=1.0, p2=1.0, p3=0.0, order=None, out=None):
        """order: optional int32 device permutation, the dispatch order (results unchanged).
        out: optional (hcv, scv, feasible, penalty) device tensors of P entries, filled with
        the searched individuals' evaluation in the same launch (tt_local_search_eval)."""
        import torch
        P = self._pop(slot, room)
        self._rng(rng, P)
        if out is not None:
            if order is not None and not (order.is_cuda and order.dtype == torch.int32 and order.is_contiguous()
                                          and order.numel() == P):
                raise ValueError("order must be a contiguous int32 CUDA tensor of P entries")
            hcv, scv, feas, pen = out
            for t, dt in ((hcv, torch.int32), (scv, torch.int32), (feas, torch.uint8), (pen, torch.int32)):
                if not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == P):
                    raise ValueError("out must be contiguous CUDA tensors (int32, int32, uint8, int32) of P entries")
            _check(self.lib, self.lib.tt_local_search_eval(
                self.handle, slot.data_ptr(), room.data_ptr(), rng.data_ptr(), P, int(max_steps), float(p1),
                float(p2), float(p3), ctypes.c_void_p(order.data_ptr() if order is not None else None),
                hcv.data_ptr(), scv.data_ptr(), feas.data_ptr(), pen.data_ptr(), self._stream(slot)))
            return
        if order is None:
            _check(self.lib, self.lib.tt_local_search(self.handle, slot.data_ptr(), room.data_ptr(), rng.data_ptr(),
                                                      P, int(max_steps), float(p1), float(p2), float(p3),
                                                      self._stream(slot)))
            return
        if not (order.is_cuda and order.dtype == torch.int32 and order.is_contiguous() and order.numel() == P):
            raise ValueError("order must be a contiguous int32 CUDA tensor of P entries")
        _check(self.lib, self.lib.tt_local_search_ordered(self.handle, slot.data_ptr(), room.data_ptr(),
                                                          rng.data_ptr(), P, int(max_steps), float(p1), float(p2),
                                                          float(p3), ctypes.c_void_p(order.data_ptr()),
                                                          self._stream(slot)))

    def local_search_stats(self, stream=None):
        """(phase-2 steps, all steps) of the last tt_local_search call on the
        stream (torch's current stream by default); waits for that call's
        counts (diagnostics)."""
        import torch
        st = torch.cuda.current_stream(self.device) if stream is None else stream
        out = (ctypes.c_ulonglong * 2)()
        _check(self.lib, self.lib.tt_local_search_stats(self.handle, ctypes.c_void_p(st.cuda_stream), out))
        return int(out[0]), int(out[1])

    def local_search_masks(self, stream=None) -> int:
        """Students with phase-2 masks in the last tt_local_search call's first
        launch on the stream (0: none, -1: no call yet; diagnostics)."""
        import torch
        st = torch.cuda.current_stream(self.device) if stream is None else stream
        out = ctypes.c_int32(0)
        _check(self.lib, self.lib.tt_local_search_masks(self.handle, ctypes.c_void_p(st.cuda_stream),
                                                        ctypes.byref(out)))
        return int(out.value)

    def lpt_order(self, key, work):
        """tt_lpt_order: indices of key (int32 CUDA) by key descending, ties by
        index, negative keys last, as an int32 CUDA tensor."""
        import torch
        n = key.numel()
        if not (key.is_cuda and key.dtype == torch.int32 and key.is_contiguous()):
            raise ValueError("key must be a contiguous int32 CUDA tensor")
        order = torch.empty(n, dtype=torch.int32, device=key.device)
        _check(self.lib, self.lib.tt_lpt_order(self.handle, ctypes.c_void_p(key.data_ptr()), n,
                                               ctypes.c_void_p(order.data_ptr()), ctypes.c_void_p(work.data_ptr()),
                                               self._stream(key)))
        return order

    # -- GA generation primitives ---------------------------------------------------
    def ga_breed(self, pop_slot, pop_room, pop_penalty, rng, child_slot, child_room, child_flags,
                 p_cross=0.8, p_mut=0.5, skip_init_draws=True):
        N = self._pop(pop_slot, pop_room)
        C = self._pop(child_slot, child_room)
        self._rng(rng, C)
        _check(self.lib, self.lib.tt_ga_breed(self.handle, pop_slot.data_ptr(), pop_room.data_ptr(),
                                              pop_penalty.data_ptr(), N, rng.data_ptr(), C, float(p_cross),
                                              float(p_mut), int(bool(skip_init_draws)), child_slot.data_ptr(),
                                              child_room.data_ptr(), child_flags.data_ptr(), self._stream(pop_slot)))

    def ga_work(self, N):
        import torch
        return torch.empty(int(self.lib.tt_ga_work_bytes(N, self.E)), dtype=torch.uint8,
                           device=torch.device("cuda", self.device))

    def ga_work_source(self, work, N) -> int:
        """The merged position tt_ga_replace's new pop[0] came from (synchronises)."""
        import torch
        off = int(self.lib.tt_ga_work_source_offset(N, self.E))
        return int(work[off:off + 4].view(torch.int32)[0].item())

    def ga_replace(self, pop, child, work):
        """pop/child: dicts of device tensors slot, room, hcv, scv, feasible, penalty."""
        N = self._pop(pop["slot"], pop["room"])
        C = self._pop(child["slot"], child["room"]) if child is not None else 0
        c = child or {k: pop[k] for k in pop}
        _check(self.lib, self.lib.tt_ga_replace(
            self.handle, pop["slot"].data_ptr(), pop["room"].data_ptr(), pop["hcv"].data_ptr(),
            pop["scv"].data_ptr(), pop["feasible"].data_ptr(), pop["penalty"].data_ptr(), N,
            c["slot"].data_ptr(), c["room"].data_ptr(), c["hcv"].data_ptr(), c["scv"].data_ptr(),
            c["feasible"].data_ptr(), c["penalty"].data_ptr(), C, work.data_ptr(), self._stream(pop["slot"])))

    # -- duplicate-free replacement (include/ttga_unique.h) ---------------------------
    def genome_first(self, slot, room, hash_bits: int = 0):
        """tt_genome_first: int32 [P], first[i] = the lowest j <= i whose genome
        (slot row + room row) equals i's; first[i] == i for the first of each kind."""
        import torch
        P = self._pop(slot, room)
        first = torch.empty(P, dtype=torch.int32, device=slot.device)
        work = torch.empty(int(self.lib.tt_genome_work_bytes(P, self.E)), dtype=torch.uint8, device=slot.device)
        _check(self.lib, self.lib.tt_genome_first(self.handle, slot.data_ptr(), room.data_ptr(), P, first.data_ptr(),
                                                  int(hash_bits), ctypes.c_void_p(work.data_ptr() if P else None),
                                                  self._stream(slot)))
        return first

    def ga_unique_work(self, N, C):
        """Work buffer of ga_replace_unique for N members and up to C children."""
        import torch
        return torch.empty(int(self.lib.tt_ga_unique_work_bytes(N, C, self.E)), dtype=torch.uint8,
                           device=torch.device("cuda", self.device))

    def ga_replace_unique(self, pop, child, work, keep=None, n_kept=None, hash_bits: int = 0):
        """tt_ga_replace_unique: ga_replace with the children dropped whose genome
        is already in the population or in a child with a lower index. Returns
        (keep uint8 [C], n_kept int32 [1]) device tensors; ga_work_source(work, N)
        is then a member's old position p < N or N + c for child c. `work` comes
        from ga_unique_work(N, C') with C' >= C."""
        import torch
        N = self._pop(pop["slot"], pop["room"])
        C = self._pop(child["slot"], child["room"]) if child is not None else 0
        dev = pop["slot"].device
        if keep is None:
            keep = torch.empty(C, dtype=torch.uint8, device=dev)
        elif not (keep.is_cuda and keep.dtype == torch.uint8 and keep.is_contiguous() and tuple(keep.shape) == (C,)
                  and keep.device == dev):
            raise ValueError("keep must be a contiguous uint8 CUDA tensor of shape [C] on the population's device")
        if n_kept is None:
            n_kept = torch.empty(1, dtype=torch.int32, device=dev)
        elif not (n_kept.is_cuda and n_kept.dtype == torch.int32 and n_kept.is_contiguous() and n_kept.numel() == 1
                  and n_kept.device == dev):
            raise ValueError("n_kept must be a contiguous int32 CUDA tensor of one entry on the population's device")
        if not (work.is_cuda and work.dtype == torch.uint8 and work.is_contiguous() and work.device == dev
                and work.numel() >= int(self.lib.tt_ga_unique_work_bytes(N, C, self.E))):
            raise ValueError("work must be a uint8 CUDA tensor of at least tt_ga_unique_work_bytes(N, C, E) bytes")
        c = child or {k: pop[k] for k in pop}
        _check(self.lib, self.lib.tt_ga_replace_unique(
            self.handle, pop["slot"].data_ptr(), pop["room"].data_ptr(), pop["hcv"].data_ptr(),
            pop["scv"].data_ptr(), pop["feasible"].data_ptr(), pop["penalty"].data_ptr(), N,
            c["slot"].data_ptr(), c["room"].data_ptr(), c["hcv"].data_ptr(), c["scv"].data_ptr(),
            c["feasible"].data_ptr(), c["penalty"].data_ptr(), C,
            ctypes.c_void_p(keep.data_ptr() if C else None), n_kept.data_ptr(), int(hash_bits), work.data_ptr(),
            self._stream(pop["slot"])))
        return keep, n_kept

    # -- greedy constructive initial population (include/ttga_greedy.h) ----------------
    def greedy_order(self):
        """tt_greedy_order: the events hardest first (int32 [E] CUDA tensor),
        computed on first use on torch's current stream and kept on the object."""
        import torch
        if getattr(self, "_greedy_order", None) is None:
            dev = torch.device("cuda", self.device)
            order = torch.empty(self.E, dtype=torch.int32, device=dev)
            work = torch.empty(int(self.lib.tt_greedy_work_bytes(self.handle)), dtype=torch.uint8, device=dev)
            _check(self.lib, self.lib.tt_greedy_order(self.handle, order.data_ptr(), work.data_ptr(),
                                                      self._stream(order)))
            self._greedy_order = order
            self._greedy_order_ev = torch.cuda.Event()
            self._greedy_order_ev.record(torch.cuda.current_stream(dev))
        else:
            # a later use may be on another stream than the one that computed it
            torch.cuda.current_stream(self._greedy_order.device).wait_event(self._greedy_order_ev)
        return self._greedy_order

    def greedy_init(self, rng, slot, room, order=None):
        """tt_greedy_init: the counterpart of random_init; `order` (int32 [E] CUDA
        tensor, a permutation of the events) defaults to greedy_order()."""
        import torch
        P = self._pop(slot, room)
        self._rng(rng, P)
        if order is None:
            order = self.greedy_order()
        elif not (order.is_cuda and order.dtype == torch.int32 and order.is_contiguous() and order.numel() == self.E
                  and order.device == slot.device):
            raise ValueError("order must be a contiguous int32 CUDA tensor of E entries on the population's device")
        _check(self.lib, self.lib.tt_greedy_init(self.handle, order.data_ptr(), rng.data_ptr(), slot.data_ptr(),
                                                 room.data_ptr(), P, self._stream(slot)))

    # -- Kempe-chain interchange (include/ttga_kempe.h) ------------------------------
    def kempe_move(self, slot, room, rng, prob, max_chain=0, chain_len=None):
        """tt_kempe_move in place on slot/room [P, E] with the streams rng [P]:
        with probability `prob` an individual moves the conflict component of
        one event between two timeslots (at most max_chain events; 0: no cap).
        chain_len: optional int32 [P] CUDA tensor (events moved, minus the
        component's size where the cap refused it, 0 where nothing was tried)."""
        P = self._pop(slot, room)
        self._rng(rng, P)
        _opt_i32("chain_len", chain_len, P, "P", slot.device)
        _check(self.lib, self.lib.tt_kempe_move(
            self.handle, slot.data_ptr(), room.data_ptr(), rng.data_ptr(), P, float(prob), int(max_chain),
            _ptr(chain_len), self._stream(slot)))

    # -- timeslot-swap descent (include/ttga_slotswap.h) ------------------------------
    def slot_swap(self, slot, max_passes, scv=None, penalty=None, gain=None, passes=None, perm=None):
        """tt_slot_swap in place on slot [P, E]: per row, the pair of timeslots
        whose exchange lowers scv most trades its events, at most max_passes
        times. scv, penalty (int32 [P], updated in place), gain, passes (int32
        [P]) and perm (uint8 [P, 45], new slot = perm[old slot]) are optional
        CUDA tensors."""
        import torch
        P = self._pop(slot)
        for name, t in (("scv", scv), ("penalty", penalty), ("gain", gain), ("passes", passes)):
            _opt_i32(name, t, P, "P", slot.device)
        if perm is not None and not (perm.is_cuda and perm.dtype == torch.uint8 and perm.is_contiguous()
                                     and tuple(perm.shape) == (P, NUM_SLOTS) and perm.device == slot.device):
            raise ValueError("perm must be a contiguous uint8 CUDA tensor of shape [P, 45] on the population's device")
        _check(self.lib, self.lib.tt_slot_swap(self.handle, slot.data_ptr(), P, int(max_passes), _ptr(scv),
                                               _ptr(penalty), _ptr(gain), _ptr(passes), _ptr(perm),
                                               self._stream(slot)))

    # -- late-acceptance search on feasible rows (include/ttga_lahc.h) -----------------
    def lahc(self, slot, room, rng, steps, history, p_swap=0.5, scv=None, penalty=None, gain=None, accepted=None,
             best_step=None):
        """tt_lahc in place on slot, room [P, E] and rng [P]: per feasible row, a
        walk of `steps` Move1 / Move2 candidates that keep hcv 0, accepted when
        no worse than the current row or the one `history` steps ago; the best
        row seen comes back. scv, penalty (int32 [P], updated in place), gain,
        accepted and best_step (int32 [P]) are optional CUDA tensors."""
        P = self._pop(slot, room)
        self._rng(rng, P)
        for name, t in (("scv", scv), ("penalty", penalty), ("gain", gain), ("accepted", accepted),
                        ("best_step", best_step)):
            _opt_i32(name, t, P, "P", slot.device)
        _check(self.lib, self.lib.tt_lahc(self.handle, slot.data_ptr(), room.data_ptr(), rng.data_ptr(), P, int(steps),
                                          int(history), float(p_swap), _ptr(scv), _ptr(penalty), _ptr(gain),
                                          _ptr(accepted), _ptr(best_step), self._stream(slot)))

    def lahc_kempe(self, slot, room, rng, steps, history, p_swap=0.25, p_kempe=0.5, max_chain=0, scv=None, penalty=None,
                   gain=None, accepted=None, best_step=None, kempe_stats=None):
        """tt_lahc_kempe in place on slot, room [P, E] and rng [P]: tt_lahc's walk
        in which a share p_kempe of the candidates is a Kempe chain between
        e1's slot and a second one, of at most max_chain events (0: no cap),
        with its rooms chosen directly; p_swap + p_kempe <= 1. The optional
        tensors are lahc()'s, and kempe_stats (int32 [P, 5]: chains tried,
        capped, without a room, accepted, and the events of the accepted ones)."""
        P = self._pop(slot, room)
        self._rng(rng, P)
        for name, t in (("scv", scv), ("penalty", penalty), ("gain", gain), ("accepted", accepted),
                        ("best_step", best_step)):
            _opt_i32(name, t, P, "P", slot.device)
        _opt_i32("kempe_stats", kempe_stats, 5 * P, "5 P" if P else "P", slot.device)
        _check(self.lib, self.lib.tt_lahc_kempe(self.handle, slot.data_ptr(), room.data_ptr(), rng.data_ptr(), P,
                                                int(steps), int(history), float(p_swap), float(p_kempe), int(max_chain),
                                                _ptr(scv), _ptr(penalty), _ptr(gain), _ptr(accepted), _ptr(best_step),
                                                _ptr(kempe_stats), self._stream(slot)))

    def lahc_kempe_aug(self, slot, room, rng, steps, history, p_swap=0.25, p_kempe=0.5, max_chain=0, room_rule=1,
                       scv=None, penalty=None, gain=None, accepted=None, best_step=None, kempe_stats=None):
        """tt_lahc_kempe_aug in place on slot, room [P, E] and rng [P]:
        lahc_kempe() with a room_rule (0: its direct rule; 1: a chain event with
        no free possible room moves the target slot's holders along an
        augmenting path). The optional tensors are lahc_kempe()'s, with
        kempe_stats int32 [P, 7]: its five counts, the chains a path rescued
        and the bystanders the accepted chains displaced."""
        P = self._pop(slot, room)
        self._rng(rng, P)
        for name, t in (("scv", scv), ("penalty", penalty), ("gain", gain), ("accepted", accepted),
                        ("best_step", best_step)):
            _opt_i32(name, t, P, "P", slot.device)
        _opt_i32("kempe_stats", kempe_stats, 7 * P, "7 P" if P else "P", slot.device)
        _check(self.lib, self.lib.tt_lahc_kempe_aug(self.handle, slot.data_ptr(), room.data_ptr(), rng.data_ptr(), P,
                                                    int(steps), int(history), float(p_swap), float(p_kempe),
                                                    int(max_chain), int(room_rule), _ptr(scv), _ptr(penalty),
                                                    _ptr(gain), _ptr(accepted), _ptr(best_step), _ptr(kempe_stats),
                                                    self._stream(slot)))

    # -- parallel walkers of the walk (include/ttga_lahc_multi.h) -----------------------
    def lahc_multi_work_bytes(self, P: int, walkers: int) -> int:
        """tt_lahc_multi_work_bytes: the bytes of lahc_multi()'s work tensor for
        P rows of `walkers` walkers; 0 for arguments the call refuses."""
        if not (0 <= int(P) < 2 ** 31 and -2 ** 31 <= int(walkers) < 2 ** 31):
            return 0
        return int(self.lib.tt_lahc_multi_work_bytes(self.handle, int(P), int(walkers)))

    def lahc_multi(self, slot, room, rng, walkers, steps, history, p_swap=0.25, p_kempe=0.5, max_chain=0, room_rule=1,
                   scv=None, penalty=None, gain=None, accepted=None, best_step=None, kempe_stats=None, winner=None,
                   walker_gain=None, work=None):
        """tt_lahc_multi in place on slot, room [P, E] and rng [P]: `walkers`
        walks of lahc_kempe_aug() from every feasible row, each on its own
        stretch of the row's stream; the best of them comes back and rng moves
        3 * steps * walkers draws on. The optional tensors are
        lahc_kempe_aug()'s (they describe the winner's walk), winner int32 [P]
        and walker_gain int32 [P, walkers]. work: a uint8 CUDA tensor of at
        least lahc_multi_work_bytes(P, walkers) bytes; it may be None with
        walkers == 1, and with more walkers None allocates one for the call."""
        import torch
        P = self._pop(slot, room)
        self._rng(rng, P)
        K = int(walkers)
        for name, t, n, what in (("scv", scv, P, "P"), ("penalty", penalty, P, "P"), ("gain", gain, P, "P"),
                                 ("accepted", accepted, P, "P"), ("best_step", best_step, P, "P"),
                                 ("kempe_stats", kempe_stats, 7 * P, "7 P"), ("winner", winner, P, "P"),
                                 ("walker_gain", walker_gain, max(K, 0) * P, "P * walkers")):
            _opt_i32(name, t, n, what, slot.device)
        if work is None and 1 < K <= MAX_WALKERS and P * K < 2 ** 31:
            work = torch.empty(self.lahc_multi_work_bytes(P, K), dtype=torch.uint8, device=slot.device)
        if work is not None:
            need = self.lahc_multi_work_bytes(P, K)
            if not (work.is_cuda and work.dtype == torch.uint8 and work.is_contiguous() and work.device == slot.device
                    and (work.numel() >= need or need == 0)):
                raise ValueError(f"work must be a contiguous uint8 CUDA tensor of at least {need} bytes "
                                 "on the population's device")
        _check(self.lib, self.lib.tt_lahc_multi(self.handle, slot.data_ptr(), room.data_ptr(), rng.data_ptr(), P, K,
                                                int(steps), int(history), float(p_swap), float(p_kempe),
                                                int(max_chain), int(room_rule), _ptr(scv), _ptr(penalty), _ptr(gain),
                                                _ptr(accepted), _ptr(best_step), _ptr(kempe_stats), _ptr(winner),
                                                _ptr(walker_gain), _ptr(work), self._stream(slot)))

    # -- conflict-guided crossover (include/ttga_cx.h) -------------------------------
    def _cx_args(self, slot, order, P, cost, repaired):
        _opt_i32("order", order, self.E, "E", slot.device)
        for name, t in (("cost", cost), ("repaired", repaired)):
            _opt_i32(name, t, P, "P", slot.device)
        return self.greedy_order() if order is None else order

    def crossover_guided(self, slot1, slot2, rng, slot, room, order=None, repair=False, cost=None, repaired=None):
        """tt_crossover_guided: the counterpart of crossover; every event, in
        `order` (int32 [E] CUDA tensor, default greedy_order()), takes the
        parent's slot that clashes less with what the child holds already, the
        coin between equals; with `repair` an event that clashes in both goes to
        a slot of least cost. cost, repaired: optional int32 [P] CUDA tensors."""
        P = self._pop(slot, room)
        if self._pop(slot1, slot2) != P or slot2.shape[0] != P:
            raise ValueError("the parents' tensors must have the children's shape [P, E]")
        self._rng(rng, P)
        order = self._cx_args(slot, order, P, cost, repaired)
        _check(self.lib, self.lib.tt_crossover_guided(self.handle, slot1.data_ptr(), slot2.data_ptr(),
                                                      order.data_ptr(), rng.data_ptr(), slot.data_ptr(),
                                                      room.data_ptr(), P, int(bool(repair)), _ptr(cost), _ptr(repaired),
                                                      self._stream(slot)))

    def ga_breed_guided(self, pop_slot, pop_room, pop_penalty, rng, child_slot, child_room, child_flags,
                        p_cross=0.8, p_mut=0.5, skip_init_draws=True, order=None, repair=False, cost=None,
                        repaired=None):
        """tt_ga_breed_guided: ga_breed with the guided crossover (order, repair,
        cost and repaired as in crossover_guided, over the C children)."""
        N = self._pop(pop_slot, pop_room)
        C = self._pop(child_slot, child_room)
        self._rng(rng, C)
        order = self._cx_args(child_slot, order, C, cost, repaired)
        _check(self.lib, self.lib.tt_ga_breed_guided(
            self.handle, pop_slot.data_ptr(), pop_room.data_ptr(), pop_penalty.data_ptr(), N, order.data_ptr(),
            rng.data_ptr(), C, float(p_cross), float(p_mut), int(bool(skip_init_draws)), int(bool(repair)),
            child_slot.data_ptr(), child_room.data_ptr(), child_flags.data_ptr(), _ptr(cost), _ptr(repaired),
            self._stream(pop_slot)))

    # -- the single-event neighbourhood (include/ttga/move1.h) ---------------------------
    def move1_scan(self, slot, room, summary=None, d_scv=None, to_room=None, stream=None):
        """tt_move1_scan on slot, room [P, E], which it only reads: per feasible
        row, for every event e and slot t, d_scv (int32 [P, E, 45]: the change
        of scv when e goes to t) and to_room (uint8 [P, E, 45]: the room it
        would take, or MOVE1_CLASH / MOVE1_NO_ROOM), and summary (int32 [P, 6]:
        scanned, feasible moves, improving ones, the least d_scv among them,
        its event, its slot). All three are optional CUDA tensors. stream: a
        torch.cuda.Stream (default: torch's current stream)."""
        import torch
        P = self._pop(slot, room)
        cells = P * self.E * NUM_SLOTS
        _opt_i32("summary", summary, 6 * P, "6 P", slot.device)
        _opt_i32("d_scv", d_scv, cells, "P * E * 45", slot.device)
        if to_room is not None and not (to_room.is_cuda and to_room.dtype == torch.uint8 and to_room.is_contiguous()
                                        and to_room.numel() == cells and to_room.device == slot.device):
            raise ValueError("to_room must be a contiguous uint8 CUDA tensor of P * E * 45 entries on the "
                             "population's device")
        _check(self.lib, self.lib.tt_move1_scan(self.handle, slot.data_ptr(), room.data_ptr(), P, _ptr(summary),
                                                _ptr(d_scv), _ptr(to_room), self._stream(slot, stream)))

    def move1_descent(self, slot, room, max_passes, scv=None, penalty=None, gain=None, passes=None, stream=None):
        """tt_move1_descent in place on slot, room [P, E]: per feasible row, the
        feasible single-event move of least d_scv is applied while it lowers
        scv, at most max_passes times. scv, penalty (int32 [P], updated in
        place), gain and passes (int32 [P]) are optional CUDA tensors."""
        P = self._pop(slot, room)
        for name, t in (("scv", scv), ("penalty", penalty), ("gain", gain), ("passes", passes)):
            _opt_i32(name, t, P, "P", slot.device)
        _check(self.lib, self.lib.tt_move1_descent(self.handle, slot.data_ptr(), room.data_ptr(), P, int(max_passes),
                                                   _ptr(scv), _ptr(penalty), _ptr(gain), _ptr(passes),
                                                   self._stream(slot, stream)))

    @staticmethod
    def _rng(rng, P):
        import torch
        if not (rng.is_cuda and rng.dtype == torch.int64 and rng.is_contiguous() and rng.numel() == P):
            raise ValueError("rng must be a contiguous int64 CUDA tensor with one state per individual")
