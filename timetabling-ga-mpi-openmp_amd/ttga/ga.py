"""The GA of ga.cpp on the device: one island per GPU, batched generations.

Mirrors ga.cpp:370-613 with the per-child operators running as batched
kernels (include/ttga.h):

* initial population: RandomInitialSolution + localSearch(maxSteps) +
  computePenalty per member (ga.cpp:429-434), then sorted;
* a generation breeds C children from the current population
  (tt_ga_breed: selection5 x2, crossover p=0.8 / copy, mutation p=0.5),
  runs localSearch + evaluation on all of them, and replaces the C worst
  members, re-sorting by penalty (tt_ga_replace). C = 1 is the reference's
  single-thread steady state; C > 1 is the batched counterpart of its
  OpenMP threads (every thread breeding against the shared population);
* optionally (Island(unique=True)) a child whose genome is already in the
  population, or in an earlier child of its sub-batch, is dropped instead of
  replacing a member (tt_ga_replace_unique): an addition, ga.cpp has no
  such test. Migration is unchanged: a migrant may duplicate a member of its
  destination;
* optionally (Island(slot_swap=N)) every searched row goes through the
  timeslot-swap descent (tt_slot_swap) before it is sorted in: an addition
  too, which changes scv only;
* optionally (Island(lahc=N)) every searched row that is feasible then walks N
  late-acceptance steps over feasible rows (tt_lahc) and comes back as the best
  row of the walk: an addition too, which lowers scv only;
* optionally (Island(move1_descent=N)) every searched row that is feasible then
  takes at most N steps of steepest descent over its single-event moves
  (tt_move1_descent): an addition too, which lowers scv only;
* optionally (Island(crossover="guided")) the children are bred with the
  conflict-guided crossover (tt_ga_breed_guided) in place of the reference's
  uniform one: an addition too, which changes only how a crossed child's
  timeslots are chosen between its parents';
* migration (ga.cpp:514-540) and the final MIN reduction (ga.cpp:234-257) are
  in ttga.islands.

Each population member and each child slot owns a Park-Miller stream
(the reference shares one unlocked stream between threads).
Stream k of an island with seed s starts at Random(|s| + 1 + k).
"""
from __future__ import annotations

import contextlib
import json
import math
import time
import types

import numpy as np

from .stages import validate

# ga.cpp:389-397: -p 1 -> 200, -p 2 -> 1000, otherwise 2000
MAX_STEPS = {1: 200, 2: 1000}


def max_steps_for(problem_type: int) -> int:
    return MAX_STEPS.get(int(problem_type), 2000)


def _fmt(v):
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    if isinstance(v, float):
        if math.isnan(v):
            return "null"
        if math.isinf(v):
            return "1e+9999" if v > 0 else "-1e+9999"
        return "%.17g" % v
    if isinstance(v, dict):
        return "{" + ",".join(json.dumps(k) + ":" + _fmt(v[k]) for k in sorted(v)) + "}"
    if isinstance(v, (list, tuple, np.ndarray)):
        return "[" + ",".join(_fmt(x) for x in v) + "]"
    return json.dumps(v)


def json_line(obj) -> str:
    """jsoncpp StreamWriterBuilder with indentation "" (ga.cpp:171): compact,
    keys sorted (std::map, json/json.h:584), doubles as %.17g (jsoncpp.cpp:4049)."""
    return _fmt(obj)


def stream_seeds(seed: int, first: int, n: int) -> np.ndarray:
    return (np.arange(first, first + n, dtype=np.int64) + np.int64(abs(int(seed)) + 1)).astype(np.int64)


def pack_member(pop: dict, k: int):
    """serializeSolutions(k, 1, ...) (ga.cpp:318-335): one migrant as a flat
    uint8 tensor on the population's device: slot[E], room[E], then int32
    hcv, scv, feasible, penalty."""
    import torch
    meta = torch.stack([pop["hcv"][k], pop["scv"][k], pop["feasible"][k].to(torch.int32), pop["penalty"][k]])
    return torch.cat([pop["slot"][k], pop["room"][k], meta.view(torch.uint8)])


def unpack_member(pop: dict, pos: int, buf) -> None:
    """deserializeSolution(offset, 1, ...) into position `pos` (ga.cpp:344-368).
    `buf` may live on another device (a host-staged payload)."""
    import torch
    E = pop["slot"].shape[1]
    buf = buf.to(pop["slot"].device)
    pop["slot"][pos].copy_(buf[:E])
    pop["room"][pos].copy_(buf[E:2 * E])
    meta = buf[2 * E:2 * E + 16].clone().view(torch.int32)
    pop["hcv"][pos] = meta[0]
    pop["scv"][pos] = meta[1]
    pop["feasible"][pos] = meta[2].to(torch.uint8)
    pop["penalty"][pos] = meta[3]


def new_population(n: int, E: int, device):
    import torch
    return {"slot": torch.zeros((n, E), dtype=torch.uint8, device=device),
            "room": torch.zeros((n, E), dtype=torch.uint8, device=device),
            "hcv": torch.zeros(n, dtype=torch.int32, device=device),
            "scv": torch.zeros(n, dtype=torch.int32, device=device),
            "feasible": torch.zeros(n, dtype=torch.uint8, device=device),
            "penalty": torch.zeros(n, dtype=torch.int32, device=device)}


class Members:
    """A population [N] of (slot, room, hcv, scv, feasible, penalty) tensors
    and the migration interface of ga.cpp (pack / unpack_into). Island adds
    the device GA on top; the class itself works on any torch device, which
    is what the CPU (gloo) tests of the ring use."""

    min_pop = 3     # ring migration writes pop[N-1] and pop[N-2] and reads pop[0], pop[1]

    def __init__(self, pop: dict):
        self.pop = pop
        self.N = int(pop["slot"].shape[0])

    def pack(self, k: int):
        return pack_member(self.pop, k)

    def unpack_into(self, pos: int, buf) -> None:
        unpack_member(self.pop, pos, buf)

    def copy_from(self, other: "Members") -> None:
        for k, t in self.pop.items():
            t.copy_(other.pop[k].to(t.device))

    def member(self, k: int) -> dict:
        """deserialised Solution fields of member k (ga.cpp:318-335 payload)."""
        p = self.pop
        return {"slot": p["slot"][k].cpu().numpy(), "room": p["room"][k].cpu().numpy(),
                "feasible": bool(p["feasible"][k].item()), "scv": int(p["scv"][k].item()),
                "hcv": int(p["hcv"][k].item()), "penalty": int(p["penalty"][k].item())}

    def member_meta(self, k: int):
        p = self.pop
        return (bool(p["feasible"][k].item()), int(p["scv"][k].item()), int(p["hcv"][k].item()),
                int(p["penalty"][k].item()))

    def best_value(self) -> tuple[bool, int]:
        """(feasible, scv) if feasible else (False, hcv*1e6 + scv) (ga.cpp:191,218,247)."""
        b = self.member_meta(0)
        return (True, b[1]) if b[0] else (False, b[2] * 1000000 + b[1])


_SIDE_STREAMS: dict = {}
_NO_STREAM = contextlib.nullcontext()     # work on torch's current stream


def _side_streams(dev, base, n: int) -> list:
    """n streams for a staggered island's parts 1..n, cached per (device, base
    stream): islands built one after another on the same base stream reuse the
    same side streams. (A process gets a few hardware queues, GPU_MAX_HW_QUEUES,
    and HIP maps streams onto them as they are created: fresh streams per
    island can land on the queue of the base stream and serialise the parts.)"""
    import torch
    key = (dev.index, None if base is None else base.cuda_stream)
    pool = _SIDE_STREAMS.setdefault(key, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(dev))
    return pool[:n]


# The stages whose per-row outputs are tallied on the device: what turns the stage on (for
# {stage}_stats()'s error), the name of its row count, its int32 per-row outputs, the names
# of its sums, and whether it also runs on the members in initialize()
_TALLIED = {
    "kempe": ("kempe > 0", "children", ("chain",), ("moved", "rejected", "chain_events"), False),
    "slot_swap": ("slot_swap > 0", "rows", ("gain", "passes"), ("improved", "passes", "gain"), True),
    "lahc": ("lahc > 0", "rows", ("gain", "accepted", "best_step"), ("searched", "improved", "accepted", "gain"), True),
    "lahc_kempe": ("lahc_kempe > 0", "rows", ("stats",), ("tried", "capped", "no_room", "accepted", "chain_events"),
                   True),
    "lahc_walkers": ("lahc_walkers > 1", None, ("winner", "walker_gain"), ("rows", "gain", "gainFirst", "winnerLater"),
                     True),
    "cx": ("crossover='guided'", "children", ("cost", "repaired"), ("crossed", "clean", "cost", "repaired"), False),
    "move1_descent": ("move1_descent > 0", "rows", ("gain", "passes"), ("improved", "passes", "gain"), True),
}


class Tally:
    """A stage's device-side tally for calls on n rows: its int32 per-row
    outputs `out[name]`, the int64 running `sums` (one entry per name), added
    up on the stream behind each call, and on the host the `rows` it was called
    on. The tensors join `register` (Island's record_stream pass)."""

    def __init__(self, n: int, outputs, sums, dev, register: list, walkers: int = 1):
        import torch
        # the outputs with more than one entry a row (tt_lahc_multi writes seven counts whatever the room rule)
        wide = {"stats": 7 if walkers > 1 else len(sums), "walker_gain": walkers}
        self.out = {k: torch.zeros((n, wide[k]) if k in wide else n, dtype=torch.int32, device=dev)
                    for k in outputs}
        self.sums = torch.zeros(len(sums), dtype=torch.int64, device=dev)
        self.rows = 0
        register += [*self.out.values(), self.sums]

    def add(self, rows: int, *scalars) -> None:
        """The device scalars of one call on `rows` rows, in the sums' order."""
        import torch
        self.sums += torch.stack(scalars)
        self.rows += rows


class Island(Members):
    """One island: population [N] + C child slots, all device-resident.

    The child slots are split into `parts` sub-batches (part j: child slots
    [j*C/parts, ...) rounded as numpy.array_split) on as many streams, and
    sub-batch h is bred from the population after the replacement of sub-batch
    h - parts, so sub-batch h's local search runs while the searches of
    h - parts + 1 .. h - 1 finish. The population operations are totally
    ordered -- breed(h) after replace(h - parts), replace(h - parts + 1) after
    breed(h) -- so results are deterministic, and C children are in flight at
    every breed, as with ga.cpp:488-588's C threads breeding from the shared
    population while the other threads' children are still searched. step()
    advances `parts` sub-batches and leaves parts - 1 of them pending; flush()
    replaces them (every host read of the population flushes first; the
    snapshots the drivers log from do not).

    schedule "batch" is the pipeline with one part: all C children, on the
    island's stream (None: torch's current stream at each call), with
    self.work; a generation breeds them, searches them in one launch and
    replaces the C worst (sub-batch h - parts + 1 is h itself), nothing stays
    pending, and no other stream or event exists. schedule "staggered" is
    `parts` >= 2: the parts run on streams of their own even when the island's
    stream is None; initialize(), step() and flush() order their population
    operations after the caller's work on its stream (the island's, else
    torch's current stream) and make that stream wait for the last of them, so
    the caller's next reads and writes of the population are ordered as on a
    one-part island.

    init="greedy": initialize() builds the members with tt_greedy_init
    (include/ttga_greedy.h) instead of tt_random_init; the local search, the
    sort and everything after it are the same, and so are breeding (its
    skip_init_draws included) and migration.

    unique=True: every replacement is tt_ga_replace_unique (include/ttga_unique.h):
    a child whose genome (slot row + room row) equals a member's or an earlier
    child's of the same sub-batch is dropped, decided on the device with no
    host synchronisation; the D kept children replace the D worst members. A
    population whose genomes are pairwise distinct stays so, migrants aside:
    migration is unchanged and a migrant may duplicate a member of its
    destination. unique_stats() reports the children bred and dropped.

    kempe=p > 0: every sub-batch's children get tt_kempe_move
    (include/ttga_kempe.h) with probability p, at most kempe_max_chain events
    a chain (0: no cap), on the sub-batch's stream directly after tt_ga_breed
    and before the search, drawing from the children's own streams. kempe=0
    issues no call at all. kempe_stats() reports what the moves did.

    slot_swap=n >= 1: tt_slot_swap(max_passes=n) (include/ttga_slotswap.h) runs
    on the part's stream directly behind every tt_local_search_eval -- on the
    children of a sub-batch before it joins the pending ones, on the members in
    initialize() before the sort -- and lowers their scv and penalty tensors
    in place, so the replacement sorts on the true penalties with no second
    evaluation. It draws no random numbers. slot_swap=0 issues no call at all.
    slot_swap_stats() reports what the descents did.

    lahc=n >= 1: tt_lahc(steps=n, history=lahc_history, p_swap=lahc_swap)
    (include/ttga_lahc.h) runs on the part's stream directly behind every
    tt_local_search_eval, and behind tt_slot_swap when that is on -- on the
    children of a sub-batch, drawing from the children's own streams, and on
    the members in initialize() before the sort, drawing from rng_init. Only
    rows that are feasible walk; their scv and penalty tensors are lowered in
    place. lahc=0 issues no call at all. lahc_stats() reports what the walks did.

    lahc_kempe=p > 0 (needs lahc >= 1 and lahc_swap + p <= 1): the walk is
    tt_lahc_kempe (include/ttga_lahc_kempe.h) in place of tt_lahc, at the same
    places and with the same arguments: a share p of its candidates is a Kempe
    chain between the event's slot and a second one, of at most
    lahc_kempe_max_chain events (0: no cap). lahc_stats() counts all three
    kinds of move; lahc_kempe_stats() reports the chains. lahc_kempe=0 calls
    tt_lahc exactly as before.

    lahc_kempe_rooms="augment" (needs lahc_kempe > 0): the walk is
    tt_lahc_kempe_aug (include/ttga_lahc_kempe_aug.h) with room_rule 1 in place
    of tt_lahc_kempe: a chain event with no free possible room moves the target
    slot's holders along an augmenting path. lahc_kempe_stats() then also has
    `rescued` and `displaced`. "direct" calls what the island called before.

    lahc_walkers=K > 1 (needs lahc > 0): the walk is tt_lahc_multi
    (include/ttga_lahc_multi.h) with the island's walk arguments: K walks from
    every searched row, each on its own stretch of the row's stream, and the
    best of them comes back. lahc_stats() and lahc_kempe_stats() then describe
    the winners' walks, and lahc_walkers_stats() compares the winners with
    walker 0, which is the single walk. lahc_walkers=1 issues exactly the calls
    the island issued before.

    crossover="guided": every sub-batch is bred with tt_ga_breed_guided
    (include/ttga_cx.h) in place of tt_ga_breed, on the same stream and at the
    same place in the operation chain, in the handle's greedy_order(); with
    crossover_repair an event that clashes in both parents' slots goes to a
    slot of least cost. Everything else is unchanged. crossover="uniform"
    issues no new call at all. cx_stats() reports what the crossovers did.

    move1_descent=n >= 1: tt_move1_descent(max_passes=n) (include/ttga/move1.h)
    runs on the part's stream directly behind every tt_local_search_eval, and
    behind tt_slot_swap and the walk where those are on -- on the children of
    a sub-batch, on the members in initialize() before the sort. Only rows that
    are feasible descend: the feasible single-event move that lowers scv most
    is applied, at most n times, and their scv and penalty tensors are lowered
    in place. It draws no random numbers. move1_descent=0 issues no call at
    all. move1_descent_stats() reports what the descents did.

    `on` is the set of these stages that are on: "unique", "kempe",
    "slot_swap", "lahc", "lahc_kempe", "cx", "move1_descent" (the
    {stage}_stats() that do not raise).
    """

    def __init__(self, dp, pop_size: int = 10, children: int = 1, max_steps: int = 200, seed: int = 1,
                 p_cross: float = 0.8, p_mut: float = 0.5, skip_init_draws: bool = True, device=None,
                 p1: float = 1.0, p2: float = 1.0, p3: float = 0.0, lpt: bool | None = None, stream=None,
                 schedule: str = "batch", parts: int = 2, unique: bool = False, init: str = "random",
                 kempe: float = 0.0, kempe_max_chain: int = 0, slot_swap: int = 0,
                 lahc: int = 0, lahc_history: int = 500, lahc_swap: float = 0.5,
                 crossover: str = "uniform", crossover_repair: bool = False,
                 lahc_kempe: float = 0.0, lahc_kempe_max_chain: int = 0, lahc_kempe_rooms: str = "direct",
                 lahc_walkers: int = 1, move1_descent: int = 0):
        """stream: a torch.cuda.Stream of the island's own, or None (torch's current
        stream). Islands multiplexed on one GPU (ttga.islands --islands K) each take
        one, so one island's launches fill the SIMD slots another's local-search tail
        leaves idle; every host read of the island (member, member_meta, best_thread)
        synchronises its stream first, and a caller that moves data between islands
        (migration) synchronises the device around it."""
        validate(init, kempe, kempe_max_chain, slot_swap, lahc, lahc_history, lahc_swap, crossover, crossover_repair,
                 lahc_kempe, lahc_kempe_max_chain, lahc_kempe_rooms, lahc_walkers, move1_descent)
        import torch
        if not (1 <= children <= pop_size):
            raise ValueError("need 1 <= children <= pop_size")
        if schedule not in ("batch", "staggered"):
            raise ValueError("schedule must be 'batch' or 'staggered'")
        if schedule == "staggered" and not (2 <= parts <= children):
            raise ValueError("the staggered schedule needs 2 <= parts <= children")
        dev = torch.device("cuda", dp.device if device is None else device)
        super().__init__(new_population(int(pop_size), dp.E, dev))
        self.dp, self.C = dp, int(children)
        self.max_steps, self.seed = int(max_steps), int(seed)
        self.p_cross, self.p_mut, self.skip = float(p_cross), float(p_mut), bool(skip_init_draws)
        self.p1, self.p2, self.p3 = float(p1), float(p2), float(p3)   # LS move probabilities (Solution.h:61)
        # longest-expected-first dispatch of the children's local search (only the
        # launch order changes); by default for generations of >= 4096 children
        self.lpt = (int(children) >= 4096) if lpt is None else bool(lpt)
        self.child = new_population(self.C, dp.E, dev)
        self.flags = torch.zeros(self.C, dtype=torch.uint8, device=dev)
        self.rng_init = torch.from_numpy(stream_seeds(seed, 0, self.N)).to(dev)
        self.rng_child = torch.from_numpy(stream_seeds(seed, self.N, self.C)).to(dev)
        self.unique = bool(unique)
        self.init = init
        self.kempe, self.kempe_max_chain = float(kempe), int(kempe_max_chain)
        self.slot_swap = int(slot_swap)
        self.lahc, self.lahc_history, self.lahc_swap = int(lahc), int(lahc_history), float(lahc_swap)
        self.lahc_kempe, self.lahc_kempe_max_chain = float(lahc_kempe), int(lahc_kempe_max_chain)
        self.lahc_kempe_rooms = lahc_kempe_rooms
        self.lahc_walkers = int(lahc_walkers)
        self.move1_descent = int(move1_descent)
        self.crossover, self.crossover_repair = crossover, bool(crossover_repair)
        self.generation = 0
        self.schedule = schedule
        self.parts = int(parts) if schedule == "staggered" else 1
        self._user_stream = stream                    # None: torch's current stream at each call
        if self.parts > 1 and stream is None:
            # every part on a stream of its own, the first included: work on the legacy
            # null stream orders itself against the other streams' work, which would
            # serialise the parts (profiles/r06_n_trace_overlap_comp20_staggered.json)
            stream = _side_streams(dev, None, 1)[0]
        self.stream = stream
        # part j: child rows [off, off + n) as views of the child, rng_child and flags tensors,
        # a work buffer and a stream; part 0 runs on the island's stream with self.work, the
        # others on streams and buffers of their own
        bounds = [0] + [int(b) for b in np.cumsum([len(x) for x in np.array_split(np.arange(self.C), self.parts)])]
        streams = [stream] + _side_streams(dev, stream, self.parts - 1)
        self._parts = []
        for j, st in enumerate(streams):
            r = slice(bounds[j], bounds[j + 1])
            n = r.stop - r.start
            self._parts.append(types.SimpleNamespace(
                off=r.start, n=n, child={k: v[r] for k, v in self.child.items()}, rng=self.rng_child[r],
                flags=self.flags[r], work=dp.ga_unique_work(self.N, n) if self.unique else dp.ga_work(self.N),
                stream=st, tally={}))
        self.work = self._parts[0].work
        # unique: each part's keep flags and kept count, the children dropped so far (added up
        # on the replacing stream) and, on the host, the children that went through a replacement
        self._extra = []
        if self.unique:
            for p in self._parts:
                p.keep = torch.zeros(p.n, dtype=torch.uint8, device=dev)
                p.n_kept = torch.zeros(1, dtype=torch.int32, device=dev)
                self._extra += [p.keep, p.n_kept]
            self._init_kept = torch.zeros(1, dtype=torch.int32, device=dev)
            self._dropped = torch.zeros(1, dtype=torch.int64, device=dev)
            self._extra += [self._init_kept, self._dropped]
        # the stages that are on, and their tallies: one per part, and the members' where the
        # stage also runs in initialize()
        self.on = {stage for stage, on in (("unique", self.unique), ("kempe", self.kempe > 0),
                                           ("slot_swap", self.slot_swap > 0), ("lahc", self.lahc > 0),
                                           ("lahc_kempe", self.lahc_kempe > 0),
                                           ("lahc_walkers", self.lahc_walkers > 1),
                                           ("cx", self.crossover == "guided"),
                                           ("move1_descent", self.move1_descent > 0)) if on}
        self._init_tally = {}
        for stage, (_, _, outputs, _, in_init) in _TALLIED.items():
            if stage in self.on:
                sums = self._sum_names(stage)
                if in_init:
                    self._init_tally[stage] = Tally(self.N, outputs, sums, dev, self._extra, self.lahc_walkers)
                for p in self._parts:
                    p.tally[stage] = Tally(p.n, outputs, sums, dev, self._extra, self.lahc_walkers)
        # tt_lahc_multi's work buffers, allocated once: one per part (the parts run on streams
        # of their own), the first of them large enough for the members too, whose walk runs
        # on the first part's stream
        if "lahc_walkers" in self.on:
            for j, p in enumerate(self._parts):
                rows = max(p.n, self.N) if j == 0 else p.n
                p.tally["lahc_walkers"].work = torch.empty(dp.lahc_multi_work_bytes(rows, self.lahc_walkers),
                                                           dtype=torch.uint8, device=dev)
                self._extra.append(p.tally["lahc_walkers"].work)
            self._init_tally["lahc_walkers"].work = self._parts[0].tally["lahc_walkers"].work
        self._replaced = 0
        self._pending = []                            # parts searched but not yet replaced, in breed order
        self._last_replace = 0                        # part whose work buffer holds the last replace's source
        # the last population operation (breed or replace): the stream it ran on, and (several
        # parts) the event recorded behind it, which the next one waits for on another stream
        self._op_stream = stream
        self._ev_op = torch.cuda.Event() if self.parts > 1 else None
        self._snap = None
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream(dev))     # the zero-filled buffers above
        for st in streams[1:]:
            st.wait_stream(stream)
        # the buffers were allocated on the creating stream and are used on the island's
        # own stream(s): tell the caching allocator, so a dropped island's blocks are not
        # handed out again while its kernels may still write them
        self._own_streams = [st for st in streams if st is not None]
        self._record_streams(list(self.pop.values()) + list(self.child.values())
                             + [self.flags, self.rng_init, self.rng_child] + [p.work for p in self._parts]
                             + self._extra)

    def _record_streams(self, tensors):
        for st in self._own_streams:
            for t in tensors:
                t.record_stream(st)

    def close(self):
        """Wait for everything the island has enqueued (its buffers can then be
        freed safely whatever the allocator knows)."""
        import torch
        self.flush()
        for st in self._own_streams:
            st.synchronize()
        torch.cuda.current_stream(self.pop["slot"].device).synchronize()

    # Cross-stream ordering, all of it: _wait_op / _record_op chain the population
    # operations, _fork / _join tie the chain to the caller's stream. Each does nothing
    # when the stream it would order is the one the last operation ran on, which on a
    # one-part island is every time (its only stream is the caller's).

    def _wait_op(self, st):
        """What `st` runs next comes after the last population operation."""
        if st is not self._op_stream:
            st.wait_event(self._ev_op)

    def _record_op(self, st):
        """A population operation (breed, replace, or the caller's writes taken
        in by _fork) has just been enqueued on `st`."""
        self._op_stream = st
        if self._ev_op is not None:
            self._ev_op.record(st)

    def _base(self):
        """The stream the caller orders its own work on: the island's stream as
        given, else torch's current stream (part 0's own stream when that is
        where the caller's work runs too: nothing to look up)."""
        import torch
        return self.stream if self.stream is self._user_stream else torch.cuda.current_stream(self.pop["slot"].device)

    def _fork(self):
        """The population operations enqueued next come after the caller's work
        enqueued so far on _base() (the chain takes it in on part 0's stream)."""
        b = self._base()
        if b is not self.stream:
            self.stream.wait_stream(b)
        self._wait_op(self.stream)
        self._record_op(self.stream)

    def _join(self):
        """The caller's stream (_base()) waits for the population's last
        operation, so what it enqueues next sees the population as a one-part
        island on that stream would leave it (pending sub-batches aside)."""
        self._wait_op(self._base())

    def _on_stream(self, stream=None):
        import torch
        st = self.stream if stream is None else stream
        return torch.cuda.stream(st) if st is not None else _NO_STREAM

    def sync(self):
        """Wait for the island's work: pending sub-batches are replaced first,
        then the island's stream is waited for."""
        self.flush()
        if self.stream is not None:
            self.stream.synchronize()

    def member(self, k: int) -> dict:
        self.sync()
        return super().member(k)

    def member_meta(self, k: int):
        self.sync()
        return super().member_meta(k)

    def report(self) -> dict:
        """ttga.report.population_report of the island's population, on the
        island's stream, with every pending sub-batch replaced first."""
        from .report import population_report
        self.flush()
        with self._on_stream():
            return population_report(self.dp, self.pop)

    def _evaluate(self, p):
        self.dp.eval(p["slot"], p["room"], out=(p["hcv"], p["scv"], p["feasible"], p["penalty"]))

    def initialize(self):
        """ga.cpp:429-434 for every member, then the population is sorted; with
        init "greedy" the members start from tt_greedy_init instead of
        RandomInitialSolution (ga.cpp:431)."""
        self._fork()
        with self._on_stream():
            p = self.pop
            if self.init == "greedy":
                self.dp.greedy_init(self.rng_init, p["slot"], p["room"])
            else:
                self.dp.random_init(self.rng_init, p["slot"], p["room"])
            self.dp.local_search(p["slot"], p["room"], self.rng_init, self.max_steps, self.p1, self.p2, self.p3,
                                 out=(p["hcv"], p["scv"], p["feasible"], p["penalty"]))
            if self.slot_swap > 0:
                self._slot_swap(p, self._init_tally["slot_swap"])
            if self.lahc > 0:
                self._lahc(p, self.rng_init, self._init_tally)
            if self.move1_descent > 0:
                self._move1_descent(p, self._init_tally["move1_descent"])
            if self.unique:
                self.dp.ga_replace_unique(p, None, self.work, n_kept=self._init_kept)
            else:
                self.dp.ga_replace(p, None, self.work)
        self._record_op(self.stream)
        self._join()

    def step(self):
        """One generation of C children (ga.cpp:543-585), enqueued on the island's
        stream(s): each sub-batch in turn."""
        self._fork()
        for j in range(self.parts):
            self._advance(j)
        self._join()
        self.generation += 1

    def _search(self, c, rng, work):
        """LPT order (optional), localSearch and evaluation of children c (one
        launch: tt_local_search_eval, ga.cpp:574-575)."""
        order = None
        if self.lpt:
            # dispatch the children longest-expected first (hcv before the search,
            # descending): the launch's tail is its slowest waves; results unchanged
            self._evaluate(c)
            order = self.dp.lpt_order(c["hcv"], work)
        self.dp.local_search(c["slot"], c["room"], rng, self.max_steps, self.p1, self.p2, self.p3, order=order,
                             out=(c["hcv"], c["scv"], c["feasible"], c["penalty"]))

    def _advance(self, j: int):
        """Sub-batch j: bred from the population behind the last population
        operation; then, with parts - 1 older sub-batches pending, the oldest of
        them is replaced behind that breed; then sub-batch j is searched (one
        part: and replaced at once, the sub-batch parts - 1 behind being itself)."""
        p = self._parts[j]
        with self._on_stream(p.stream):
            self._wait_op(p.stream)                                         # breed(h) after replace(h - parts)
            if self.crossover == "guided":
                self._breed_guided(p)
            else:
                self.dp.ga_breed(self.pop["slot"], self.pop["room"], self.pop["penalty"], p.rng, p.child["slot"],
                                 p.child["room"], p.flags, self.p_cross, self.p_mut, self.skip)
            self._record_op(p.stream)
            if self._pending and len(self._pending) >= self.parts - 1:
                self._replace_oldest()                                      # replace(h - parts + 1) after breed(h)
            if self.kempe > 0:
                self._kempe(p)
            self._search(p.child, p.rng, p.work)
            if self.slot_swap > 0:
                self._slot_swap(p.child, p.tally["slot_swap"])
            if self.lahc > 0:
                self._lahc(p.child, p.rng, p.tally)
            if self.move1_descent > 0:
                self._move1_descent(p.child, p.tally["move1_descent"])
            self._pending.append(j)
            if len(self._pending) >= self.parts:
                self._replace_oldest()

    def _breed_guided(self, p):
        """tt_ga_breed_guided for part p (on its stream, the current one) and
        its counts, summed on the device behind the breed."""
        t = p.tally["cx"]
        cost, repaired = t.out["cost"], t.out["repaired"]
        self.dp.ga_breed_guided(self.pop["slot"], self.pop["room"], self.pop["penalty"], p.rng, p.child["slot"],
                                p.child["room"], p.flags, self.p_cross, self.p_mut, self.skip,
                                repair=self.crossover_repair, cost=cost, repaired=repaired)
        crossed = (p.flags & 1) != 0
        t.add(p.n, crossed.sum(), (crossed & (cost == 0)).sum(), cost.sum(), repaired.sum())

    def _kempe(self, p):
        """tt_kempe_move on the children of part p (on its stream, the current
        one) and its counts, summed on the device behind the move."""
        t = p.tally["kempe"]
        chain = t.out["chain"]
        self.dp.kempe_move(p.child["slot"], p.child["room"], p.rng, self.kempe, self.kempe_max_chain, chain)
        t.add(p.n, (chain > 0).sum(), (chain < 0).sum(), chain.clamp(min=0).sum())

    def _slot_swap(self, rows, t):
        """tt_slot_swap on the searched rows (on the current stream, behind
        their search and evaluation) and its counts, summed on the device
        behind the call."""
        self._descent(t, rows, lambda **out: self.dp.slot_swap(rows["slot"], self.slot_swap, **out))

    @staticmethod
    def _descent(t, rows, call):
        """A descent that credits scv and penalty in place and reports gain and
        passes a row: call(scv=, penalty=, gain=, passes=), then the tally's
        rows, rows improved, passes and gain."""
        gain, passes = t.out["gain"], t.out["passes"]
        call(scv=rows["scv"], penalty=rows["penalty"], gain=gain, passes=passes)
        t.add(int(rows["slot"].shape[0]), (passes > 0).sum(), passes.sum(), gain.sum())

    def _move1_descent(self, rows, t):
        """tt_move1_descent on the searched rows, behind their search,
        evaluation, timeslot swap and walk; counted as _slot_swap's."""
        self._descent(t, rows, lambda **out: self.dp.move1_descent(rows["slot"], rows["room"], self.move1_descent, **out))

    def _lahc(self, rows, rng, tally):
        """tt_lahc, or with lahc_kempe > 0 tt_lahc_kempe (tt_lahc_kempe_aug
        under lahc_kempe_rooms="augment"), on the searched rows
        (on the current stream, behind their search and evaluation) and its
        counts, summed on the device behind the call. The rows that walk are
        the feasible ones: the call's own gate is tt_eval's hcv."""
        t = tally["lahc"]
        gain, accepted = t.out["gain"], t.out["accepted"]
        n = int(rows["slot"].shape[0])
        if self.lahc_walkers > 1:
            # tt_lahc_multi with the walk the island would call: without chains p_kempe 0 and
            # room_rule 0, which is tt_lahc's walk
            tw, tk = tally["lahc_walkers"], tally.get("lahc_kempe")
            winner, first = tw.out["winner"], tw.out["walker_gain"]
            self.dp.lahc_multi(rows["slot"], rows["room"], rng, self.lahc_walkers, self.lahc, self.lahc_history,
                               self.lahc_swap, self.lahc_kempe, self.lahc_kempe_max_chain,
                               int(self.lahc_kempe_rooms == "augment"), scv=rows["scv"], penalty=rows["penalty"],
                               gain=gain, accepted=accepted, best_step=t.out["best_step"],
                               kempe_stats=tk.out["stats"] if tk else None, winner=winner, walker_gain=first,
                               work=tw.work)
            if tk:
                tk.add(n, *tk.out["stats"][:, :len(tk.sums)].sum(dim=0).unbind())
            tw.add(0, (rows["feasible"] != 0).sum(), gain.sum(), first[:, 0].sum(), (winner > 0).sum())
        elif self.lahc_kempe > 0 and self.lahc_kempe_rooms == "augment":
            tk = tally["lahc_kempe"]
            self.dp.lahc_kempe_aug(rows["slot"], rows["room"], rng, self.lahc, self.lahc_history, self.lahc_swap,
                                   self.lahc_kempe, self.lahc_kempe_max_chain, 1, scv=rows["scv"],
                                   penalty=rows["penalty"], gain=gain, accepted=accepted, best_step=t.out["best_step"],
                                   kempe_stats=tk.out["stats"])
            tk.add(n, *tk.out["stats"].sum(dim=0).unbind())
        elif self.lahc_kempe > 0:
            tk = tally["lahc_kempe"]
            self.dp.lahc_kempe(rows["slot"], rows["room"], rng, self.lahc, self.lahc_history, self.lahc_swap,
                               self.lahc_kempe, self.lahc_kempe_max_chain, scv=rows["scv"], penalty=rows["penalty"],
                               gain=gain, accepted=accepted, best_step=t.out["best_step"], kempe_stats=tk.out["stats"])
            tk.add(n, *tk.out["stats"].sum(dim=0).unbind())
        else:
            self.dp.lahc(rows["slot"], rows["room"], rng, self.lahc, self.lahc_history, self.lahc_swap,
                         scv=rows["scv"], penalty=rows["penalty"], gain=gain, accepted=accepted,
                         best_step=t.out["best_step"])
        t.add(n, (rows["feasible"] != 0).sum(), (gain > 0).sum(), accepted.sum(), gain.sum())

    def _sum_names(self, stage: str) -> tuple:
        """The names of a tallied stage's sums: _TALLIED's, and for the chains
        of the walk under lahc_kempe_rooms="augment" tt_lahc_kempe_aug's two more."""
        names = _TALLIED[stage][3]
        if stage == "lahc_kempe" and self.lahc_kempe_rooms == "augment":
            names += ("rescued", "displaced")
        return names

    def _stats(self, stage: str) -> dict:
        """A tallied stage's row count and sums over all its holders, as Python
        ints. Pending sub-batches are replaced first; synchronises."""
        need, count, _, _, _ = _TALLIED[stage]
        names = self._sum_names(stage)
        if stage not in self.on:
            raise ValueError(f"{stage}_stats() needs Island({need})")
        self.flush()
        self.sync()
        holders = [t[stage] for t in [self._init_tally] + [p.tally for p in self._parts] if stage in t]
        totals = sum(t.sums.cpu() for t in holders).tolist()
        out = {k: int(v) for k, v in zip(names, totals)}
        return {count: sum(t.rows for t in holders), **out} if count else out

    def cx_stats(self) -> dict:
        """Island(crossover="guided"): the children bred, how many of them
        crossed, how many of those came out with cost 0, and the cost and the
        repaired events summed over the crossed children."""
        return self._stats("cx")

    def lahc_stats(self) -> dict:
        """Island(lahc > 0): the rows tt_lahc was called on, how many of them
        were feasible at entry and walked, how many came back better, the
        candidates accepted and the scv gained in all."""
        return self._stats("lahc")

    def lahc_kempe_stats(self) -> dict:
        """Island(lahc_kempe > 0): the rows tt_lahc_kempe was called on, and of
        their Kempe candidates those tried, capped, without a room and
        accepted, and the events of the accepted chains; under
        lahc_kempe_rooms="augment" also the candidates a path `rescued` and the
        bystanders the accepted chains `displaced`."""
        return self._stats("lahc_kempe")

    def lahc_walkers_stats(self) -> dict:
        """Island(lahc_walkers > 1): the `rows` that walked, the `walkers` a
        row, the winners' `gain`, `gainFirst`: the gain of walker 0 summed over
        the same rows, which is what the single walk gets from them, and
        `winnerLater`: the rows won by another walker than 0."""
        return {**self._stats("lahc_walkers"), "walkers": self.lahc_walkers}

    def slot_swap_stats(self) -> dict:
        """Island(slot_swap > 0): the rows tt_slot_swap was called on, how many
        of them it improved, the swaps applied and the scv gained in all."""
        return self._stats("slot_swap")

    def move1_descent_stats(self) -> dict:
        """Island(move1_descent > 0): the `rows` tt_move1_descent was called on,
        how many of them it `improved`, `meanPasses`: the moves applied per
        improved row (0 when there is none) and the scv gained in all."""
        st = self._stats("move1_descent")
        improved = st["improved"]
        return {"rows": st["rows"], "improved": improved,
                "meanPasses": float(st["passes"]) / improved if improved else 0.0, "gain": st["gain"]}

    def kempe_stats(self) -> dict:
        """Island(kempe > 0): the children tt_kempe_move was called on, how many
        of them moved a chain, how many chains the cap rejected, and the events
        moved in all."""
        return self._stats("kempe")

    def _replace_oldest(self):
        j = self._pending.pop(0)
        p = self._parts[j]
        with self._on_stream(p.stream):
            self._wait_op(p.stream)
            if self.unique:
                self.dp.ga_replace_unique(self.pop, p.child, p.work, p.keep, p.n_kept)
                self._dropped += p.n - p.n_kept               # on the device, behind the replacement
                self._replaced += p.n
            else:
                self.dp.ga_replace(self.pop, p.child, p.work)
            self._record_op(p.stream)
        self._last_replace = j

    def _source_range(self, part):
        """(k, n): the source word of the part's last replacement names its child
        c when k <= word < n, as word - k (tt_ga_replace: positions N - C + c;
        tt_ga_replace_unique: N + c)."""
        return (self.N, self.N + part.n) if self.unique else (self.N - part.n, self.N)

    def unique_stats(self) -> dict:
        """Island(unique=True): the children that went through a replacement, how
        many of them were dropped as duplicates, and the distinct genomes of the
        population (the i with tt_genome_first's first[i] == i), as Python ints.
        Pending sub-batches are replaced first; synchronises."""
        import torch
        if not self.unique:
            raise ValueError("unique_stats() needs Island(unique=True)")
        self.flush()
        with self._on_stream():
            first = self.dp.genome_first(self.pop["slot"], self.pop["room"])
            distinct = (first == torch.arange(self.N, dtype=torch.int32, device=first.device)).sum()
            dropped = self._dropped.clone()
        self.sync()
        return {"children": int(self._replaced), "dropped": int(dropped.item()), "distinct": int(distinct.item())}

    def flush(self):
        """Replace the pending sub-batches in order, and make the island's stream
        wait for the population's last operation (one part: nothing is pending
        and the last operation ran there)."""
        self._fork()
        while self._pending:
            self._replace_oldest()
        self._join()
        self._wait_op(self.stream)

    def snapshot(self) -> "Snapshot":
        """pop[0]'s (feasible, scv, hcv) and best_thread()'s source position,
        copied into pinned host memory behind the last replacement enqueued
        (pending sub-batches stay pending, so the snapshot is the population as
        the last replacement left it); Snapshot.values() waits for that copy
        only, so the host can log generation g while generation g + 1 runs. Two
        slots -- a pinned buffer, a device staging tensor and an event each --
        are reused in turn (generation g's snapshot is read after g + 1 has
        been enqueued). The staging tensor is the slot's own: consecutive
        snapshots may run on different parts' streams with nothing ordering
        them, and the later one must not write what the earlier one's copy to
        the host still reads."""
        import torch
        if self._snap is None:
            dev = self.pop["slot"].device
            self._snap = [(torch.empty(4, dtype=torch.int32, pin_memory=True),
                           torch.empty(4, dtype=torch.int32, device=dev), torch.cuda.Event()) for _ in range(2)]
            self._record_streams([m for _, m, _ in self._snap])
            self._snap_i = 0
            self._snap_owner = [None, None]
        i = self._snap_i
        host, m, ev = self._snap[i]
        if self._snap_owner[i] is not None:
            self._snap_owner[i].values()     # the slot's previous snapshot, read before the reuse
        self._snap_i ^= 1
        last = self._parts[self._last_replace]
        with self._on_stream(last.stream):
            off = int(self.dp.lib.tt_ga_work_source_offset(self.N, self.dp.E))
            p = self.pop
            m[0] = p["feasible"][0]
            m[1] = p["scv"][0]
            m[2] = p["hcv"][0]
            m[3] = last.work[off:off + 4].view(torch.int32)[0]
            host.copy_(m, non_blocking=True)
            ev.record()
        snap = Snapshot(host, ev, self.generation, *self._source_range(last), last.off)
        self._snap_owner[i] = snap
        return snap

    def best_thread(self) -> int:
        """The reference thread (ga.cpp:498, one per child slot) whose
        replacement put the current pop[0] in place: child c of the last
        tt_ga_replace (the source position it leaves in its own slot of the
        work buffer, tt_ga_work_source_offset), else thread 0: the child slot
        index over all sub-batches, after the pending ones are replaced."""
        self.sync()
        last = self._parts[self._last_replace]
        src = self.dp.ga_work_source(last.work, self.N)
        k, n = self._source_range(last)
        return last.off + src - k if self.generation > 0 and k <= src < n else 0


class Snapshot:
    """Island.snapshot(): pop[0]'s fields after a generation, landing in
    pinned host memory behind an event."""

    def __init__(self, host, event, generation: int, k: int, n: int, base: int = 0):
        self.host, self.event, self.generation, self.k, self.n, self.base = host, event, generation, k, n, base
        self._vals = None

    def values(self):
        """(feasible, scv, hcv, best thread) once the copy has landed (read once:
        the pinned buffer is reused two snapshots later)."""
        if self._vals is None:
            self.event.synchronize()
            f, scv, hcv, src = (int(v) for v in self.host.tolist())
            thread = self.base + src - self.k if self.generation > 0 and self.k <= src < self.n else 0
            self._vals = (bool(f), scv, hcv, thread)
        return self._vals


class CostLog:
    """setCurrentCost (ga.cpp:203-228): a logEntry line whenever pop[0] changes
    the island's best (feasible: scv differs; infeasible: hcv*1e6+scv lower)."""

    def __init__(self, proc_id: int, out, t0: float):
        self.proc_id, self.out, self.t0 = proc_id, out, t0
        self.best_scv = 2 ** 31 - 1          # beginTry (ga.cpp:163-167)
        self.best_eval = 2 ** 31 - 1

    def offer(self, feasible: bool, scv: int, hcv: int, thread_id: int = 0, t: float | None = None):
        """pop[0] now has these fields; returns the logged line or None."""
        entry = None
        if feasible:
            if scv != self.best_scv:
                self.best_scv = scv
                self.best_eval = scv
                entry = scv
        else:
            ev = hcv * 1000000 + scv
            if ev < self.best_eval:
                self.best_eval = ev
                entry = ev
        if entry is None:
            return None
        if t is None:
            t = max(0.0, time.perf_counter() - self.t0)
        line = json_line({"logEntry": {"best": entry, "procID": self.proc_id, "threadID": thread_id, "time": t}})
        if self.out is not None:
            self.out.write(line + "\n")
        return line

    def update(self, island, thread_id: int = 0):
        feas, scv, hcv, _ = island.member_meta(0)
        return self.offer(feas, scv, hcv, thread_id)

    def update_from(self, snap: "Snapshot"):
        """update() from a Snapshot taken right after the generation."""
        feas, scv, hcv, thread = snap.values()
        return self.offer(feas, scv, hcv, thread)


def run_best_line(feasible: bool, total_best: int) -> str:
    """setGlobalCost's line (ga.cpp:234-257), printed by rank 0."""
    return json_line({"runEntry": {"feasible": bool(feasible), "totalBest": int(total_best)}})


def solution_line(best: dict, proc_id: int, total_time: float) -> str:
    """endTry (ga.cpp:169-197) for pop[0] = `best` (Members.member fields);
    threadID is the global tid, 0 outside the parallel region."""
    sol = {"feasible": bool(best["feasible"]), "procID": int(proc_id), "threadID": 0, "totalTime": float(total_time)}
    if best["feasible"]:
        sol["totalBest"] = int(best["scv"])
        sol["timeslots"] = [int(x) for x in best["slot"]]
        sol["rooms"] = [int(x) for x in best["room"]]
    else:
        sol["totalBest"] = int(best["hcv"]) * 1000000 + int(best["scv"])
    return json_line({"solution": sol})


def unique_line(stats: dict, proc_id: int, island: int) -> str:
    """The drivers' --unique line of one island: Island.unique_stats() plus
    the island's global id (procID) and its index within the process."""
    return json_line({"unique": {"children": int(stats["children"]), "distinct": int(stats["distinct"]),
                                 "dropped": int(stats["dropped"]), "island": int(island), "procID": int(proc_id)}})


def kempe_line(stats: dict) -> str:
    """The drivers' --kempe line of one island: Island.kempe_stats() with the
    mean length of the chains moved (0 when none moved)."""
    moved = int(stats["moved"])
    return json_line({"kempe": {"children": int(stats["children"]), "moved": moved,
                                "rejected": int(stats["rejected"]),
                                "meanChain": float(stats["chain_events"]) / moved if moved else 0.0}})


def slot_swap_line(stats: dict) -> str:
    """The drivers' --slot-swap line of one island: Island.slot_swap_stats()
    with the mean number of swaps over the improved rows (0 when there are none)."""
    improved = int(stats["improved"])
    return json_line({"slotSwap": {"gain": int(stats["gain"]), "improved": improved,
                                   "meanPasses": float(stats["passes"]) / improved if improved else 0.0,
                                   "rows": int(stats["rows"])}})


def move1_descent_line(stats: dict) -> str:
    """The drivers' --move1-descent line of one island: Island.move1_descent_stats()."""
    return json_line({"move1Descent": {"gain": int(stats["gain"]), "improved": int(stats["improved"]),
                                       "meanPasses": float(stats["meanPasses"]), "rows": int(stats["rows"])}})


def lahc_line(stats: dict) -> str:
    """The drivers' --lahc line of one island: Island.lahc_stats()."""
    return json_line({"lahc": {k: int(stats[k]) for k in ("accepted", "gain", "improved", "rows", "searched")}})


def lahc_kempe_line(stats: dict) -> str:
    """The drivers' --lahc-kempe line of one island: Island.lahc_kempe_stats()
    with the mean length of the accepted chains (0 when there are none), and
    under --lahc-kempe-rooms augment `rescued` and `displaced` as well."""
    accepted = int(stats["accepted"])
    line = {"tried": int(stats["tried"]), "capped": int(stats["capped"]), "noRoom": int(stats["no_room"]),
            "accepted": accepted, "meanChain": float(stats["chain_events"]) / accepted if accepted else 0.0}
    if "rescued" in stats:
        line.update(rescued=int(stats["rescued"]), displaced=int(stats["displaced"]))
    return json_line({"lahcKempe": line})


def lahc_walkers_line(stats: dict) -> str:
    """The drivers' --lahc-walkers line of one island: Island.lahc_walkers_stats()."""
    return json_line({"lahcWalkers": {k: int(stats[k]) for k in ("gain", "gainFirst", "rows", "walkers", "winnerLater")}})


def crossover_line(stats: dict) -> str:
    """The drivers' --crossover guided line of one island: Island.cx_stats()
    with the mean cost of the crossed children (0 when none crossed)."""
    crossed = int(stats["crossed"])
    return json_line({"crossover": {"children": int(stats["children"]), "clean": int(stats["clean"]),
                                    "crossed": crossed,
                                    "meanCost": float(stats["cost"]) / crossed if crossed else 0.0,
                                    "repaired": int(stats["repaired"])}})


def run_final_line(procs: int, threads: int, total_time: float) -> str:
    """main's closing runEntry (ga.cpp:603-609)."""
    return json_line({"runEntry": {"procsNum": int(procs), "threadsNum": int(threads), "totalTime": float(total_time)}})


# The drivers' stage lines in print order: the stage (Island.on), whether its line follows
# the island's solution line directly (the others come behind all solution lines, stage by
# stage), and the line of island `isl` with global id `proc` and index `k` in its process
STAGE_LINES = (
    ("cx", True, lambda isl, proc, k: crossover_line(isl.cx_stats())),
    ("kempe", True, lambda isl, proc, k: kempe_line(isl.kempe_stats())),
    ("unique", False, lambda isl, proc, k: unique_line(isl.unique_stats(), proc, k)),
    ("slot_swap", False, lambda isl, proc, k: slot_swap_line(isl.slot_swap_stats())),
    ("lahc", False, lambda isl, proc, k: lahc_line(isl.lahc_stats())),
    ("lahc_kempe", False, lambda isl, proc, k: lahc_kempe_line(isl.lahc_kempe_stats())),
    ("lahc_walkers", False, lambda isl, proc, k: lahc_walkers_line(isl.lahc_walkers_stats())),
    ("move1_descent", False, lambda isl, proc, k: move1_descent_line(isl.move1_descent_stats())),
)
