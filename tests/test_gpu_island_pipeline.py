"""Island's scheduling as one pipeline of sub-batches (ttga/ga.py): the
sequence of device calls and the stream of each, for one part (the batch
schedule) and for several; no stream-ordering traffic on one part; snapshots
taken around a flush()."""
import numpy as np
import pytest

import ttga
from helpers import oracle_population
from oracle_lib import oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from ttga import native  # noqa: E402
from ttga.ga import Island, stream_seeds  # noqa: E402

N, C, STEPS, SEED = 10, 4, 50, 17
TRACED = ("ga_breed", "eval", "lpt_order", "local_search", "ga_replace")


@pytest.fixture(scope="module")
def sm():
    inst = ttga.config_instance("sm")
    return native.DeviceProblem(inst), oracle().problem(inst)


class Recorder:
    """A DeviceProblem that notes (method, torch's current stream) for every
    call of the GA's device operations and passes everything through."""

    def __init__(self, dp):
        self._dp, self.calls = dp, []

    def __getattr__(self, name):
        attr = getattr(self._dp, name)
        if name not in TRACED:
            return attr

        def traced(*a, **kw):
            self.calls.append((name, torch.cuda.current_stream()))
            return attr(*a, **kw)
        return traced


def run_traced(dp, **kw):
    rec = Recorder(dp)
    isl = Island(rec, pop_size=N, children=C, max_steps=STEPS, seed=SEED, **kw)
    isl.initialize()
    for _ in range(3):
        isl.step()
    isl.flush()
    isl.close()
    return isl, rec.calls


INIT = ["local_search", "ga_replace"]                      # initialize(): the search, then the sort


@pytest.mark.parametrize("own_stream,lpt", [(False, False), (True, False), (False, True)],
                         ids=["current_stream", "own_stream", "lpt"])
def test_one_part_call_trace(sm, own_stream, lpt):
    """The batch schedule: every call on the base stream (the island's, else
    torch's current stream), a generation being breed, (evaluation and LPT
    order,) search, replace; flush() adds nothing."""
    dp, _ = sm
    base = torch.cuda.Stream() if own_stream else torch.cuda.current_stream()
    isl, calls = run_traced(dp, lpt=lpt, stream=base if own_stream else None)
    assert isl.parts == 1
    gen = ["ga_breed", "eval", "lpt_order", "local_search", "ga_replace"] if lpt else \
        ["ga_breed", "local_search", "ga_replace"]
    assert [name for name, _ in calls] == INIT + gen + gen + gen
    assert all(st == base for _, st in calls)


def B(j):
    return ("ga_breed", j)


def S(j):
    return ("local_search", j)


def R(j):
    return ("ga_replace", j)


# (call, part) of three generations and a flush(): sub-batch h on part h % parts is bred,
# then sub-batch h - parts + 1 (if there is one) is replaced, then h is searched;
# flush() replaces what is still pending, in breed order
TWO_PARTS = [B(0), S(0), B(1), R(0), S(1),
             B(0), R(1), S(0), B(1), R(0), S(1),
             B(0), R(1), S(0), B(1), R(0), S(1),
             R(1)]
THREE_PARTS = [B(0), S(0), B(1), S(1), B(2), R(0), S(2),
               B(0), R(1), S(0), B(1), R(2), S(1), B(2), R(0), S(2),
               B(0), R(1), S(0), B(1), R(2), S(1), B(2), R(0), S(2),
               R(1), R(2)]


@pytest.mark.parametrize("parts,own_stream,expected", [(2, False, TWO_PARTS), (3, True, THREE_PARTS)],
                         ids=["2parts", "3parts_own_stream"])
def test_staggered_call_trace(sm, parts, own_stream, expected):
    """Several parts (3 of 4 children: uneven ones): per sub-batch the breed on
    its part's stream, the oldest pending part's replacement on that part's
    stream, the search on its part's stream; the parts' streams are distinct,
    part 0's being the island's (the one given, if one was)."""
    dp, _ = sm
    given = torch.cuda.Stream() if own_stream else None
    isl, calls = run_traced(dp, lpt=False, stream=given, schedule="staggered", parts=parts)
    assert isl.parts == parts
    if own_stream:
        assert isl.stream == given
    assert [name for name, _ in calls[:2]] == INIT and all(st == isl.stream for _, st in calls[:2])
    calls = calls[2:]
    assert [name for name, _ in calls] == [name for name, _ in expected]
    stream_of = {0: isl.stream}
    for (name, st), (_, j) in zip(calls, expected):
        if j not in stream_of:
            assert all(st != other for other in stream_of.values()), (name, j)
            stream_of[j] = st
        assert st == stream_of[j], (name, j)
    assert len(stream_of) == parts
    assert all(st != torch.cuda.default_stream() for st in stream_of.values())


@pytest.mark.parametrize("own_stream", [False, True], ids=["current_stream", "own_stream"])
def test_one_part_step_orders_no_streams(sm, monkeypatch, own_stream):
    """Three generations of a batch island record no event and make no stream
    wait for an event or for another stream (the reference's configuration,
    one child per generation, is bound by the host's launch overhead)."""
    dp, _ = sm
    isl = Island(dp, pop_size=N, children=C, max_steps=STEPS, seed=SEED,
                 stream=torch.cuda.Stream() if own_stream else None)
    isl.initialize()
    counts = {}
    for cls, name in ((torch.cuda.Event, "record"), (torch.cuda.Stream, "wait_event"),
                      (torch.cuda.Stream, "wait_stream")):
        def counting(self, *a, _orig=getattr(cls, name), _name=name, **kw):
            counts[_name] = counts.get(_name, 0) + 1
            return _orig(self, *a, **kw)
        monkeypatch.setattr(cls, name, counting)
    for _ in range(3):
        isl.step()
    monkeypatch.undo()
    assert counts == {}
    assert isl.generation == 3
    isl.close()


def test_snapshots_around_a_flush(sm):
    """step(), a = snapshot(), flush(), b = snapshot(), step() on a two-part
    island: a is pop[0] with the last sub-batch still pending, b with every
    sub-batch replaced, each read after the next generation was enqueued. a is
    taken on part 0's stream and b on part 1's with nothing ordering the two,
    so each snapshot slot stages its values in a device tensor of its own; the
    race a shared tensor allows (b's writes landing before a's copy to the
    host has read it) depends on timing, so this test cannot be expected to
    fail without the per-slot tensor: it fixes the values."""
    dp, o = sm
    isl = Island(dp, pop_size=N, children=C, max_steps=STEPS, seed=SEED, schedule="staggered", parts=2)
    isl.initialize()
    isl.step()
    a = isl.snapshot()
    isl.flush()
    b = isl.snapshot()
    isl.step()
    got_a, got_b = a.values(), b.values()
    isl.close()

    # the order of oracle_staggered (test_gpu_ga.py): breed(0), search(0); breed(1), replace(0), search(1)
    pop = oracle_population(o, N, SEED, STEPS)
    rng = stream_seeds(SEED, N, C)
    half = C // 2
    pending = []
    for j in (0, 1):
        cs, cr, fl, r = o.ga_breed(pop["slot"], pop["room"], pop["penalty"], rng[j * half:(j + 1) * half].copy(), half,
                                   0.8, 0.5, 1)
        if pending:
            pop = o.ga_replace(pop, pending.pop(0))
        cs, cr, r = o.local_search(cs, cr, r, STEPS)
        h, sc, f, p = o.eval(cs, cr)
        pending.append(dict(slot=cs, room=cr, hcv=h, scv=sc, feasible=f, penalty=p))

    def first(pop):
        return bool(pop["feasible"][0]), int(pop["scv"][0]), int(pop["hcv"][0])
    assert got_a[:3] == first(pop)                           # sub-batch 1 pending
    pop = o.ga_replace(pop, pending.pop(0))
    assert got_b[:3] == first(pop)                           # every sub-batch replaced
    assert np.all(np.diff(pop["penalty"].astype(np.uint32).astype(np.int64)) >= 0)
