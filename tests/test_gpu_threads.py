"""One tt_problem, four host threads (ttga.h: "One tt_problem may be used by
several host threads on different streams").

A fresh handle, so the first-call decisions race (the memoised occupancies of
tt_eval and of the local search's masks, the per-stream redo records under the
handle's mutex); four threads released together, each on its own stream with
its own seeds and buffers: random_init, eval, three local_search_eval calls
(the third decides its masks from the first's counts), mutation, eval. Every
thread's rows, streams and outputs equal the oracle's, its
tt_local_search_stats equal those of the same sequence run alone on a fresh
handle, tt_last_error is the calling thread's own, and the handle's status is
0. Run once: the test does not hunt for a race."""
import ctypes
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ttga
from helpers import dev
from oracle_lib import oracle

pytestmark = pytest.mark.gpu

import torch  # noqa: E402
from ttga import native  # noqa: E402

T, P, STEPS, CALLS = 4, 67, 300, 3
BAD, QUIET = 1, 2                      # the thread that makes a refused call, and one that reads its own message


def instance():
    return ttga.generate(80, 10, 5, 120, seed=101)         # tests/test_gpu_footprint.py's A: E > 64, the redo records


def seeds_of(t):
    return ttga.population_seeds(5000 + 97 * t, P)


def sequence(dp, t, start=None, bad_done=None):
    """Thread t's calls on a stream of its own; returns the host copies of every
    stage, the stream's search statistics and what tt_last_error said."""
    E = dp.E
    lib = dp.lib
    said = {"start": lib.tt_last_error()}
    st = torch.cuda.Stream()
    stages = []
    with torch.cuda.stream(st):
        rng = dev(seeds_of(t))
        slot = torch.empty((P, E), dtype=torch.uint8, device="cuda")
        room = torch.empty_like(slot)

        def outputs():
            return (torch.empty(P, dtype=torch.int32, device="cuda"), torch.empty(P, dtype=torch.int32, device="cuda"),
                    torch.empty(P, dtype=torch.uint8, device="cuda"), torch.empty(P, dtype=torch.int32, device="cuda"))

        def stage(out):
            stages.append((slot.clone(), room.clone(), rng.clone(), *out))
        if start is not None:
            start.wait(120)
        dp.random_init(rng, slot, room)
        stage(dp.eval(slot, room))
        for k in range(CALLS):
            out = outputs()
            dp.local_search(slot, room, rng, STEPS, out=out)
            stage(out)
            if t == BAD and k == 1 and bad_done is not None:
                rc = lib.tt_eval(dp.handle, slot.data_ptr(), room.data_ptr(), -1, out[0].data_ptr(), out[1].data_ptr(),
                                 out[2].data_ptr(), out[3].data_ptr(), ctypes.c_void_p(st.cuda_stream))
                said["rc"], said["bad"] = rc, lib.tt_last_error()
                bad_done.set()
        dp.mutation(slot, room, rng)
        stage(dp.eval(slot, room))
        st.synchronize()
        stats = dp.local_search_stats(st)
    if t == QUIET and bad_done is not None:
        assert bad_done.wait(120)                          # set as soon as the other thread's call was refused
    said["end"] = lib.tt_last_error()
    return [tuple(x.cpu().numpy() for x in s) for s in stages], stats, said


def expected(o, t):
    """The oracle's stages for thread t's seeds."""
    s, r, g = o.random_init(seeds_of(t))
    out = [(s, r, g, *o.eval(s, r))]
    for _ in range(CALLS):
        s, r, g = o.local_search(s, r, g, STEPS)
        out.append((s, r, g, *o.eval(s, r)))
    s, r, g = o.mutation(s, r, g)
    out.append((s, r, g, *o.eval(s, r)))
    return out


def test_four_threads_one_handle():
    inst = instance()
    assert inst.E > 64                                     # the searches keep per-stream records on the handle
    o = oracle().problem(inst)
    dp = native.DeviceProblem(inst)                        # fresh: nothing decided yet
    start, bad_done = threading.Barrier(T), threading.Event()
    with ThreadPoolExecutor(T) as ex:
        futs = [ex.submit(sequence, dp, t, start, bad_done) for t in range(T)]
        got = [f.result(timeout=600) for f in futs]
    names = ("slot", "room", "rng", "hcv", "scv", "feasible", "penalty")
    for t in range(T):
        want = expected(o, t)
        assert len(got[t][0]) == len(want) == CALLS + 2
        for k, (g, w) in enumerate(zip(got[t][0], want)):
            for n, a, b in zip(names, g, w):
                assert np.array_equal(a, b), f"thread {t}, stage {k}: {n} differs from the oracle"
    assert dp.status() == 0
    # the statistics of each stream: those of the same sequence alone on a fresh handle
    for t in range(T):
        alone = native.DeviceProblem(inst)
        stages, stats, _ = sequence(alone, t)
        assert stats == got[t][1], f"thread {t}: stats {got[t][1]} in the crowd, {stats} alone"
        assert stats[1] > 0 and stats[0] <= stats[1]
        for g, w in zip(stages, got[t][0]):
            assert all(np.array_equal(a, b) for a, b in zip(g, w))
        assert alone.status() == 0
        alone.close()
    # tt_last_error is per thread
    said = got[BAD][2]
    assert said["rc"] == native.TT_ERR_INVALID and said["bad"] == b"negative population size"
    assert said["end"] == said["bad"] and said["start"] != said["bad"]
    quiet = got[QUIET][2]
    assert quiet["end"] == quiet["start"] and quiet["end"] != said["bad"]
    dp.close()
