"""Helpers shared by the test modules (imported like oracle_lib; no fixtures)."""
import json
import socket

import numpy as np


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def oracle_population(o, N, seed, steps, p1=1.0, p2=1.0, p3=0.0):
    """Island.initialize() on the oracle's primitives: ga.cpp:429-434 for every
    member (local search with move probabilities p1, p2, p3), then the
    population sorted."""
    from ttga.ga import stream_seeds
    s, r, g = o.random_init(stream_seeds(seed, 0, N))
    s, r, g = o.local_search(s, r, g, steps, p1, p2, p3)
    h, sc, f, p = o.eval(s, r)
    pop = dict(slot=s, room=r, hcv=h, scv=sc, feasible=f, penalty=p)
    empty = {k: v[:0] for k, v in pop.items()}
    return o.ga_replace(pop, empty)


def oracle_generations(o, pop, rng, C, gens, steps, p1=1.0, p2=1.0, p3=0.0):
    """Island.step() `gens` times on the oracle's primitives (the ga.cpp:543-585
    loop for C children at once): breed, local search, eval, replace-worst +
    sort. Returns the population and the children's streams."""
    for _ in range(gens):
        cs, cr, fl, rng = o.ga_breed(pop["slot"], pop["room"], pop["penalty"], rng, C, 0.8, 0.5, 1)
        cs, cr, rng = o.local_search(cs, cr, rng, steps, p1, p2, p3)
        h, sc, f, p = o.eval(cs, cr)
        pop = o.ga_replace(pop, dict(slot=cs, room=cr, hcv=h, scv=sc, feasible=f, penalty=p))
    return pop, rng


def free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def json_lines(text):
    """JSON lines with the wall-clock fields removed."""
    out = []
    for ln in text.splitlines():
        if ln.startswith("{"):
            obj = json.loads(ln)
            for v in obj.values():
                v.pop("time", None)
                v.pop("totalTime", None)
            out.append(obj)
    return out
