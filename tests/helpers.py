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


def oracle_population(o, N, seed, steps):
    """Island.initialize() on the oracle's primitives: ga.cpp:429-434 for every
    member, then the population sorted."""
    from ttga.ga import stream_seeds
    s, r, g = o.random_init(stream_seeds(seed, 0, N))
    s, r, g = o.local_search(s, r, g, steps)
    h, sc, f, p = o.eval(s, r)
    pop = dict(slot=s, room=r, hcv=h, scv=sc, feasible=f, penalty=p)
    empty = {k: v[:0] for k, v in pop.items()}
    return o.ga_replace(pop, empty)


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
