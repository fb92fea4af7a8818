"""Population report: which constraints a device-resident population violates
and how different its individuals still are (include/ttga_report.h).

    {"best":       the six constraint parts of pop[0] (native.PART_NAMES),
     "population": {"size", "feasible", "invalid" (rows with an out-of-range
                    gene: -1 parts), "sum" (each part over the valid rows),
                    "nonzero" (valid rows where the part is non-zero)},
     "diversity":  {"events", "size", "pairs_differing"}}

pairs_differing = sum_e (N_e^2 - sum_t hist[e][t]^2) / 2 with N_e = sum_t
hist[e][t]: the (unordered pair of individuals, event) combinations whose
slots differ, 0 for a converged population, E * N * (N - 1) / 2 at most.
Every value is a Python int; the reductions run on the device in int64.
"""
from __future__ import annotations

from .ga import json_line
from .native import PART_NAMES


def pairs_differing(hist) -> int:
    """The exact count from a tt_slot_histogram tensor [E, 45]."""
    import torch
    h = hist.to(torch.int64)
    n = h.sum(dim=1)
    return int(((n * n - (h * h).sum(dim=1)).sum() // 2).item())


def population_report(dp, pop: dict) -> dict:
    """Report of a population dict (ttga.ga.new_population) on dp's device,
    enqueued on torch's current stream; synchronises to read the sums."""
    import torch
    slot, room = pop["slot"], pop["room"]
    parts = dp.eval_parts(slot, room)
    hist = dp.slot_histogram(slot)
    p64 = parts.to(torch.int64)
    valid = p64[:, 0] >= 0
    pv = p64 * valid.unsqueeze(1)
    feasible = valid & (pv[:, :3].sum(dim=1) == 0)
    tot = torch.cat([pv.sum(dim=0), (pv != 0).sum(dim=0), p64[0], valid.sum().view(1), feasible.sum().view(1)])
    v = [int(x) for x in tot.tolist()]
    k = len(PART_NAMES)
    N = int(slot.shape[0])
    return {
        "best": dict(zip(PART_NAMES, v[2 * k:3 * k])),
        "population": {"size": N, "feasible": v[3 * k + 1], "invalid": N - v[3 * k],
                       "sum": dict(zip(PART_NAMES, v[:k])), "nonzero": dict(zip(PART_NAMES, v[k:2 * k]))},
        "diversity": {"events": int(slot.shape[1]), "size": N, "pairs_differing": pairs_differing(hist)},
    }


def report_line(report: dict, proc_id: int, island: int) -> str:
    """The drivers' --report line: the report plus procID and the island's
    index within its process, in the format of the other JSON lines."""
    body = dict(report)
    body["procID"] = int(proc_id)
    body["island"] = int(island)
    return json_line({"report": body})
