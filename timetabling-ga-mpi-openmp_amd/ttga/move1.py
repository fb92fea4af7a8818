"""Where can an event go, and is this timetable a local optimum?

    python -m ttga.move1 instance.tim [output.jsonl | -] [--event E]

For every feasible `solution` line of a driver's output (parsed as
ttga.validate does) one JSON line from tt_move1_scan (include/ttga/move1.h):

    {"move1": {"procID", "feasibleMoves", "improving", "bestDelta", "bestEvent", "bestSlot"}}

feasibleMoves: the single-event moves that keep hcv 0; improving: those that
lower scv (0: the timetable is a local optimum of this neighbourhood);
bestDelta, bestEvent, bestSlot: the move of least change of scv (-1, -1 and a
delta of 0 where there is no feasible move). With --event E the line also
carries that event's 45 "d_scv" values (the change of scv in every slot) and
its 45 "to_room" codes (the room it would take there; 255: a correlated event
sits in the slot, 254: no possible room is free). A timetable the scan refuses
(hcv != 0 under the library's own gate) gets "scanned": false and nothing else.

A solution line whose timetable has another length than E, a gene out of range
or, under ttga.validate's evaluation, hcv != 0 is left out with a word on
stderr. It needs a GPU, as everything else here does. Exit status 1 if no
feasible solution line was read, 3 if some line was left out."""
from __future__ import annotations

import json
import sys

import numpy as np

from .native import NUM_SLOTS


def move_table(dp, slot, room):
    """(summary int32 [P, 6], d_scv int32 [P, E, 45], to_room uint8 [P, E, 45])
    of tt_move1_scan as numpy arrays; slot, room: uint8 [P, E] or [E] arrays."""
    import torch
    slot, room = np.atleast_2d(np.asarray(slot, np.uint8)), np.atleast_2d(np.asarray(room, np.uint8))
    P, E = slot.shape
    dev = torch.device("cuda", dp.device)
    s, r = torch.from_numpy(np.ascontiguousarray(slot)).to(dev), torch.from_numpy(np.ascontiguousarray(room)).to(dev)
    summary = torch.empty((P, 6), dtype=torch.int32, device=dev)
    d_scv = torch.empty((P, E, NUM_SLOTS), dtype=torch.int32, device=dev)
    to_room = torch.empty((P, E, NUM_SLOTS), dtype=torch.uint8, device=dev)
    dp.move1_scan(s, r, summary=summary, d_scv=d_scv, to_room=to_room)
    torch.cuda.synchronize(dev)
    return summary.cpu().numpy(), d_scv.cpu().numpy(), to_room.cpu().numpy()


def move1_line(proc_id, summary, d_scv=None, to_room=None, event=None) -> str:
    """The tool's line for one timetable: its summary row and, with `event`, that event's rows of the tables."""
    from .ga import json_line
    if not summary[0]:
        return json_line({"move1": {"procID": proc_id, "scanned": False}})
    line = {"procID": proc_id, "feasibleMoves": int(summary[1]), "improving": int(summary[2]),
            "bestDelta": int(summary[3]), "bestEvent": int(summary[4]), "bestSlot": int(summary[5])}
    if event is not None:
        line.update(event=int(event), d_scv=[int(x) for x in d_scv[event]], to_room=[int(x) for x in to_room[event]])
    return json_line({"move1": line})


def solutions(inst, text: str, err=sys.stderr):
    """(procID, timeslots, rooms) of every solution line that carries a
    timetable which ttga.validate finds feasible, and how many lines were left
    out with a word on `err`: a timetable of another length than E, a gene out
    of range, or hard-constraint violations."""
    from .validate import evaluate
    found, left_out = [], 0
    for ln in text.splitlines():
        if not ln.startswith("{"):
            continue
        try:
            obj = json.loads(ln)
        except ValueError:
            continue
        sol = obj.get("solution") if isinstance(obj, dict) else None
        if not isinstance(sol, dict) or "timeslots" not in sol or "rooms" not in sol:
            continue                                 # an infeasible solution line carries only its cost
        t, r, who = sol["timeslots"], sol["rooms"], sol.get("procID")
        if len(t) != inst.E or len(r) != inst.E:
            why = f"{len(t)} timeslots and {len(r)} rooms for {inst.E} events"
        elif not all(isinstance(x, int) and 0 <= x < NUM_SLOTS for x in t) or \
                not all(isinstance(x, int) and 0 <= x < inst.R for x in r):
            why = "a timeslot outside 0..44 or a room outside 0..R-1"
        else:
            hcv = evaluate(inst, t, r)["hcv"]
            why = f"hcv {hcv}" if hcv else None
        if why:
            err.write(f"solution of procID {who} left out: {why}\n")
            left_out += 1
        else:
            found.append((who, t, r))
    return found, left_out


def main(argv=None) -> int:
    from .instance import read_tim
    from .native import DeviceProblem
    argv = list(sys.argv[1:] if argv is None else argv)
    event = None
    if "--event" in argv:
        i = argv.index("--event")
        try:
            event = int(argv[i + 1])
        except (IndexError, ValueError):
            event = -1
        del argv[i:i + 2]
    if not argv or len(argv) > 2:
        sys.stderr.write("usage: python -m ttga.move1 instance.tim [output.jsonl | -] [--event E]\n")
        return 2
    inst = read_tim(argv[0])
    if event is not None and not 0 <= event < inst.E:
        sys.stderr.write(f"--event must be an event of the instance, 0 to {inst.E - 1}\n")
        return 2
    text = sys.stdin.read() if len(argv) == 1 or argv[1] == "-" else open(argv[1]).read()
    found, left_out = solutions(inst, text)
    if not found:
        return 1
    import torch  # noqa: F401  (before the library is loaded: one HIP runtime in the process)
    dp = DeviceProblem(inst)
    summary, d_scv, to_room = move_table(dp, np.array([s[1] for s in found]), np.array([s[2] for s in found]))
    for k, (proc_id, _, _) in enumerate(found):
        print(move1_line(proc_id, summary[k], d_scv[k], to_room[k], event))
    dp.close()
    return 3 if left_out else 0


if __name__ == "__main__":
    sys.exit(main())
