"""Pure-Python statement of tt_lahc_multi (include/ttga_lahc_multi.h) on top of
tests/lahc_kempe_aug_model.py: one walk of that model per walker on copies of
the entry row, the rng state chained from walk to walk, and the winner rule.
The walk itself is not restated here."""
import numpy as np

import lahc_kempe_aug_model as am
from ttga.rng import ParkMiller


class _FirstDraw(ParkMiller):
    """A 64-bit seed at or above 2^31 - 1 can make the first state negative (every
    later one is in range). The kernels clamp the index drawn from it to 0; the
    walk's model indexes with it as it is. A draw below 0 comes back as 0.0
    here, which picks index 0; in-range streams are untouched."""

    def next(self) -> float:
        return max(ParkMiller.next(self), 0.0)


class Model(am.Model):
    def lahc_multi(self, slot, room, seed, walkers, steps, history, p_swap=0.5, p_kempe=0.0, max_chain=0,
                   room_rule=1):
        """(slot, room, rng state, gain, accepted, best_step, the seven counts,
        winner, walker_gain [walkers]) of one row. A closed row (or steps 0)
        comes back as it is, rng state included, with zeros."""
        state, walks = int(seed), []
        plain, am.ParkMiller = am.ParkMiller, _FirstDraw
        try:
            for _ in range(int(walkers)):
                walks.append(self.lahc_kempe_aug(slot, room, state, steps, history, p_swap, p_kempe, max_chain,
                                                 room_rule))
                state = walks[-1][2]                                 # the next walker's stretch starts here
        finally:
            am.ParkMiller = plain
        gains = [w[3] for w in walks]
        win = gains.index(max(gains))                                # the lowest index of the largest gain
        s, r, _, gain, accepted, best_step, stats = walks[win]
        return s, r, state, gain, accepted, best_step, stats, win, tuple(gains)

    def lahc_multi_rows(self, slot, room, seeds, walkers, steps, history, p_swap=0.5, p_kempe=0.0, max_chain=0,
                        room_rule=1):
        """The whole population: (slot, room, rng, gain, accepted, best_step,
        stats [P, 7], winner [P], walker_gain [P, walkers]) as arrays."""
        out = [self.lahc_multi(slot[i], room[i], int(seeds[i]), walkers, steps, history, p_swap, p_kempe, max_chain,
                               room_rule) for i in range(len(slot))]
        i32 = lambda k, shape: np.array([o[k] for o in out], np.int32).reshape(shape)      # noqa: E731
        P = len(out)
        return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int64),
                i32(3, P), i32(4, P), i32(5, P), i32(6, (P, 7)), i32(7, P), i32(8, (P, int(walkers))))


# ---------------------------------------------------------------- the cases of tests/test_gpu_lahc_multi.py
# id: (shape, P, walkers, steps, history, p_swap, p_kempe, room_rule); rows from lahc_model.population
CASES = {
    "sm-plain": ("sm", 9, 5, 300, 50, 0.5, 0.0, 0), "sm": ("sm", 9, 5, 300, 50, 0.25, 0.5, 1),
    "E65": ("E65", 9, 3, 300, 50, 0.25, 0.5, 1), "med": ("med", 4, 3, 300, 500, 0.25, 0.5, 1),
    "E1": ("E1", 9, 3, 200, 50, 0.0, 1.0, 1), "E2": ("E2", 9, 3, 200, 50, 0.0, 1.0, 1),
    "S0": ("S0", 9, 3, 200, 50, 0.25, 0.5, 1), "R64": ("R64", 9, 3, 200, 50, 0.25, 0.5, 1),
    "tight": ("tight", 9, 3, 200, 50, 0.25, 0.5, 1), "syn_sparse": ("syn_sparse", 2, 2, 100, 100, 0.25, 0.5, 1),
}
WIDE_SEED = 2 ** 40 + 7                          # row 0 of case "sm": a 64-bit state out of range


def case_rows(cid, inst, model):
    """lahc_model.population for case cid, with WIDE_SEED in row 0 of "sm"."""
    import lahc_model as lm
    slot, room, seeds = lm.population(inst, CASES[cid][1], model)
    if cid == "sm":
        seeds[0] = WIDE_SEED
    return slot, room, seeds
