"""The GA's optional stages, described once: the table of their command-line
flags (ttga.islands.parse_control strips them with take(); the tools declare
them for argparse with add_arguments() and hand them to Island with
island_kwargs()) and the check of Island's stage arguments (validate()).
A flag's key is Island's keyword, parse_control's key and argparse's dest."""
from __future__ import annotations

import collections

INT_MAX = 2 ** 31 - 1

# kind "flag": a bare flag; "int" / "float": a number within arg = (low, high); "choice": one of
# the two words of arg, the first being the default. message: parse_control's error, help: argparse's
Flag = collections.namedtuple("Flag", "flag key kind arg message help")
FLAGS = (
    Flag("--unique", "unique", "flag", None, None, "duplicate-free replacement (Island(unique=True))"),
    Flag("--init", "init", "choice", ("random", "greedy"), "--init must be random or greedy",
         "the initial population: tt_random_init or tt_greedy_init (Island(init=...))"),
    Flag("--kempe", "kempe", "float", (0.0, 1.0),
         "--kempe must be a probability in [0, 1], --kempe-max-chain an integer >= 0",
         "probability of tt_kempe_move per child (Island(kempe=...)); 0: never called"),
    Flag("--kempe-max-chain", "kempe_max_chain", "int", (0, float("inf")),
         "--kempe must be a probability in [0, 1], --kempe-max-chain an integer >= 0",
         "the cap on a chain's length (0: none)"),
    Flag("--slot-swap", "slot_swap", "int", (0, INT_MAX), "--slot-swap must be a non-negative integer",
         "max_passes of tt_slot_swap behind every search (Island(slot_swap=...)); 0: never called"),
    Flag("--lahc", "lahc", "int", (0, INT_MAX), "--lahc must be a non-negative integer",
         "steps of tt_lahc behind every search (Island(lahc=...)); 0: never called"),
    Flag("--lahc-history", "lahc_history", "int", (1, INT_MAX), "--lahc-history must be a positive integer",
         "tt_lahc's history length"),
    Flag("--lahc-swap", "lahc_swap", "float", (0.0, 1.0), "--lahc-swap must be a probability in [0, 1]",
         "tt_lahc's share of Move2 candidates"),
    Flag("--lahc-kempe", "lahc_kempe", "float", (0.0, 1.0), "--lahc-kempe must be a probability in [0, 1]",
         "share of Kempe-chain candidates in the walk: tt_lahc_kempe in place of tt_lahc (Island(lahc_kempe=...)); "
         "0: tt_lahc"),
    Flag("--lahc-kempe-max-chain", "lahc_kempe_max_chain", "int", (0, INT_MAX),
         "--lahc-kempe-max-chain must be a non-negative integer", "the cap on a chain's length in the walk (0: none)"),
    Flag("--lahc-kempe-rooms", "lahc_kempe_rooms", "choice", ("direct", "augment"),
         "--lahc-kempe-rooms must be direct or augment",
         "the room rule of the walk's chains: tt_lahc_kempe's direct one, or augmenting paths, tt_lahc_kempe_aug "
         "(Island(lahc_kempe_rooms=...))"),
    Flag("--lahc-walkers", "lahc_walkers", "int", (1, 1024), "--lahc-walkers must be an integer from 1 to 1024",
         "walks from every row, each on its own stretch of the row's stream, the best one kept: tt_lahc_multi "
         "(Island(lahc_walkers=...)); 1: the single walk"),
    Flag("--crossover-repair", "crossover_repair", "flag", None, None,
         "guided: an event that clashes in both parents' slots goes to a slot of least cost"),
    Flag("--crossover", "crossover", "choice", ("uniform", "guided"), "--crossover must be uniform or guided",
         "the breeding operator: tt_ga_breed or tt_ga_breed_guided (Island(crossover=...))"),
    Flag("--move1-descent", "move1_descent", "int", (0, INT_MAX), "--move1-descent must be a non-negative integer",
         "max_passes of tt_move1_descent behind every search, timeslot swap and walk (Island(move1_descent=...)); "
         "0: never called"),
)
KEYS = tuple(f.key for f in FLAGS)


# what parse_control and the native driver say where --lahc-kempe does not go with the other --lahc flags
LAHC_KEMPE_NEEDS_LAHC = "--lahc-kempe needs --lahc"
LAHC_KEMPE_SHARES = "--lahc-swap and --lahc-kempe must not add up to more than 1"


# and where --lahc-kempe-rooms augment comes without chains
LAHC_KEMPE_ROOMS_NEEDS_KEMPE = "--lahc-kempe-rooms augment needs --lahc-kempe"


# and where --lahc-walkers comes without the walk
LAHC_WALKERS_NEEDS_LAHC = "--lahc-walkers needs --lahc"


def lahc_kempe_error(lahc, lahc_swap, lahc_kempe):
    """The message for a --lahc-kempe that does not go with --lahc and
    --lahc-swap (the values in force, defaults included), or None."""
    if lahc_kempe > 0 and lahc <= 0:
        return LAHC_KEMPE_NEEDS_LAHC
    if lahc_kempe > 0 and not lahc_swap <= 1.0 - lahc_kempe:          # tt_lahc_kempe's own test
        return LAHC_KEMPE_SHARES
    return None


def validate(init, kempe, kempe_max_chain, slot_swap, lahc, lahc_history, lahc_swap, crossover, crossover_repair,
             lahc_kempe=0.0, lahc_kempe_max_chain=0, lahc_kempe_rooms="direct", lahc_walkers=1, move1_descent=0):
    """Island's stage arguments: the first one out of range raises ValueError."""
    for ok, message in (
            (crossover in ("uniform", "guided"), "crossover must be 'uniform' or 'guided'"),
            (not crossover_repair or crossover == "guided", "crossover_repair needs crossover='guided'"),
            (init in ("random", "greedy"), "init must be 'random' or 'greedy'"),
            (0.0 <= float(kempe) <= 1.0, "kempe must be a probability in [0, 1]"),
            (int(kempe_max_chain) >= 0, "kempe_max_chain must be >= 0 (0: no cap)"),
            (int(slot_swap) >= 0, "slot_swap must be >= 0 (0: off)"),
            (int(lahc) >= 0, "lahc must be >= 0 (0: off)"),
            (int(lahc_history) >= 1, "lahc_history must be >= 1"),
            (0.0 <= float(lahc_swap) <= 1.0, "lahc_swap must be a probability in [0, 1]"),
            (0.0 <= float(lahc_kempe) <= 1.0, "lahc_kempe must be a probability in [0, 1]"),
            (int(lahc_kempe_max_chain) >= 0, "lahc_kempe_max_chain must be >= 0 (0: no cap)"),
            (not float(lahc_kempe) > 0 or int(lahc) > 0, "lahc_kempe > 0 needs lahc > 0"),
            (not float(lahc_kempe) > 0 or float(lahc_swap) <= 1.0 - float(lahc_kempe),
             "lahc_swap + lahc_kempe must be <= 1"),
            (lahc_kempe_rooms in ("direct", "augment"), "lahc_kempe_rooms must be 'direct' or 'augment'"),
            (lahc_kempe_rooms != "augment" or float(lahc_kempe) > 0, "lahc_kempe_rooms='augment' needs lahc_kempe > 0"),
            (1 <= int(lahc_walkers) <= 1024, "lahc_walkers must be from 1 to 1024"),
            (int(lahc_walkers) == 1 or int(lahc) > 0, "lahc_walkers > 1 needs lahc > 0"),
            (int(move1_descent) >= 0, "move1_descent must be >= 0 (0: off)")):
        if not ok:
            raise ValueError(message)


def take(args: list, f: Flag, err):
    """Strip flag f, and its value, from args. Returns the value (True for a
    bare flag), or None where the flag is absent; a missing or bad value
    writes f's message to err and exits with status 1."""
    if f.flag not in args:
        return None
    i = args.index(f.flag)
    if f.kind == "flag":
        del args[i]
        return True
    word = args[i + 1] if i + 1 < len(args) else None
    if f.kind == "choice":
        ok, v = word in f.arg, word
    else:
        try:
            v = (int if f.kind == "int" else float)(word)
        except (TypeError, ValueError):
            v = -1
        ok = f.arg[0] <= v <= f.arg[1]              # a NaN fails
    if not ok:
        err.write(f"Error: {f.message}\n")
        raise SystemExit(1)
    del args[i:i + 2]
    return v


def add_arguments(ap, help: dict | None = None) -> None:
    """Declare every stage flag on the argparse parser ap, with Island's own
    defaults; help[key] replaces a flag's help text (None: no text)."""
    import inspect

    from .ga import Island
    defaults = inspect.signature(Island.__init__).parameters
    for f in FLAGS:
        text = (help or {}).get(f.key, f.help)
        if f.kind == "flag":
            ap.add_argument(f.flag, action="store_true", help=text)
        elif f.kind == "choice":
            ap.add_argument(f.flag, choices=list(f.arg), default=defaults[f.key].default, help=text)
        else:
            ap.add_argument(f.flag, type=int if f.kind == "int" else float, default=defaults[f.key].default, help=text)


def island_kwargs(namespace) -> dict:
    """Island's stage keywords from a namespace add_arguments() filled."""
    return {k: getattr(namespace, k) for k in KEYS}
