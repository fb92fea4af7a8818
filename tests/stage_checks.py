"""What the test modules of every optional stage share (imported like
helpers.py; no fixtures, no GPU import at module level): the boundary of a
stage's header as a C++98 consumer sees it, the stage's flags in both drivers'
parse, the two drivers run side by side, and the small Island run of the
walk-family modules. tests/test_stage_checks_cpu.py plants the defects these
checks must catch."""
import os
import pathlib
import re
import subprocess
import sys

import pytest

from helpers import json_lines

REPO = pathlib.Path(__file__).resolve().parent.parent
PKG = REPO / "timetabling-ga-mpi-openmp_amd"
GA = PKG / "ttga-ga"
PAIR_COUNT = "Parse error: Number of command line parameters incorrect"
_CALL = r"\b(tt_[a-z_0-9]+)\s*\("


# ---------------------------------------------------------------- the boundary
def header_symbols(header, guard=None):
    """The tt_ functions a header declares; with a guard, those below its #ifndef."""
    text = pathlib.Path(header).read_text()
    return set(re.findall(_CALL, text if guard is None else text.split("#ifndef " + guard)[1]))


def check_exports(header, guard, group, consumer, expect=None, native=None):
    """A header's symbols are `expect`, are ttga.native's tuple `group` and belong
    to no other *EXPORTS tuple there, whichever stage added it; libttga.so has
    every one and the consumer calls every one. Returns the symbols."""
    if native is None:
        from ttga import native
    syms = header_symbols(header, guard)
    assert expect is None or syms == set(expect), sorted(syms)
    assert syms == set(getattr(native, group)), (group, sorted(syms))
    others = [n for n in dir(native) if n.endswith("EXPORTS") and n != group]
    assert "EXPORTS" in others and len(others) >= 10, others
    for other in others:
        assert not syms & set(getattr(native, other)), (other, sorted(syms & set(getattr(native, other))))
    lib = native.load()
    for s in syms:
        assert hasattr(lib, s), s
    called = set(re.findall(_CALL, pathlib.Path(consumer).read_text()))
    assert syms <= called, sorted(syms - called)
    return syms


def build_and_run_consumer(consumer, tmp_path):
    """The reference's flags, warning-free; then the run: without a GPU it stops
    at TT_ERR_DEVICE (2) after the null-handle checks, with one it ends at 0
    after the checks against a live handle."""
    exe = tmp_path / "consumer"
    r = subprocess.run(["g++", "-Wall", "-ansi", "-O3", "-pedantic", "-Werror", "-I", str(REPO / "include"),
                        "-I", str(REPO / "tests"), str(consumer), "-L", str(PKG), "-lttga", f"-Wl,-rpath,{PKG}",
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode in (0, 2), run.stdout + run.stderr
    if run.returncode == 2:
        assert "TT_ERR_DEVICE" in run.stdout and "null-handle checks: 0 wrong" in run.stdout
    else:
        assert "null-buffer checks: 0 wrong" in run.stdout
    return run


# ---------------------------------------------------------------- the flags
class Sink:
    def __init__(self):
        self.text = ""

    def write(self, s):
        self.text += s


def _rejected(text, message, exact, what):
    if exact:
        assert text == f"Error: {message}\n", (what, text)
    else:
        assert message in text, (what, text)


def rejected_by_parse_control(bad, message, exact):
    """parse_control leaves with status 1 and the message (exact: nothing but it)."""
    from ttga.islands import parse_control
    err = Sink()
    with pytest.raises(SystemExit) as ex:
        parse_control(bad, out=Sink(), err=err)
    assert ex.value.code == 1, (bad, ex.value.code)
    _rejected(err.text, message, exact, bad)


def rejected_by_native_driver(bad, message, exact):
    assert GA.exists(), "ttga-ga not built (make -C timetabling-ga-mpi-openmp_amd)"
    r = subprocess.run([str(GA), *bad], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (bad, r.returncode, r.stderr)
    _rejected(r.stderr, message, exact, bad)


def stripped_before_pair_count(flags):
    """The stage's flags and their values leave the argument list before the
    reference's pair count: with a lone -s behind them both drivers stop there."""
    from ttga.islands import parse_control
    assert GA.exists(), "ttga-ga not built (make -C timetabling-ga-mpi-openmp_amd)"
    r = subprocess.run([str(GA), *flags, "-s"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and PAIR_COUNT in r.stderr, r.stderr
    with pytest.raises(SystemExit) as ex:
        parse_control([*flags, "-s"], out=Sink(), err=Sink())
    assert ex.value.code == 1


# ---------------------------------------------------------------- the drivers
def run_driver(cmd, cwd):
    env = dict(os.environ, PYTHONPATH=str(PKG))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=str(cwd))
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def stage_lines(text, key):
    return [ln for ln in text.splitlines() if ln.startswith('{"%s"' % key)]


def same_output(py_text, cc_text, key, inst=None):
    """The two drivers' outputs of one run: the same JSON lines, the stage's own
    line byte for byte and somewhere behind `solution`, and (given the instance)
    every solution valid. key None: a stage without a line. Returns the parsed
    lines and the stage's among them."""
    a, b = json_lines(py_text), json_lines(cc_text)
    assert a == b and a
    lines = []
    if key is not None:
        assert stage_lines(py_text, key) == stage_lines(cc_text, key)
        lines = [x[key] for x in a if key in x]
        kinds = [next(iter(x)) for x in a]
        assert lines and kinds.index(key) > kinds.index("solution"), kinds
    if inst is not None:
        from ttga.validate import check_text
        for text in (py_text, cc_text):
            reps = check_text(inst, text)
            assert reps and all(x["ok"] for x in reps), reps
    return a, lines


def both_drivers(tmp_path, base, flags, key, inst):
    """python -m ttga.islands and ttga-ga on the same arguments (the flags behind
    the base for the one, in front for the other), through same_output. Returns
    both finished processes, the parsed lines and the stage's lines."""
    assert GA.exists(), "ttga-ga not built (make -C timetabling-ga-mpi-openmp_amd)"
    py = run_driver([sys.executable, "-m", "ttga.islands", *base, *flags], tmp_path)
    cc = run_driver([str(GA), *flags, *base], tmp_path)
    a, lines = same_output(py.stdout, cc.stdout, key, inst)
    return py, cc, a, lines


# ---------------------------------------------------------------- Island
def run_island(dp, gens=30, children=1, **kw):
    from ttga.ga import Island
    isl = Island(dp, pop_size=10, children=children, max_steps=50, seed=31, **kw)
    isl.initialize()
    for _ in range(gens):
        isl.step()
    isl.flush()
    return isl


VARIANTS = {"batch": {}, "staggered": dict(schedule="staggered", parts=2, children=4), "unique": dict(unique=True),
            "slot_swap": dict(slot_swap=1)}
