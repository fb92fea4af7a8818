"""CPU checks of the population report (no GPU): the boundary of
include/ttga_report.h as a C++98 consumer sees it, the null-argument handling
of its entry points, the --report flag's place in the Control-style parse, and
the format of the report line both drivers print."""
import ctypes
import pathlib
import re
import shutil
import subprocess

import pytest

from stage_checks import Sink, build_and_run_consumer, check_exports, stripped_before_pair_count
from ttga import native
from ttga.islands import parse_control
from ttga.report import report_line

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "ttga_report.h"
CONSUMER = REPO / "tests" / "boundary_report_cxx98.cpp"


def test_header_symbols_are_exported_listed_and_called():
    check_exports(HEADER, None, "REPORT_EXPORTS", CONSUMER, {"tt_eval_parts", "tt_slot_histogram"})
    assert native.PART_NAMES == ("room_pairs", "corr_pairs", "unsuitable", "last_slot", "consecutive", "single_class")
    text = HEADER.read_text()
    for k, name in enumerate(native.PART_NAMES):
        assert re.search(r"#define TT_PART_%s\s+%d\b" % (name.upper(), k), text), name
    assert re.search(r"#define TT_NUM_PARTS\s+6\b", text)


def test_load_rejects_a_library_without_the_report_symbols(tmp_path):
    """A libttga.so that lacks the report entry points fails at load(), like one
    that lacks any other symbol."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "stub.cpp"
    decl = "\n".join('extern "C" int %s() { return 0; }' % s for s in native.EXPORTS)
    src.write_text(decl + "\n")
    so = tmp_path / "libstub.so"
    subprocess.run(["g++", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    with pytest.raises(AttributeError):
        native.load(so)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cxx98_report_consumer_builds_and_links(tmp_path):
    build_and_run_consumer(CONSUMER, tmp_path)


def test_null_arguments_are_invalid_without_a_device():
    lib = native.load()
    buf = (ctypes.c_int32 * 64)()
    genes = (ctypes.c_uint8 * 8)()
    for args in ((None, None, None, 1, None, None, None), (None, genes, genes, 1, buf, None, None),
                 (None, genes, genes, 1, buf, buf, None), (None, genes, genes, -1, buf, None, None)):
        assert lib.tt_eval_parts(*args) == native.TT_ERR_INVALID
        assert b"null tt_problem" in lib.tt_last_error()
    for args in ((None, None, 1, None, None), (None, genes, 1, buf, None), (None, genes, 0, buf, None)):
        assert lib.tt_slot_histogram(*args) == native.TT_ERR_INVALID
        assert b"null tt_problem" in lib.tt_last_error()


def test_report_flag_is_stripped_before_the_pair_count():
    stripped_before_pair_count(["--report"])
    ctl = parse_control(["-i", "x.tim", "--report", "-s", "42"], out=Sink(), err=Sink())
    assert ctl["report"] is True and ctl["seed"] == 42 and ctl["input"] == "x.tim"
    assert "report" not in parse_control(["-i", "x.tim", "-s", "42"], out=Sink(), err=Sink())


def test_report_line_format():
    names = native.PART_NAMES
    rep = {"best": dict(zip(names, (0, 2, 1, 30, 4, 5))),
           "population": {"size": 12, "feasible": 3, "invalid": 0, "sum": dict(zip(names, (1, 20, 3, 400, 50, 60))),
                          "nonzero": dict(zip(names, (1, 9, 2, 12, 11, 12)))},
           "diversity": {"events": 100, "size": 12, "pairs_differing": 5000000000}}
    assert report_line(rep, 3, 1) == (
        '{"report":{"best":{"consecutive":4,"corr_pairs":2,"last_slot":30,"room_pairs":0,"single_class":5,'
        '"unsuitable":1},"diversity":{"events":100,"pairs_differing":5000000000,"size":12},"island":1,'
        '"population":{"feasible":3,"invalid":0,"nonzero":{"consecutive":11,"corr_pairs":9,"last_slot":12,'
        '"room_pairs":1,"single_class":12,"unsuitable":2},"size":12,"sum":{"consecutive":50,"corr_pairs":20,'
        '"last_slot":400,"room_pairs":1,"single_class":60,"unsuitable":3}},"procID":3}}')
    assert "procID" not in rep and "island" not in rep
