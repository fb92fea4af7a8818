"""CPU checks of duplicate-free replacement (no GPU): the boundary of
include/ttga_unique.h as a C++98 consumer sees it, the argument handling of its
entry points before any device call, the --unique flag's place in the
Control-style parse, and the format of the unique line both drivers print."""
import ctypes
import pathlib
import shutil

import pytest

from stage_checks import Sink, build_and_run_consumer, check_exports, stripped_before_pair_count
from ttga import native
from ttga.ga import unique_line
from ttga.islands import parse_control

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "ttga_unique.h"
CONSUMER = REPO / "tests" / "boundary_unique_cxx98.cpp"


def test_header_symbols_are_exported_listed_and_called():
    check_exports(HEADER, None, "UNIQUE_EXPORTS", CONSUMER,
                  {"tt_genome_work_bytes", "tt_genome_first", "tt_ga_unique_work_bytes", "tt_ga_replace_unique"})
    assert '#include "ttga.h"' in HEADER.read_text()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_cxx98_unique_consumer_builds_and_links(tmp_path):
    build_and_run_consumer(CONSUMER, tmp_path)


def _replace_args(handle, N, C, hash_bits, buf, work):
    return (handle,) + (buf,) * 6 + (N,) + (buf,) * 6 + (C, buf, buf, hash_bits, work, None)


def test_argument_errors_without_a_device():
    lib = native.load()
    buf = (ctypes.c_int32 * 64)()
    # a null handle is named, whatever else is wrong
    for args in ((None, None, None, 1, None, 0, None, None), (None, buf, buf, 1, buf, 0, buf, None),
                 (None, buf, buf, -1, buf, 0, buf, None), (None, buf, buf, 1, buf, 32, buf, None)):
        assert lib.tt_genome_first(*args) == native.TT_ERR_INVALID
        assert b"null tt_problem" in lib.tt_last_error()
    for N, C, bits, work in ((4, 2, 0, buf), (4, 5, 0, buf), (4, -1, 0, buf), (0, 0, 0, buf), (4, 2, 32, buf),
                             (4, 2, 0, None)):
        assert lib.tt_ga_replace_unique(*_replace_args(None, N, C, bits, buf, work)) == native.TT_ERR_INVALID
        assert b"null tt_problem" in lib.tt_last_error()
    # with a handle, sizes, buffers and hash_bits are checked before any device call: a
    # stand-in handle that the library must not look into
    fake = ctypes.cast((ctypes.c_uint8 * 8)(), ctypes.c_void_p)
    for args in ((fake, None, buf, 1, buf, 0, buf, None), (fake, buf, None, 1, buf, 0, buf, None),
                 (fake, buf, buf, 1, None, 0, buf, None), (fake, buf, buf, 1, buf, 0, None, None),
                 (fake, buf, buf, -1, buf, 0, buf, None), (fake, buf, buf, 1, buf, 32, buf, None),
                 (fake, buf, buf, 1, buf, -1, buf, None)):
        assert lib.tt_genome_first(*args) == native.TT_ERR_INVALID
        assert b"null tt_problem" not in lib.tt_last_error()
    assert lib.tt_genome_first(fake, None, None, 0, None, 0, None, None) == native.TT_OK
    for N, C, bits, work in ((4, 5, 0, buf), (4, -1, 0, buf), (0, 0, 0, buf), (-3, 0, 0, buf), (4, 2, 32, buf),
                             (4, 2, -1, buf), (4, 2, 0, None), (4, 0, 32, buf)):
        assert lib.tt_ga_replace_unique(*_replace_args(fake, N, C, bits, buf, work)) == native.TT_ERR_INVALID
    for k in (8, 13, 15, 16):                    # a null child buffer, keep or n_kept with C > 0
        args = list(_replace_args(fake, 4, 2, 0, buf, buf))
        args[k] = None
        assert lib.tt_ga_replace_unique(*args) == native.TT_ERR_INVALID


def test_work_bytes():
    lib = native.load()
    for P, E in ((0, 100), (-1, 100), (10, 0), (10, -5)):
        assert lib.tt_genome_work_bytes(P, E) == 0
    for N, C, E in ((0, 0, 100), (-1, 0, 100), (10, -1, 100), (10, 2, 0)):
        assert lib.tt_ga_unique_work_bytes(N, C, E) == 0
    assert lib.tt_genome_work_bytes(1, 1) >= 16 and lib.tt_genome_work_bytes(9000, 65) >= 2 * 8 * 9000
    for N, C, E in ((1, 0, 1), (10, 1, 100), (64, 16, 100), (300, 300, 20), (9000, 8500, 20), (65536, 8192, 400)):
        assert lib.tt_ga_unique_work_bytes(N, C, E) >= lib.tt_ga_work_bytes(N, E) + 4 * N + 32 * C
        assert lib.tt_ga_unique_work_bytes(N, C, E) >= lib.tt_ga_unique_work_bytes(N, max(C - 1, 0), E)
        assert lib.tt_ga_work_source_offset(N, E) + 4 <= lib.tt_ga_work_bytes(N, E)


def test_unique_flag_is_stripped_before_the_pair_count():
    stripped_before_pair_count(["--unique"])
    ctl = parse_control(["-i", "x.tim", "--unique", "-s", "42"], out=Sink(), err=Sink())
    assert ctl["unique"] is True and ctl["seed"] == 42 and ctl["input"] == "x.tim"
    assert "unique" not in parse_control(["-i", "x.tim", "-s", "42"], out=Sink(), err=Sink())
    both = parse_control(["--report", "-i", "x.tim", "--unique"], out=Sink(), err=Sink())
    assert both["unique"] is True and both["report"] is True


def test_unique_line_format():
    stats = {"children": 4800, "dropped": 1222, "distinct": 64}
    assert unique_line(stats, 3, 1) == (
        '{"unique":{"children":4800,"distinct":64,"dropped":1222,"island":1,"procID":3}}')
    assert "procID" not in stats and "island" not in stats
