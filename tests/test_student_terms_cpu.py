"""CPU checks of eval_tile5's per-student scv terms (no GPU): the word form the
lane phase evaluates (mask_scv_shift5, csrc/tt_common.h) against the mask_scv
formula through a small host program, and the crafted populations of the GPU
test against the CPU oracle and the intended values.

tests/student_terms_host.cpp compiles the kernel's own function for the host
and feeds it masks as the kernel builds them (slot s at bit s + 5, the sentinel
column's byte 63 shifted out): every one of the 512 fields in each of the five
day positions (the other days empty and full), and 1.2 * 10^5 seeded random
45-bit masks, dense and sparse, each with bit 63 clear and set.
"""
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle_lib import oracle
from student_terms_cases import (PATTERNS, craft, golden_instance, pick_students, scv_model, spread_rows,
                                 student_terms, with_long_student)

REPO = pathlib.Path(__file__).resolve().parent.parent
CSRC = REPO / "timetabling-ga-mpi-openmp_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_word_form_matches_mask_scv(tmp_path):
    exe = tmp_path / "student_terms_host"
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++20", "-I", str(CSRC),
                    str(REPO / "tests" / "student_terms_host.cpp"), "-o", str(exe)], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:]
    checked, failed = (int(x) for x in re.search(r"checked (\d+) masks, (\d+) failed", r.stdout).groups())
    assert failed == 0 and checked >= 5 * 512 * 4 + 2 * 100000


def test_patterns_have_the_intended_terms():
    for name, (lst, want) in PATTERNS.items():
        assert student_terms(lst) == want, name
    assert student_terms(list(range(9))) == 7
    # no window across days: 8 | 9, 10 and 26 | 27, 28 leave a single class, not a triple
    assert student_terms([8, 9, 10]) == 1 and student_terms([26, 27, 28]) == 1 and student_terms([31, 32, 33]) == 1


@pytest.mark.parametrize("name,P,long_student", [("sm", 65, False), ("med", 130, False), ("sm", 65, True)],
                         ids=["sm", "med", "sm_long_student"])
def test_crafted_rows_on_the_oracle(golden_dir, name, P, long_student):
    """The oracle's scv of every row is the model's (students' terms + last-slot term), and in
    the crafted rows the chosen students' slots give the intended terms."""
    inst = golden_instance(golden_dir, name)
    if long_student:
        inst = with_long_student(inst)
        assert inst.student_events[pick_students(inst)[0]].sum() == 40
    slots, intended = craft(inst, P, 4100 + P, spread_rows(P))
    assert len({row for row, *_ in intended}) == (14 if P > 128 else 7)
    o = oracle().problem(inst)
    scv = o.eval(slots, o.assign_rooms(slots))[1]
    assert np.array_equal(scv, scv_model(inst, slots))
    for row, student, pat, want in intended:
        ev = np.flatnonzero(inst.student_events[student])
        assert student_terms(slots[row, ev]) == want, (row, student, pat)
    big = pick_students(inst)[0]
    assert {want for _, s, _, want in intended if s == big} == {w for _, w in PATTERNS.values()}
