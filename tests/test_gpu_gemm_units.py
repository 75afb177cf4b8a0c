"""Every instantiation of the GEMM tile kernel and every split-K reduce kernel of the library, launched once and held to the bits
of the parent of the split of gemm.hip into build units (tests/golden/gemm_units_parent.json, recorded from the parent's library
by oracle/make_goldens_gemm_units.py; cases and operands: tests/gemm_units_cases.py).  A unit that drops a kernel, launches
another form, or forgets the dynamic-LDS opt-in of the tiles above 64 KiB fails here.  (All tiles compute the same function: a
table row that names ANOTHER tile passes; profiles/gemm_split_kernel_names.log compared the traced kernel names once.)"""
import json
from pathlib import Path

import pytest

from seervideoldm_amd import _lib
from tests import gemm_units_cases as guc

pytestmark = pytest.mark.gpu
GOLDEN = json.loads((Path(__file__).parent / "golden" / "gemm_units_parent.json").read_text())
CASES = guc.cases()


def test_a_case_for_every_kernel_of_the_parent():
    assert {k for c in CASES for k in c["kernels"]} == set(GOLDEN["kernels"])
    assert sorted(c["id"] for c in CASES) == sorted(GOLDEN["cases"])


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_case_has_the_parents_bits(case, device):
    lib = _lib.load()
    launch = guc.Launch(case, device)
    assert launch.plan(lib) == guc.expected_plan(case)
    assert launch.run(lib) == GOLDEN["cases"][case["id"]]
