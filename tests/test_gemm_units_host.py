"""The build units of the GEMM tile kernel, read from the device assembly the build keeps (seervideoldm_amd/lib/obj/*gfx950.s) and
from the host planner: every instantiation of seer_gemm_kernel and every split-K reduce kernel is emitted exactly once, they are
the kernels the parent of the split emitted from its one gemm.hip (tests/golden/gemm_units_parent.json, recorded by
oracle/make_goldens_gemm_units.py), and every tile code the parent's planner took by name is still taken, with the same plan.
No GPU.  A missing build is a failure, as it is for the plan tests."""
import json
from pathlib import Path

import pytest

from seervideoldm_amd import _lib
from seervideoldm_amd.build import LIBDIR, SOURCES
from tests import gemm_units_cases as guc

GOLDEN = json.loads((Path(__file__).parent / "golden" / "gemm_units_parent.json").read_text())


@pytest.fixture(scope="module")
def emitted():
    """kernel symbol -> the units whose assembly holds it, over the sources of the library"""
    _lib.load()                                     # (raises with the build command when there is no build)
    where = {}
    for src in SOURCES:
        asm = LIBDIR / "obj" / f"{Path(src).stem}-hip-amdgcn-amd-amdhsa-gfx950.s"
        assert asm.exists(), f"{asm}: the build keeps the device assembly of every source"
        for name in guc.KERNEL.findall(asm.read_text()):
            where.setdefault(name, []).append(src)
    return where


def test_every_kernel_is_emitted_by_exactly_one_unit(emitted):
    twice = {k: v for k, v in emitted.items() if len(v) != 1}
    assert not twice, twice
    assert not [k for k, v in emitted.items() if v == ["gemm.hip"]], "the planner's unit holds no kernel"


def test_the_kernels_are_the_parents(emitted):
    assert len(GOLDEN["kernels"]) == 120 and len(set(GOLDEN["kernels"])) == 120
    assert sum("seer_gemm_kernel" in k for k in GOLDEN["kernels"]) == 116
    assert sorted(emitted) == sorted(GOLDEN["kernels"])


def test_the_case_list_names_every_kernel():
    """(the GPU test launches the cases; that they cover the fixture's kernels needs no GPU)"""
    named = {k for c in guc.cases() for k in c["kernels"]}
    assert named == set(GOLDEN["kernels"])


def test_tile_codes_the_parent_took_are_taken_with_the_same_plan():
    lib = _lib.load()
    assert sum(p[0] == 0 and p[1] == _lib.SEER_GEMM_KERNEL_TILE and p[2] == int(code) for code, p in GOLDEN["plan_256"].items()) == 18
    for code, parent in GOLDEN["plan_256"].items():
        if parent[0] == 0:
            assert guc.plan_256(lib, int(code)) == parent, code

