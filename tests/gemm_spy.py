"""TEST INFRASTRUCTURE ONLY -- the `spy` fixture of the GEMM matrices (tests/test_gpu_t320_matrix.py, tests/test_gpu_gemm_epi_matrix.py):
proves from seer_gemm_plan WHICH kernel a launch ran.  A tile request silently falls back when a launch is not eligible for it, so the
descriptor ops._launch_gemm hands to seer_gemm_bf16 (workspace and sync filled in) is captured and the plan of exactly that descriptor
is recorded.  A test module imports the fixture by name:  from tests.gemm_spy import spy  # noqa: F401"""
import ctypes as C_

import pytest


class _Spy:
    """stands in for the loaded library: seer_gemm_bf16 records seer_gemm_plan of the descriptor it is handed (and a copy of it), then
    launches; everything else passes through"""

    def __init__(self, lib):
        self._real, self.plans, self.descs, self.tweak, self.keep = lib, [], [], None, []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def plan_of(self, d):
        out = (C_.c_int32 * 5)()
        assert self._real.seer_gemm_plan(C_.byref(d), out) == 0
        return list(out)

    def seer_gemm_bf16(self, dref, stream):
        d = dref._obj
        self.plans.append(self.plan_of(d))
        self.descs.append(type(d).from_buffer_copy(d))
        return self._real.seer_gemm_bf16(dref, stream)


@pytest.fixture
def spy(monkeypatch):
    from seervideoldm_amd import ops
    s = _Spy(ops._lib.load())
    monkeypatch.setattr(ops._lib, "load", lambda: s)
    launch = ops._launch_gemm

    def tweaked(d, *a, **kw):
        if s.tweak is not None:
            s.tweak(d)                                                   # a field the wrappers do not expose (a phase launch with splits)
        return launch(d, *a, **kw)
    monkeypatch.setattr(ops, "_launch_gemm", tweaked)
    return s
