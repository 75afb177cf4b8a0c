"""TEST INFRASTRUCTURE ONLY -- one launch of every instantiation of the GEMM tile kernel and of every split-K reduce kernel.

Shared by tests/test_gpu_gemm_units.py (digests against tests/golden/gemm_units_parent.json), tests/test_gemm_units_host.py (the
kernel names) and oracle/make_goldens_gemm_units.py (the recording).  The table below is written down here on purpose, not read
from csrc/gemm_tiles.h: it says which kernel stands behind a tile code at the commit the fixture was recorded from.

Cases, for each of the 18 tile codes and both storage types (bf16, IEEE half):
  plain   bias + residual, M = BM + 16 (one full tile and one ragged one), N = BN + 32, K = 64 (max(NS, 2) + 1): the ring wraps
          and the tail waits run
  geglu   the same with SEER_EPI_GEGLU where the tile allows it ((BN / 32) even)
  conv    3x3, stride 1, one 20 x 20 image, Cin = 64, Cout = BN + 32, bias
and for the four tiles that exist in split-K form, splits = 2 with K doubled:
  plain_s2 / conv_s2          the plain reduce pass
  plain_s2_cs / conv_s2_cs    the pass with per-tile column sums
  plain_s2_fx                 the pass with accumulated column sums on 32-row blocks.  That pass needs M % 32 == 0, which neither
                              BM + 16 nor the 400 rows of the conv are: this case has M = BM + 32 (still one full and one ragged tile)
  fx64 (G64x64_3 only)        the same on 64-row blocks, which takes M >= 1024: 1024 x 64 x 256
Operands come from a seeded CPU generator; a case's digest is the SHA-256 of its output bytes, then those of its column sums."""
import ctypes as C
import hashlib
import re

import torch

from seervideoldm_amd import _lib

# (SEER_TILE_* code, name, BM, BN, NS, WM, WN, split-K form)
TILES = [(1, "128x128", 128, 128, 0, 2, 2, False), (3, "128x64", 128, 64, 0, 2, 2, False), (2, "64x64", 64, 64, 0, 2, 2, True),
         (5, "G128x128_2", 128, 128, 2, 2, 2, True), (6, "G128x128_3", 128, 128, 3, 2, 2, False),
         (7, "G128x64_3", 128, 64, 3, 2, 2, False), (8, "G64x64_3", 64, 64, 3, 2, 2, True), (9, "G64x64_4", 64, 64, 4, 2, 2, False),
         (10, "G64x64_5", 64, 64, 5, 2, 2, False), (11, "G128x64_4", 128, 64, 4, 2, 2, False),
         (12, "G128x160_2", 128, 160, 2, 2, 2, False), (13, "G64x160_3", 64, 160, 3, 2, 2, False),
         (14, "G256x128_2", 256, 128, 2, 4, 2, False), (15, "G256x64_3", 256, 64, 3, 4, 2, False),
         (21, "G256x256_2", 256, 256, 2, 2, 4, False), (16, "G96x160_2", 96, 160, 2, 2, 2, True),
         (17, "G96x160_3", 96, 160, 3, 2, 2, False), (18, "G96x128_2", 96, 128, 2, 2, 2, False)]
REDUCE_KERNELS = {_lib.SEER_GEMM_REDUCE_PLAIN: "_ZN12_GLOBAL__N_125seer_splitk_reduce_kernelE14seer_gemm_desc",
                  _lib.SEER_GEMM_REDUCE_COLSUM: "_ZN12_GLOBAL__N_132seer_splitk_reduce_colsum_kernelE14seer_gemm_desc",
                  _lib.SEER_GEMM_REDUCE_COLSUM_FX64: "_ZN12_GLOBAL__N_128seer_splitk_reduce_fx_kernelILi64ELi16ELi4EEEv14seer_gemm_desc",
                  _lib.SEER_GEMM_REDUCE_COLSUM_FX32: "_ZN12_GLOBAL__N_128seer_splitk_reduce_fx_kernelILi32ELi32ELi1EEEv14seer_gemm_desc"}

# the kernel symbols of the tile kernel and the reduce pass in a device assembly file
KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S*(?:seer_gemm_kernel|seer_splitk_reduce)\S*)", re.M)


def tile_kernel_name(bm, bn, conv, geglu, split, ns, wm, wn, f16):
    b = lambda v: f"Lb{int(bool(v))}E"
    return (f"_ZN12_GLOBAL__N_116seer_gemm_kernelILi{bm}ELi{bn}E{b(conv)}{b(geglu)}{b(split)}Li{ns}ELi{wm}ELi{wn}E{b(f16)}"
            "EEv14seer_gemm_desc")


def cases():
    """the case list: dicts of id, tile code, f16, form ("plain" | "geglu" | "conv"), M / N / K (conv: Cin), splits, reduce
    (SEER_GEMM_REDUCE_*), and `kernels`, the symbols the launch runs"""
    out = []
    for code, name, bm, bn, ns, wm, wn, may_split in TILES:
        for f16 in (False, True):
            def add(tag, form, m, n, k, splits=1, reduce=0):
                ks = [tile_kernel_name(bm, bn, form == "conv", form == "geglu", splits > 1, ns, wm, wn, f16)]
                if splits > 1:
                    ks.append(REDUCE_KERNELS[reduce])
                out.append(dict(id=f"{name}-{'f16' if f16 else 'bf16'}-{tag}", tile=code, f16=f16, form=form, M=m, N=n, K=k,
                                splits=splits, reduce=reduce, kernels=ks))
            k = 64 * (max(ns, 2) + 1)
            add("plain", "plain", bm + 16, bn + 32, k)
            if (bn // 32) % 2 == 0:
                add("geglu", "geglu", bm + 16, bn + 32, k)
            add("conv", "conv", 400, bn + 32, 64)
            if may_split:
                add("plain_s2", "plain", bm + 16, bn + 32, 2 * k, 2, _lib.SEER_GEMM_REDUCE_PLAIN)
                add("conv_s2", "conv", 400, bn + 32, 128, 2, _lib.SEER_GEMM_REDUCE_PLAIN)
                add("plain_s2_cs", "plain", bm + 16, bn + 32, 2 * k, 2, _lib.SEER_GEMM_REDUCE_COLSUM)
                add("conv_s2_cs", "conv", 400, bn + 32, 128, 2, _lib.SEER_GEMM_REDUCE_COLSUM)
                add("plain_s2_fx", "plain", bm + 32, bn + 32, 2 * k, 2, _lib.SEER_GEMM_REDUCE_COLSUM_FX32)
                if name == "G64x64_3" and not f16:
                    add("fx64", "plain", 1024, 64, 256, 2, _lib.SEER_GEMM_REDUCE_COLSUM_FX64)
    return out


def expected_plan(case):
    """the five words of seer_gemm_plan a case asks for: status, kernel, tile, K slices, reduce pass"""
    split = case["splits"] > 1
    return [0, _lib.SEER_GEMM_KERNEL_SPLITK if split else _lib.SEER_GEMM_KERNEL_TILE, case["tile"], case["splits"], case["reduce"]]


class Launch:
    """the descriptor of one case with its operands on `device`; keeps the tensors alive"""

    def __init__(self, case, device):
        g = torch.Generator().manual_seed(20261020)
        dt = torch.float16 if case["f16"] else torch.bfloat16
        m, n, conv, geglu = case["M"], case["N"], case["form"] == "conv", case["form"] == "geglu"
        cin = case["K"] if conv else 0
        k = 9 * cin if conv else case["K"]
        n_out = n // 2 if geglu else n
        rnd = lambda *shape, scale=1.0: torch.randn(*shape, generator=g) * scale
        self.a = rnd(m, cin if conv else k).to(dt).to(device)                 # conv: NHWC [1, 20, 20, Cin]
        self.w = rnd(n, k, scale=k ** -0.5).to(dt).to(device)
        self.bias = rnd(n).to(device)
        self.res = None if conv else rnd(m, n_out).to(dt).to(device)
        self.c = torch.zeros(m, n_out, dtype=dt, device=device)
        d = self.desc = _lib.GemmDesc()
        d.A, d.W, d.bias, d.C = self.a.data_ptr(), self.w.data_ptr(), self.bias.data_ptr(), self.c.data_ptr()
        d.M, d.N, d.K, d.ldc = m, n, k, n_out
        d.epilogue = (_lib.SEER_EPI_F16 if case["f16"] else 0) | (_lib.SEER_EPI_GEGLU if geglu else 0)
        if conv:
            d.mode, d.Hin, d.Win, d.Cin, d.Hout, d.Wout, d.stride = _lib.SEER_GEMM_CONV3X3, 20, 20, cin, 20, 20, 1
        else:
            d.mode, d.lda, d.residual, d.ldr = _lib.SEER_GEMM_PLAIN, k, self.res.data_ptr(), n_out
        d.tile, d.splits = case["tile"], case["splits"]
        self.sums = None
        if case["splits"] > 1:
            self.ws = torch.zeros(case["splits"] * m * n, dtype=torch.float32, device=device)
            d.workspace, d.workspace_bytes = self.ws.data_ptr(), self.ws.numel() * 4
            if case["reduce"] == _lib.SEER_GEMM_REDUCE_COLSUM:
                self.sums = torch.zeros((m + 3) // 4 * n * 2, dtype=torch.float32, device=device)      # 4-row strips below 2048 rows
                d.colsum = self.sums.data_ptr()
            elif case["reduce"] in (_lib.SEER_GEMM_REDUCE_COLSUM_FX64, _lib.SEER_GEMM_REDUCE_COLSUM_FX32):
                self.sums = torch.zeros(2 * n, dtype=torch.int64, device=device)                       # one batch element, one replica
                d.colsum_fx, d.colsum_fx_rows, d.colsum_fx_reps = self.sums.data_ptr(), m, 1

    def plan(self, lib):
        out = (C.c_int32 * 5)()
        assert lib.seer_gemm_plan(C.byref(self.desc), out) == 0
        return list(out)

    def run(self, lib):
        """launch, wait, and return the digest of the outputs"""
        _lib.check(lib.seer_gemm_bf16(C.byref(self.desc), None), "seer_gemm_bf16")
        torch.cuda.synchronize()
        h = hashlib.sha256(self.c.cpu().view(torch.int16).numpy().tobytes())
        if self.sums is not None:
            h.update(self.sums.cpu().numpy().tobytes())
        return h.hexdigest()


def plan_256(lib, tile):
    """the five words of seer_gemm_plan for a plain 256 x 256 x 256 descriptor that asks for `tile` (fake aligned addresses)"""
    d = _lib.GemmDesc()
    d.A, d.W, d.C = 0x10000, 0x20000, 0x30000
    d.M = d.N = d.K = d.lda = d.ldc = 256
    d.mode, d.tile = _lib.SEER_GEMM_PLAIN, tile
    out = (C.c_int32 * 5)()
    assert lib.seer_gemm_plan(C.byref(d), out) == 0
    return list(out)
