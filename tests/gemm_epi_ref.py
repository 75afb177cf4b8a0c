"""Float64 references, exact constructions and the case tables for the EPILOGUES of the three kernels that run almost every launch of a
denoising step: the tile kernel (csrc/gemm_tile_kernel.h, the 18 rows of csrc/gemm_tiles.h, each also as GEGLU / conv / split form), its
split-K second pass (csrc/gemm_reduce.hip, three reduce kernels) and the weight-stationary kernel (csrc/gemm_ws.hip).  Plain torch on
whatever device the operands live; the library is never imported and nothing here comes from a kernel's output.  Used by
tests/test_gpu_gemm_epi_matrix.py (the kernels) and tests/test_gemm_epi_ref_cpu.py (preconditions, bodies, mutation table; no GPU).

The epilogue, in the order of include/seer_hip.h and of both bodies of the tile kernel (tests/t320_ref.py::epilogue, re-used):
    [folded LayerNorm: rstd * (acc - mean * wsum)]; + bias[n]; GEGLU val * gelu(gate); + rowvec[m / rows_per_batch][n]; SiLU or
    quick-GELU; rotary on n < rot_cols; * col_scale on n < col_scale_cols; + residual[m][n]; row statistics (sum, sum of squares) * 2^24
    of the fp32 values; then ONE round-to-nearest-even to the storage type -- or none (fp32 output) -- row-major or transposed.

WHERE THE KERNELS ROUND (the emulation of Part 2 rounds there and nowhere else):
    1. the operands are stored in 16 bits (A, A2, W, the residual; bias, row vector, rotary table and wsum are stored fp32 operands);
    2. W' = gamma (.) W is rounded to 16 bits BEFORE wsum is summed (fp32) from it;
    3. the row statistics are taken from the producer's fp32 values before ITS 16-bit store, as integers at 2^24;
    4. mean and variance come from those integer totals in double; rstd and mean * rstd are cast to fp32;
    5. one 16-bit store of the result.
SiLU and quick-GELU evaluate expf in fp32: their allowance adds 2x the error of a float32 CPU evaluation of the same formula
(f32_activation), as tests/attn_fwd_ref.py::f32_intrinsics does for the attention kernels.

A problem is a dict of float64 operands: the keys of t320_ref.gemm() / conv() plus silu, qgelu, ln (dict: stats int64 [M, 2], wsum, eps).
`mut` applies one of MUTATIONS at the geometry of the tile under test; a reference returns None where it does not apply."""
import torch

from tests import t320_ref as T
from tests.t320_ref import (colsum_fx, colsum_tiles, conv, epilogue, exact_conv, exact_gemm, interleave_order, r16,  # noqa: F401
                            random_problem, trunc16)
from tests.test_gpu_f16_matrix import _ints

f16, bf16, f32, f64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
BK, LN_SHIFT = 64, 24                                   # csrc/gemm_tiles.h; SEER_LN_FX_SHIFT (include/seer_hip.h)
K_TILE, K_SPLITK, K_WS = 1, 2, 3                        # SEER_GEMM_KERNEL_*
RED_PLAIN, RED_COLSUM, RED_FX64, RED_FX32 = 1, 2, 3, 4  # SEER_GEMM_REDUCE_*
WS, INVARIANT = 19, 23                                  # SEER_TILE_WS, SEER_TILE_AUTO_INVARIANT

# code -> (name, BM, BN, NS, WM, WN, split form), read off csrc/gemm_tiles.h (tests/test_gemm_epi_ref_cpu.py compares with the header)
TILES = {1: ("128x128", 128, 128, 0, 2, 2, False), 3: ("128x64", 128, 64, 0, 2, 2, False), 2: ("64x64", 64, 64, 0, 2, 2, True),
         5: ("G128x128_2", 128, 128, 2, 2, 2, True), 6: ("G128x128_3", 128, 128, 3, 2, 2, False), 7: ("G128x64_3", 128, 64, 3, 2, 2, False),
         8: ("G64x64_3", 64, 64, 3, 2, 2, True), 9: ("G64x64_4", 64, 64, 4, 2, 2, False), 10: ("G64x64_5", 64, 64, 5, 2, 2, False),
         11: ("G128x64_4", 128, 64, 4, 2, 2, False), 12: ("G128x160_2", 128, 160, 2, 2, 2, False), 13: ("G64x160_3", 64, 160, 3, 2, 2, False),
         14: ("G256x128_2", 256, 128, 2, 4, 2, False), 15: ("G256x64_3", 256, 64, 3, 4, 2, False), 21: ("G256x256_2", 256, 256, 2, 2, 4, False),
         16: ("G96x160_2", 96, 160, 2, 2, 2, True), 17: ("G96x160_3", 96, 160, 3, 2, 2, False), 18: ("G96x128_2", 96, 128, 2, 2, 2, False)}
REPRESENTATIVE = (2, 5, 12, 16, 14, 21)                 # one tile per epilogue class (the table of the issue / profiles/gemm_epi_matrix.md)
SPLIT_TILES = (2, 5, 8, 16)
MUTATIONS = ["silu_before_bias", "ln_wsum_wrong_quad", "ln_mean_from_neighbour_row", "rowstat_after_rounding", "rowstat_ragged_row_counted",
             "reduce_slice_order_irrelevant_but_slice_dropped", "trans_out_ld_is_N", "unstaged_tail_quad_skipped", "ws_colscale_whole_wave",
             "ws_panel_tail_from_previous_panel", "activation_dropped", "silu_qgelu_exchanged", "activation_after_colscale"]


# ------------------------------------------------------------------------------------------- the tile's classes, restated from the kernel
def shape_of(tile):
    name, BM, BN, NS, WM, WN, may_split = TILES[tile]
    WTM, WTN = BM // WM, BN // WN
    pp8 = WM == 2 and WN == 4 and BM == 256 and BN == 256
    return dict(name=name, BM=BM, BN=BN, NS=NS, WM=WM, WN=WN, WTM=WTM, WTN=WTN, TM=WTM // 16, TN=WTN // 16, PP8=pp8, NT=64 * WM * WN,
                geglu_ok=(BN // 32) % 2 == 0, may_split=may_split)


def ln_ok(tile):
    """TileShape::ln_ok (csrc/gemm_tiles.h): the (mean * rstd, rstd) pairs of the BM rows fit behind the staged C tile and the scratch"""
    s = shape_of(tile)
    stage_bytes = (s["BM"] + s["BN"]) * BK * 2
    ring = (2 if s["NS"] == 0 else s["NS"]) * stage_bytes
    cswz = s["BM"] * (s["BN"] * 2 + 16) > 2 * stage_bytes
    cpitch = s["BN"] * 2 + (0 if cswz else 16)
    return (not s["PP8"]) and s["BM"] <= s["NT"] and s["BM"] * cpitch + 4096 + s["BM"] * 8 <= ring


def geom_of(tile, K=320):
    """t320_ref's mutation geometry for a tile code (or the weight-stationary kernel: a wave owns 64 columns at K = 320, 32 at 640)"""
    if tile == WS:
        cw = 64 if K == 320 else 32
        return dict(BM=128, BN=8 * cw, WTM=16, wave_cols=(cw, 2 * cw), frag=(0, cw + 16))
    s = shape_of(tile)
    return dict(BM=s["BM"], BN=s["BN"], WTM=s["WTM"], wave_cols=(s["WTN"], 2 * s["WTN"]), frag=(16, s["WTN"] + min(48, s["WTN"] - 16)))


def preload_class(tile, geglu=False, split=False):
    """BIAS_PRE / RV_PRE / RES_PRE of gemm_tile_kernel.h from BM, BN, WM, WN: which epilogue loads are issued before the K loop"""
    s = shape_of(tile)
    return dict(BIAS_PRE=not split and s["TN"] <= 4 and not s["PP8"], RV_PRE=not split and not geglu and s["TN"] <= 4 and not s["PP8"],
                RES_PRE=not geglu and not split and s["TM"] * s["TN"] <= 16)


def n_out_of(spec):
    return spec["N"] // 2 if spec.get("geglu") else spec["N"]


def staged(spec):
    """the kernel's `staged`: a 16-bit row-major output with ldc % 8 == 0, N % 8 (GEGLU: 16) == 0 and a 16-byte aligned base.  The GPU file
    puts the output at column 8 (n_off 4: column 4) of a buffer n_out + 16 columns wide: ldc % 8 == n_out % 8"""
    return (not spec.get("f32") and not spec.get("trans") and n_out_of(spec) % 8 == 0 and spec["N"] % (16 if spec.get("geglu") else 8) == 0
            and not spec.get("n_off"))


def body_of(spec, tile, m0=0, n0=0):
    """("fast" | "general", preload class) of the block whose first row / GEMM column is (m0, n0): the kernel's `fast_epi`, restated.
    A split form has no epilogue of its own ("reduce"): the second pass applies the terms"""
    M, N = spec["M"], spec["N"]
    s, geglu = shape_of(tile), bool(spec.get("geglu"))
    if spec.get("splits", 1) > 1:
        return "reduce", preload_class(tile, geglu, True)
    pre = preload_class(tile, geglu)
    rv_ok = True
    if spec.get("rpb"):
        rv_ok = pre["RV_PRE"] and (min(m0 + s["BM"], M) - 1) // spec["rpb"] == m0 // spec["rpb"]
    fast = (staged(spec) and m0 + s["BM"] <= M and n0 + s["BN"] <= N and not spec.get("silu") and not spec.get("qgelu")
            and spec.get("request", tile) != INVARIANT and not (geglu and (spec.get("rot") or spec.get("cs"))) and rv_ok
            and (not spec.get("res") or pre["RES_PRE"]))
    return ("fast" if fast else "general"), pre


def bodies_of(spec, tile):
    """the set of bodies the blocks of one launch take"""
    s = shape_of(tile)
    return {body_of(spec, tile, m0, n0)[0] for m0 in range(0, spec["M"], s["BM"]) for n0 in range(0, spec["N"], s["BN"])}


def reachable(term, tile):
    """the bodies a launch with `term` can take on `tile` at all (the compile-time classes decide: a row vector or a residual that has no
    preload, and SiLU / quick-GELU, only ever see the general body; unstaged and fp32 / transposed output likewise)"""
    pre = preload_class(tile, term == "geglu")
    if (term == "geglu" and not shape_of(tile)["geglu_ok"]) or (term == "rowstat" and not ln_ok(tile)):
        return set()                                     # the tile has no such form
    if term in ("silu", "qgelu", "f32", "trans", "unstaged") or (term == "rpb" and not pre["RV_PRE"]) or (term == "res" and not pre["RES_PRE"]):
        return {"general"}
    return {"fast", "general"}


def planned(spec):
    """the plan [status, kernel, tile, K slices, reduce pass] a case is MEANT to get (gemm.hip's rules for a tile asked for by name)"""
    tile, S = spec["tile"], spec.get("splits", 1)
    nk = (9 * spec["Ci"] if "n" in spec else spec["K"]) // BK
    if tile == WS:
        # the tile word: what AUTO would run should the launch hand back (it never does).  resolve_tile() on the shapes of WS_EXACT: no
        # grid of 128-row tiles reaches 200 tiles and the K loop has fewer than 12 tiles -- the register-staged 64 x 64 tile
        assert -(-spec["M"] // 128) * -(-spec["N"] // 64) < 200 and nk < 12
        return [0, K_WS, 2, 1, 0]
    if tile == INVARIANT:
        return [0, K_TILE, spec["runs"], 1, 0]
    can = S > 1 and TILES[tile][6] and not (spec.get("geglu") or spec.get("trans") or spec.get("rot") or spec.get("batch", 1) > 1
                                             or spec.get("rowstat") or spec.get("ln") or spec.get("up"))
    if not can:
        return [0, K_TILE, tile, 1, 0]
    M = spec["M"] if "M" in spec else None
    red = {None: RED_PLAIN, "tiles": RED_COLSUM, "fx": RED_FX64 if (M or 0) >= 1024 else RED_FX32}[spec.get("gets", spec.get("colsum"))]
    return [0, K_SPLITK, tile, min(S, nk), red]


# ------------------------------------------------------------------------------------------- references
def f32_activation(pre_act64, kind):
    """the same formula evaluated in float32 on the CPU: x / (1 + exp(-c x)), c = 1 (SiLU) or 1.702 (quick-GELU)"""
    x = pre_act64.to(f32)
    c = torch.tensor(1.0 if kind == "silu" else 1.702, dtype=f32, device=x.device)
    return (x / (1.0 + torch.exp(-(c * x)))).to(f64)


def rowstat_of(pre64, after_rounding=None):
    """[M, 2] int64: (round(sum * 2^24), round(sum of squares * 2^24)) of the fp32 values before the 16-bit store.  The kernel adds one
    pair per (row, wave column); the totals are what is compared -- equal on integers, whatever the split into wave columns"""
    v = (pre64 if after_rounding is None else after_rounding).to(f32).to(f64)
    return torch.stack([(v.sum(1) * (1 << LN_SHIFT)).round(), (v.pow(2).sum(1) * (1 << LN_SHIFT)).round()], 1).to(torch.int64)


def ln_moments(stats, K, eps):
    """(mean * rstd, rstd) as the consumer forms them: E[x^2] - mean^2 in double on the integer totals, rstd cast to fp32, the product
    (float) mean * rstd in fp32"""
    k = 1.0 / (float(1 << LN_SHIFT) * K)
    mean = stats[:, 0].to(f64) * k
    var = (stats[:, 1].to(f64) * k - mean * mean).clamp_min(0)
    r = (1.0 / (var + eps).sqrt()).to(f32)
    return (mean.to(f32) * r).to(f64), r.to(f64)


def fold(w64, gamma64, beta64, bias64, dt):
    """ops.fold_layernorm restated: W' = round16(fp32(W) * fp32(gamma)), wsum = fp32 row sums of W' AS ROUNDED, b' = W beta + b"""
    wp = (w64.to(f32) * gamma64.to(f32)[None, :]).to(dt)
    bp = w64.to(f32) @ beta64.to(f32)
    return wp.to(f64), wp.float().sum(1).to(f64), (bp if bias64 is None else bp + bias64.to(f32)).to(f64)


def gemm(p, mut=None, exact=False, tile=5, store=bf16):
    """t320_ref.gemm at the geometry of `tile` with the terms that kernel does not have.  p adds: silu / qgelu, ln (dict stats, wsum,
    eps -- p["w"] is then W' and p["bias"] b'), f32 (no store rounding), trans ([N, M] output with leading dimension ldc), rowstat.
    Returns dict(pre, out[, rowstat]) or None where `mut` does not apply"""
    geom = geom_of(tile, p["w"].shape[1])
    M, N, K = p["a"].shape[0], p["w"].shape[0], p["w"].shape[1]
    q = dict(p)
    tmut = mut if mut in T.MUTATIONS else None
    if mut == "silu_before_bias":
        if not ((p.get("silu") or p.get("qgelu")) and p.get("bias") is not None):
            return None
        q["bias"] = None
    act = "silu" if p.get("silu") else "qgelu" if p.get("qgelu") else None
    if mut in ("activation_dropped", "silu_qgelu_exchanged", "activation_after_colscale"):
        if act is None or (mut == "activation_after_colscale" and (p.get("col_scale") is None or p.get("rot") is not None)):
            return None
        q.update(silu=False, qgelu=False)
        if mut == "silu_qgelu_exchanged":
            q["qgelu" if act == "silu" else "silu"] = True
        if mut == "activation_after_colscale":
            q["res"] = None                                                # activation(x * scale) + residual, below
    ln = p.get("ln")
    if mut in ("ln_wsum_wrong_quad", "ln_mean_from_neighbour_row") and ln is None:
        return None
    A = p["a"] if p.get("a2") is None else torch.cat([p["a"], p["a2"]], 1)
    w = p["w"]
    if mut == "ws_panel_tail_from_previous_panel":
        pw = geom["BN"]
        if tile != WS or N % pw == 0 or N < pw:
            return None
        w = w.clone()
        w[N // pw * pw:] = p["w"][N // pw * pw - pw:N - pw]
        q["w"] = w
    if mut == "reduce_slice_order_irrelevant_but_slice_dropped":
        S = p.get("S", 1)
        if S < 2:
            return None
        k0, k1 = T.slice_bounds(K, S, S - 1)
        q["acc_fix"] = (slice(M - min(4, M), M), -(A[M - min(4, M):, k0:k1] @ w[:, k0:k1].t()))
    if mut == "ws_colscale_whole_wave":
        cw = geom["wave_cols"][0]
        if tile != WS or p.get("col_scale") is None or p["col_scale"][1] % cw == 0:
            return None
        q["col_scale"] = (p["col_scale"][0], -(-p["col_scale"][1] // cw) * cw)
    if ln is not None or q.get("acc_fix") is not None:
        # the terms in front of the bias: done here, the rest by t320_ref.epilogue on an accumulator that already carries them
        acc = A @ w.t()
        if q.get("acc_fix") is not None:
            acc = acc.clone()
            acc[q["acc_fix"][0]] += q["acc_fix"][1]
        if ln is not None:
            mr, r = ln_moments(ln["stats"], K, ln["eps"])
            wsum = ln["wsum"]
            if mut == "ln_wsum_wrong_quad":
                n16 = N // 16 * 16                                         # the lane's neighbour quad inside each whole 16-column fragment
                wsum = torch.cat([wsum[:n16].reshape(-1, 4, 4).roll(1, 1).reshape(-1), wsum[n16:]])
            if mut == "ln_mean_from_neighbour_row":
                mr = mr[torch.arange(M, device=mr.device) ^ 1 if M % 2 == 0 else torch.arange(M, device=mr.device).roll(1)]
            acc = r[:, None] * acc - mr[:, None] * wsum[None, :]
        pre = epilogue(acc, q, tmut, exact and ln is None, geom)
        out = None if pre is None else T._store(pre, q, tmut, geom)
        res = None if out is None else dict(pre=pre, out=out)
    else:
        res = T.gemm(q, tmut, exact, geom)
    if res is None:
        return None
    pre = res["pre"]
    if mut == "silu_before_bias":
        # activation(acc) + bias in place of activation(acc + bias); the case carries bias and the activation alone
        assert all(p.get(k) is None for k in ("rowvec", "rot", "col_scale", "res"))
        pre = pre + p["bias"]
    if mut == "activation_after_colscale":
        assert not p.get("act_exact")
        pre = pre * torch.sigmoid((1.0 if act == "silu" else 1.702) * pre)
        if p.get("res") is not None:
            pre = pre + p["res"]
    out = r16x(pre, store) if not p.get("f32") else pre
    if tmut == "truncating_stores" and not p.get("f32"):
        out = res["out"]
    if tmut == "tile_twice_one_missing":
        out = torch.where(res["out"].isnan(), res["out"], out)
    if mut == "unstaged_tail_quad_skipped":
        n_out = pre.shape[1]
        if n_out % 8 != 4:
            return None
        out = out.clone()
        out[:, n_out - 4:] = float("nan")                                  # the buffer's pre-fill
    r = dict(pre=pre, out=out)
    if p.get("trans"):
        ld = N if mut == "trans_out_ld_is_N" else M
        if mut == "trans_out_ld_is_N" and M == N:
            return None
        flat = torch.full((N * M,), float("nan"), dtype=f64, device=pre.device)
        idx = torch.arange(N, device=pre.device)[:, None] * ld + torch.arange(M, device=pre.device)[None, :]
        ok = idx < flat.numel()
        flat[idx[ok]] = out.t()[ok]
        r["out"], r["pre"] = flat.reshape(N, M), pre.t().contiguous()
    elif mut == "trans_out_ld_is_N":
        return None
    if p.get("rowstat"):
        rs = rowstat_of(pre, out if mut == "rowstat_after_rounding" else None)
        if mut == "rowstat_after_rounding" and torch.equal(rs, rowstat_of(pre)):
            return None
        if mut == "rowstat_ragged_row_counted":
            if M % geom["BM"] == 0:
                return None
            rs = rs.clone()
            rs[M - 1] *= 2                                                 # the clamped row behind the last one adds to it
        r["rowstat"] = rs
    elif mut in ("rowstat_after_rounding", "rowstat_ragged_row_counted"):
        return None
    return r


def r16x(x64, dt):
    return x64.to(dt).to(f64)


# ------------------------------------------------------------------------------------------- the exact constructions (Part 1)
def exact_problem(spec, dev):
    """t320_ref.exact_gemm / exact_conv, and for SiLU / quick-GELU the class where fp32 leaves the formula no choice (t320_ref.epilogue,
    act_exact): the value entering the activation is 0 (whole rows of A are zero, bias and row vector 0 or 24), at least 20 (returned
    unchanged) or at most -104 (negative rows of A: expf overflows, the result is -0) -- the last class is not the identity, so a launch
    that drops its activation differs"""
    if "n" in spec:
        p = exact_conv(spec, dev)
    elif spec.get("silu") or spec.get("qgelu"):
        M, N, K = spec["M"], spec["N"], spec["K"]
        seed = spec.get("seed", 0) * 1000 + M + 7 * N + 13 * K
        A, w = _ints((M, K), dev, seed + 1, 0, 3), _ints((N, K), dev, seed + 2, 1, 3)
        A[::7] = 0.0
        A[1::7, 0] = 3.0                                                   # (no other row is all zero)
        A[3::7] = -_ints((len(range(3, M, 7)), K), dev, seed + 6, 2, 3)    # rows whose products sum to -2 K or below: the third class
        p = dict(a=A, w=w, S=1, act_exact=True)
        if spec.get("bias"):
            p["bias"] = _ints((N,), dev, seed + 3, 0, 1) * 24
        if spec.get("rpb"):
            p["rows_per_batch"], p["rowvec"] = spec["rpb"], _ints((-(-M // spec["rpb"]), N), dev, seed + 4, 0, 1) * 24
        if spec.get("cs"):
            p["col_scale"] = (0.5, spec["cs"])
        if spec.get("res"):
            p["res"] = _ints((M, N), dev, seed + 5, -8, 8)
        p["silu" if spec.get("silu") else "qgelu"] = True
    else:
        p = exact_gemm(spec, dev)
    if spec.get("k1") and p.get("a2") is None:                             # (the constructions t320_ref does not split)
        p["a"], p["a2"] = p["a"][:, :spec["k1"]].contiguous(), p["a"][:, spec["k1"]:].contiguous()
    p["S"] = planned(spec)[3]
    for k in ("f32", "trans", "rowstat"):
        if spec.get(k):
            p[k] = True
    return p


def exact_reference(spec, p):
    """the reference of a Part 1 case with its preconditions asserted: exact in fp32, |C| < 60000, activation class"""
    tile = spec.get("runs", spec["tile"])
    store = f16 if spec.get("dt") == "f16" else bf16
    if "n" in spec:
        r = conv(p, exact=True, geom=geom_of(tile))
        r = dict(pre=r["pre"], out=r16x(r["pre"], store))
    else:
        # (SiLU / quick-GELU: the class is asserted where the activation is applied, t320_ref.epilogue)
        r = gemm(p, exact=not (p.get("silu") or p.get("qgelu")), tile=tile, store=store)
    assert torch.equal(r["pre"].to(f32).to(f64), r["pre"]), f"{case_id(spec)}: not exact in fp32"
    assert float(r["pre"].abs().max()) < 60000, case_id(spec)
    if spec.get("rowstat") or spec.get("colsum"):
        assert float(r["pre"].pow(2).sum(-1).max()) < 2 ** 24 and float(r["pre"].pow(2).sum(0).max()) < 2 ** 24, "sums of squares exact in fp32"
    if spec.get("colsum"):
        assert torch.equal(r["out"], r["pre"]), "column sums: the stored value is the fp32 value"
    return r


def _c(tile, M, N, K, **kw):
    return dict(tile=tile, M=M, N=N, K=K, **kw)


def _v(tile, n, H, W, Co, **kw):
    return dict(tile=tile, n=n, H=H, W=W, Ci=64, Co=Co, **kw)


ALL = dict(bias=True, rpb=96, res="lds")


def _cs_inside(BN, N):
    """a column-scale count that ends inside the second column tile"""
    return min(BN + 20, N - 4)


def _rep_cases(t):
    """the edges of every term on one representative tile"""
    s = shape_of(t)
    BM, BN = s["BM"], s["BN"]
    Mr, Nr, K = 2 * BM + 37, 2 * BN + 8, 192
    allc = dict(ALL, cs=_cs_inside(BN, Nr))
    out = [_c(t, Mr, Nr, K, **terms) for terms in (
        dict(bias=True), dict(rpb=96), dict(rpb=100), dict(rpb=BM), dict(res="lds"), dict(res="ldr4"), dict(res="base8"),
        dict(cs=min(164, Nr - 4) // 4 * 4), dict(cs=_cs_inside(BN, Nr)), allc, dict(allc, dt="f16"), dict(allc, k1=64), dict(allc, f32=True),
        dict(allc, f32=True, k1=128, dt="f16"))]
    out += [_c(t, 2 * BM, 2 * BN, K, **terms) for terms in (dict(bias=True), dict(rpb=BM), dict(res="lds"), dict(cs=BN + 20), dict(allc, rpb=BM), dict(allc, rpb=BM, dt="f16"))]
    alln = dict(allc, cs=BN + 4)                                           # (the narrow shapes: the count still ends inside the second tile)
    out += [_c(t, M, BN + 8, 128, **alln) for M in (1, BM - 1, BM, BM + 1)]
    out += [_c(t, BM + 37, BN + 4, 128, **dict(allc, cs=BN)), _c(t, BM + 37, 68 if BN == 64 else 132, 128, bias=True, res="lds", cs=36),
            _c(t, BM + 37, BN + 8, 128, n_off=4, **alln)]
    # rotary from a dyadic table: heads of 40 / 80 / 160 with 32 rotated channels, 96 tokens (wraps inside a tile), offset 16, a column
    # count that ends inside a column tile; the column scale on the first head
    for hd, cols in ((40, 200), (80, 240), (160, 480 if BN == 160 else 160)):
        N = max(Nr, cols + 8)
        out.append(_c(t, Mr, N, K, rot=(hd, 32, 96, 16, cols), cs=hd, **({"k1": 64} if hd == 40 else {})))
        out.append(_c(t, 2 * BM, -(-max(2 * BN, cols) // BN) * BN, K, rot=(hd, 32, 96, 16, cols), cs=hd))
    if s["geglu_ok"]:
        out += [_c(t, Mr, 2 * BN + 32, K, geglu=True), _c(t, 2 * BM, 2 * BN, K, geglu=True), _c(t, Mr, 2 * BN + 32, K, geglu=True, k1=64, dt="f16")]
    out += [_c(t, Mr, Nr, K, bias=True, **{act: True}) for act in ("silu", "qgelu")]
    out += [_c(t, Mr, Nr, K, silu=True, k1=64, **allc), _c(t, 2 * BM, 2 * BN, K, qgelu=True, bias=True)]
    out += [_c(t, BM + 37, BN + 8, 128, trans=True, batch=b, bias=True, cs=20) for b in (1, 2)]
    # rounding: sums near 12 000, where the 16-bit store rounds most elements
    out += [_c(t, BM + 37, BN + 8, 768, big=True), _c(t, BM + 37, BN + 8, 768, big=True, dt="f16")]
    if ln_ok(t):
        out += [_c(t, Mr, Nr, K, sums=True, rowstat=True, **terms) for terms in (dict(), dict(bias=True, res="lds"))]
        # (K = 512 of [-3, 3] x [-3, 3]: some |C| pass 256, where the bf16 store rounds -- statistics taken AFTER the store would differ)
        out += [_c(t, BM + 37, BN + 8, 512, rowstat=True, bias=True, res="lds")]
        out += [_c(t, 2 * BM, 2 * BN, K, sums=True, rowstat=True, bias=True, res="lds")]
    return out


GEMM_EXACT = [c for t in REPRESENTATIVE for c in _rep_cases(t)]
# every tile code: bias + row vector + residual + column scale at 2 BM + 37 rows, N = 2 BN + 8, K = 192
GEMM_EXACT += [_c(t, 2 * TILES[t][1] + 37, 2 * TILES[t][2] + 8, 192, **dict(ALL, cs=_cs_inside(TILES[t][2], 2 * TILES[t][2] + 8)))
               for t in TILES if t not in REPRESENTATIVE]
GEMM_EXACT += [_c(21, 293, 2 * 256 + 32, 192, f32=True, trans=True, batch=1, bias=True, cs=20)]
# ---- split-K through the three reduce kernels: the terms alone and together, both slice counts, both storage types for the together case
_SPLIT_TERMS = (dict(bias=True), dict(rpb=96), dict(res="ldr4"), dict(cs=36), dict(silu=True, bias=True), dict(qgelu=True, bias=True),
                dict(f32=True, bias=True), dict(ALL, cs=36), dict(ALL, cs=36, dt="f16"), dict(ALL, cs=36, silu=True), dict(ALL, cs=36, f32=True, k1=64))
SPLIT_EXACT = [_c(t, TILES[t][1] + 37, TILES[t][2] + 8, 256, splits=S, **terms) for t in SPLIT_TILES for S in (2, 3) for terms in _SPLIT_TERMS
               if S == 2 or t in (2, 16)]
SPLIT_EXACT += [_c(t, 101, 68, 256, splits=2, **dict(ALL, cs=36)) for t in (2, 16)]
SPLIT_EXACT += [_c(t, TILES[t][1] + 37, TILES[t][2] + 8, 768, splits=3, big=True, **kw) for t in SPLIT_TILES for kw in ({}, dict(dt="f16"))]
# column sums of the STORED values with the terms applied: 4-row strips (M < 2048; a ragged last strip is admitted), 16-row strips from
# 2048 rows, the accumulating pass on 32-row blocks below 1024 rows and 64-row blocks from there
SUMS_TERMS = dict(bias=True, rpb=96, res="lds", sums=True)
SPLIT_SUMS = ([_c(t, 192, TILES[t][2] + 8, 256, splits=2, colsum=f, **SUMS_TERMS) for t in SPLIT_TILES for f in ("tiles", "fx")]
              + [_c(8, 192, 72, 256, splits=2, colsum=f, dt="f16", **SUMS_TERMS) for f in ("tiles", "fx")]
              # a partial that would straddle two batch elements is not admitted (decided on the host before the launch): 99 rows per
              # element leave no 4-row strips; 104 / 560 rows per element leave no 32- / 64-row blocks, the per-strip form runs instead
              + [_c(16, 198, 68, 256, splits=3, colsum="tiles", gets=None, **dict(SUMS_TERMS, rpb=99)),
                 _c(8, 208, 72, 256, splits=2, colsum="fx", gets="tiles", **dict(SUMS_TERMS, rpb=104)),
                 _c(2, 1024 + 96, 72, 128, splits=2, colsum="fx", gets="tiles", **dict(SUMS_TERMS, rpb=560)),
                 _c(8, 2048 + 32, 72, 128, splits=2, colsum="tiles", **dict(SUMS_TERMS, rpb=1040)),  # 16-row strips
                 _c(8, 960, 72, 128, splits=2, colsum="fx", **dict(SUMS_TERMS, rpb=480)),            # 32-row blocks
                 _c(8, 192, 68, 256, splits=2, colsum="tiles", gets=None, **SUMS_TERMS),            # N % 8 == 4: the sums need a staged-width output
                 _c(2, 1024, 72, 128, splits=2, colsum="fx", **dict(SUMS_TERMS, rpb=512)),           # 64-row blocks
                 _c(2, 1024 + 128, 72, 128, splits=2, colsum="fx", cs=36, **dict(SUMS_TERMS, rpb=576))])
# ---- the weight-stationary kernel: K = 320 (a wave owns 64 columns, a panel 512) and 640 (32 / 256)
WS_EXACT = ([_c(WS, M, N, K, **terms) for K, N, cs2 in ((320, 520, 516), (640, 264, 260)) for M in (1024, 1061) for terms in (
                 dict(bias=True), dict(bias=True, cs=164), dict(bias=True, cs=cs2), dict(bias=True, cs=164, k1=64), dict(bias=True, cs=164, dt="f16"))]
            + [_c(WS, M, N, K, geglu=True, **kw) for K, N in ((320, 576), (640, 320)) for M, kw in ((1024, {}), (1061, dict(dt="f16")), (1061, dict(k1=64)))])
# ---- the layout-invariant request keeps every tile on the general body: N = 320, K = 320 runs on G96x160_2
INV_EXACT = [_c(INVARIANT, M, 320, 320, runs=16, request=INVARIANT, **dict(ALL, cs=164)) for M in (192, 384)]
# ---- convs on the tile kernel: images whose boundaries fall inside a tile
CONV_EXACT = ([_v(t, 3, H, W, TILES[t][2] + 8, stride=st, pad_after=pa, bias=True, rpb=rpb, res="lds")
               for t in (16, 2) for (H, W, st, pa, rpb) in ((6, 10, 1, False, 60), (6, 10, 2, False, 15), (16, 24, 2, True, 96))]
              + [_v(t, 3, 6, 10, TILES[t][2] + 8, up=True, bias=True, cs=36) for t in (16, 2)])


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if case_id(c) not in seen:
            seen.add(case_id(c))
            out.append(c)
    return out


def case_id(s):
    name = {WS: "WS", INVARIANT: "INV"}.get(s["tile"]) or TILES[s["tile"]][0]
    tail = "".join(f"-{k}{'' if s[k] is True else '_' + str(s[k]).replace(' ', '')}" for k in (
        "bias", "rpb", "cs", "res", "rot", "big", "sums", "geglu", "silu", "qgelu", "f32", "trans", "batch", "k1", "n_off", "rowstat", "colsum", "dt", "stride", "pad_after", "up") if s.get(k))
    if "gets" in s:
        tail += f"-gets_{s['gets']}"
    if "n" in s:
        return f"{name}-conv-n{s['n']}-{s['H']}x{s['W']}-co{s['Co']}-S{s.get('splits', 1)}{tail}"
    return f"{name}-{s['M']}x{s['N']}x{s['K']}-S{s.get('splits', 1)}{tail}"


GEMM_EXACT, SPLIT_EXACT = _unique(GEMM_EXACT), _unique(SPLIT_EXACT)
for _i, _s in enumerate(GEMM_EXACT + SPLIT_EXACT + SPLIT_SUMS + WS_EXACT + INV_EXACT + CONV_EXACT):
    _s["seed"] = _i + 1
ALL_EXACT = GEMM_EXACT + SPLIT_EXACT + SPLIT_SUMS + WS_EXACT + INV_EXACT + CONV_EXACT
assert len({case_id(_s) for _s in ALL_EXACT}) == len(ALL_EXACT)


# ------------------------------------------------------------------------------------------- Part 3: full tiles against a ragged launch
def bodies_cases():
    """Part 3: 2 BM full rows (the fast body where the class has one).  The GPU file launches the same operands again into an output at
    column 4 (unstaged: every block on the general body) and launches the first 2 BM - 27 rows alone (the second row tile ragged: the
    general body, staged).  Without the LayerNorm term the bodies must give the same bits"""
    out = []
    for t in REPRESENTATIVE:
        BM, BN = TILES[t][1], TILES[t][2]
        for terms in (dict(ALL, rpb=BM, cs=BN + 20), dict(bias=True, rot=(40, 32, 96, 16, 200), cs=40)):
            N = max(2 * BN, 256)
            out.append(_c(t, 2 * BM, N, 192, seed=77, **terms))
        if shape_of(t)["geglu_ok"]:
            out.append(_c(t, 2 * BM, 2 * BN, 192, seed=78, geglu=True))
    return out


def head_rows(p, M):
    """the problem of the first M rows of p (same operands): what a shorter launch of the same rows computes"""
    q = dict(p)
    for k in ("a", "a2", "res"):
        if p.get(k) is not None:
            q[k] = p[k][:M].contiguous()
    if p.get("rowvec") is not None:
        q["rowvec"] = p["rowvec"][:-(-M // p["rows_per_batch"])].contiguous()
    return q


# ------------------------------------------------------------------------------------------- Part 2: per own row
def _randn(shape, dev, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=f64) * scale).to(dev)


ROWS_TILES = (5, 12, 16, 14)
# (kind, tile, M, amp): full-tile M = 2 BM (fast body) and ragged M = 2 BM + 37 (general body in the last row tile)
ROWS_CASES = ([(kind, t, 2 * TILES[t][1] + r, amp) for kind in ("ln", "ln_rot") for t in ROWS_TILES for r in (0, 37) for amp in (1.0, 4.0)]
              + [("ln_geglu", t, 2 * TILES[t][1] + r, amp) for t in (5, 14) for r in (0, 37) for amp in (1.0, 4.0)]
              + [(kind, t, 2 * TILES[t][1] + 37, amp) for kind in ("silu", "qgelu", "geglu", "rot") for t in (5, 16) for amp in (1.0, 4.0)
                 if not (kind == "geglu" and t == 16)])
LN_K = 320


def batch_rows(M, rows_pb, K, dev, seed, amp):
    """rows of batch element b drawn as N(b, 4^b) x amp: foreign or shifted statistics are an O(1) error in a row"""
    b = (torch.arange(M) // rows_pb).to(f64)[:, None].to(dev)
    return (_randn((M, K), dev, seed) * 2.0 ** b + b) * amp


def producer_problem(tile, M, amp, dev, dt=bf16):
    """the GEMM that leaves the rows AND their statistics: x = a W1^T + b1 + res, res the batch rows, a W1^T N(0, 1) x amp"""
    seed = 17 * M + 1000 * int(amp) + tile
    return dict(a=r16x(_randn((M, 128), dev, seed + 1, amp), dt), w=r16x(_randn((LN_K, 128), dev, seed + 2, 128 ** -0.5), dt),
                bias=_randn((LN_K,), dev, seed + 3, 0.1).to(f32).to(f64), res=r16x(batch_rows(M, 100, LN_K, dev, seed + 4, amp), dt), rowstat=True)


def consumer_problem(kind, tile, M, amp, x16, stats, dev, dt=bf16, make_table=None, folded=None):
    """kind ln: norm -> a projection (N = 2 BN + 8); ln_geglu: norm3 -> ff.net.0; ln_rot: norm1 -> q | k | v with rotary on two thirds and
    the q prescale.  Returns (problem for gemm() -- W', b', wsum as stored operands --, dict of the unfolded float64 operands)"""
    seed = 23 * M + 1000 * int(amp) + tile + {"ln": 0, "ln_geglu": 300, "ln_rot": 600}[kind]
    BN = TILES[tile][2]
    N = {"ln": 2 * BN + 8, "ln_geglu": 2 * BN + 64, "ln_rot": 480}[kind]
    w = r16x(_randn((N, LN_K), dev, seed + 1, LN_K ** -0.5), dt)
    gamma = (1.0 + 0.2 * _randn((LN_K,), dev, seed + 2)).to(f32).to(f64)
    beta = (0.2 * _randn((LN_K,), dev, seed + 3)).to(f32).to(f64)
    b = _randn((N,), dev, seed + 4, 0.5).to(f32).to(f64)
    wp, wsum, bp = folded(w, gamma, beta, b) if folded is not None else fold(w, gamma, beta, b, dt)
    p = dict(a=x16, w=wp, bias=bp, ln=dict(stats=stats, wsum=wsum, eps=1e-5))
    if kind == "ln_geglu":
        p["geglu"] = True
    if kind == "ln_rot":
        p["rot"] = dict(table=(make_table or T.real_rotary_table)(max(M, 96) + 16, 32, dev), tokens=96, off=16, head_dim=40, rot_dim=32, cols=320)
        p["col_scale"] = (float(torch.tensor(40 ** -0.5 * 1.4426950408889634, dtype=f32)), 160)
    return p, dict(w=w, gamma=gamma, beta=beta, b=b)


def ln_reference(p, plain):
    """the operator in float64 on the stored rows: LayerNorm(x; gamma, beta) W^T + b with W unrounded by gamma, then the epilogue's other
    terms; no rounding anywhere"""
    x = p["a"]
    d = x - x.mean(-1, keepdim=True)
    y = d * (d.pow(2).mean(-1, keepdim=True) + p["ln"]["eps"]).rsqrt() * plain["gamma"] + plain["beta"]
    q = {k: v for k, v in p.items() if k not in ("ln", "bias")}
    return epilogue(y @ plain["w"].t() + plain["b"], q, geom=geom_of(5))


def act_problem(kind, tile, M, amp, dev, make_table=None, dt=bf16):
    """SiLU / quick-GELU behind bias and row vector, GEGLU on N(0, 1) gates, rotary from the real table: N(0, 1) x amp operands"""
    BN = TILES[tile][2]
    seed = 29 * M + 1000 * int(amp) + tile
    if kind in ("geglu", "rot"):
        N = 2 * BN + 64 if kind == "geglu" else 480
        p = random_problem("geglu" if kind == "geglu" else "rotary", M, amp, dev, make_table=make_table, N=N, K=192)
        if kind == "rot":
            p["rot"]["cols"], p["col_scale"] = 320, (p["col_scale"][0], 160)
        return p
    N, K = 2 * BN + 8, 192
    p = dict(a=r16x(_randn((M, K), dev, seed + 1, amp), dt), w=r16x(_randn((N, K), dev, seed + 2, K ** -0.5), dt),
             bias=_randn((N,), dev, seed + 3).to(f32).to(f64), rows_per_batch=100, rowvec=_randn((-(-M // 100), N), dev, seed + 4).to(f32).to(f64))
    p[kind] = True
    return p


def act_f32_error(p, kind, ref_pre):
    """worst row of what the float32 CPU evaluation of the activation moves the result by (its error, times the column scale where one
    follows), as the row criterion measures it"""
    A = p["a"] if p.get("a2") is None else torch.cat([p["a"], p["a2"]], 1)
    v = A @ p["w"].t() + p["bias"] + p["rowvec"][torch.arange(A.shape[0], device=A.device) // p["rows_per_batch"]]
    d = f32_activation(v, kind) - v * torch.sigmoid((1.0 if kind == "silu" else 1.702) * v)
    if p.get("col_scale") is not None:
        d[:, :p["col_scale"][1]] *= p["col_scale"][0]
    return float((d.norm(dim=-1) / ref_pre.norm(dim=-1).clamp_min(T.row_floor(ref_pre))).max())


# SiLU / quick-GELU through the split-K second pass, whose activation code is its own (gemm_reduce.hip, splitk_reduce_quad): N(0, 1) data,
# bias + row vector in front of the activation, column scale + residual behind it, 2 and 3 slices, and the two passes with column sums.
# (kind, tile, M, N, K, slices, column sums): 192 rows = 2 batch elements of 96 (4-row strips, 32-row blocks); 1024 rows: 64-row blocks
ROWS_SPLIT = ([(kind, t, TILES[t][1] + 37, TILES[t][2] + 8, 256, S, None) for kind in ("silu", "qgelu") for t in SPLIT_TILES for S in (2, 3)]
              + [(kind, 8, 192, 72, 256, 2, form) for kind in ("silu", "qgelu") for form in ("tiles", "fx")]
              + [(kind, 2, 1024, 72, 128, 2, "fx") for kind in ("silu", "qgelu")])


def split_act_spec(kind, tile, M, N, K, S, form):
    return dict(tile=tile, M=M, N=N, K=K, splits=S, bias=True, rpb=96 if form is None else M // 2, cs=36, res="lds", colsum=form, seed=0, **{kind: True})


def split_act_problem(kind, tile, M, N, K, S, form, dev, dt=bf16):
    spec = split_act_spec(kind, tile, M, N, K, S, form)
    seed = 37 * M + 11 * N + 100 * S + tile
    p = dict(a=r16x(_randn((M, K), dev, seed + 1), dt), w=r16x(_randn((N, K), dev, seed + 2, K ** -0.5), dt),
             bias=_randn((N,), dev, seed + 3).to(f32).to(f64), rows_per_batch=spec["rpb"],
             rowvec=_randn((-(-M // spec["rpb"]), N), dev, seed + 4).to(f32).to(f64), col_scale=(0.125, 36),
             res=r16x(_randn((M, N), dev, seed + 5), dt), S=min(S, K // BK))
    p[kind] = True
    return spec, p
