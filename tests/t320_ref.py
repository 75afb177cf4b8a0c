"""Float64 references, exact constructions and the case table for the 256 x 320 tile GEMM / conv kernel (csrc/gemm_t320.hip,
SEER_TILE_T256x320, plan kernel SEER_GEMM_KERNEL_T320).  Plain torch on whatever device the operands live; the library is never
imported and nothing here comes from a kernel's output.  Used by tests/test_gpu_t320_matrix.py (the kernel) and
tests/test_t320_ref_cpu.py (the preconditions and the mutation table, no GPU).

    gemm:  C = epi([a | a2] w^T)          conv:  C = epi(conv3x3(x, w))  stride 1 / 2, pad_after_only, or behind a nearest-2x upsample
    epi, in the order of include/seer_hip.h and of the kernel's epilogue:
           + bias[n]; GEGLU val * gelu(gate); + rowvec[m / rows_per_batch][n]; rotary on n < rot_cols; * col_scale on n < col_scale_cols;
           + residual[m][n]; then ONE round-to-nearest-even to bf16.
    column sums: (sum, sum of squares) of the STORED values per 64-row partial (unsplit) or 16-row partial (K slices), per tile
           ([z][partial][N][2] fp32) or accumulated in fixed point ([rep][batch][2][N] int64 at 2^20).

A problem is a dict of float64 operands (keys: see gemm() / conv()).  `mut` applies one of MUTATIONS: the kernel bugs the matrix must
be able to see; a reference returns None where the mutation does not apply to the problem."""
import torch
import torch.nn.functional as Fn

from tests.fused320_ref import (assert_exact_sums, dyadic_table, geglu_interleave_order, gelu64, rotary, row_err,  # noqa: F401
                                row_floor)
from tests.test_gpu_f16_matrix import _exact_pre, _ints

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
BM, BN, BK, FX_SHIFT = 256, 320, 64, 20
# where the mutations sit, for a kernel of another geometry (tests/gemm_epi_ref.py passes its own): the block tile, the rows of a wave
# tile, the columns of the wave whose K step is dropped, and the 16 x 16 fragment (row offset in that wave, columns) of the slice mutations
GEOM = dict(BM=BM, BN=BN, WTM=64, wave_cols=(160, 320), frag=(16, 160 + 48))
T320, KERNEL_T320 = 22, 4            # SEER_TILE_T256x320, SEER_GEMM_KERNEL_T320 (include/seer_hip.h)
MUTATIONS = ["drop_kstep_one_wave", "residual_row_clamped", "slice_last_twice", "slice0_skipped", "rowvec_batch_per_wave_tile",
             "rot_no_modulo", "colscale_whole_fragment", "value_gate_exchanged_16", "pad_after_border_valid", "phases_swapped",
             "a2_read_with_lda", "truncating_stores", "tile_twice_one_missing"]


def r16(x64):
    """one round-to-nearest-even to bf16, back in float64"""
    return x64.to(bf16).to(f64)


def trunc16(x64):
    """the store that drops the low 16 bits of the fp32 value instead of rounding"""
    bits = x64.to(f32).view(torch.int32) & -65536
    return bits.view(f32).to(f64)


def planned_slices(K, splits):
    """the K slices seer_gemm_plan gives an explicit SEER_TILE_T256x320 request (gemm.hip, t320_plan): at most 16, and a slice keeps
    at least four 64-wide K tiles"""
    return 1 if splits <= 1 else max(1, min(splits, K // BK // 4, 16))


def interleave_order(inner, dev):
    """packed GEGLU row p -> row of the natural [value inner | gate inner] matrix: 16 value rows, then their 16 gate rows"""
    p = torch.arange(2 * inner, device=dev)
    order = ((p // 16) % 2) * inner + 16 * (p // 32) + p % 16
    if inner == 1280:
        assert torch.equal(order, geglu_interleave_order(dev))
    return order


def slice_bounds(K, S, s):
    nk = K // BK
    return nk * s // S * BK, nk * (s + 1) // S * BK


# ------------------------------------------------------------------------------------------- the epilogue
def _rot_blocks(v, rot, no_modulo):
    """fused320_ref.rotary on the 320-column blocks below rot_cols where head_dim divides 320; any other width (cols a multiple of
    head_dim) through the same formula on the heads themselves"""
    v = v.clone()
    if rot["cols"] % 320 == 0 and 320 % rot["head_dim"] == 0:
        for c0 in range(0, rot["cols"], 320):
            v[:, c0:c0 + 320] = rotary(v[:, c0:c0 + 320], rot["table"], rot["tokens"], rot["off"], rot["head_dim"], rot["rot_dim"],
                                       no_modulo=no_modulo)
        return v
    M, hd, rd, cols = v.shape[0], rot["head_dim"], rot["rot_dim"], rot["cols"]
    assert cols % hd == 0 and cols <= v.shape[1]
    rows = torch.arange(M, device=v.device)
    cs = rot["table"][(rows if no_modulo else rows % rot["tokens"]) + rot["off"]].to(f64)
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    h = v[:, :cols].reshape(M, cols // hd, hd).clone()
    x0, x1 = h[:, :, 0:rd:2].clone(), h[:, :, 1:rd:2].clone()
    h[:, :, 0:rd:2], h[:, :, 1:rd:2] = x0 * c - x1 * s, x1 * c + x0 * s
    v[:, :cols] = h.reshape(M, cols)
    return v


def epilogue(acc, p, mut=None, exact=False, geom=GEOM):
    """acc [M, N] float64 -> the value the kernel rounds, or None where `mut` does not apply.  p["silu"] / p["qgelu"] (the tile kernel
    and the reduce pass; not this kernel): v / (1 + exp(-v)) or v * sigmoid(1.702 v) behind bias and row vector"""
    M, N = acc.shape
    BM, WTM = geom["BM"], geom["WTM"]
    dev = acc.device
    rows = torch.arange(M, device=dev)
    v = acc
    if p.get("bias") is not None:
        v = v + p["bias"]
    if p.get("geglu"):
        inner = N // 2
        val, gate = v[:, :inner].clone(), v[:, inner:].clone()
        if mut == "value_gate_exchanged_16":
            i0 = 16 * 3                                                    # the fourth group of the first column tile
            val[:, i0:i0 + 16], gate[:, i0:i0 + 16] = v[:, inner + i0:inner + i0 + 16], v[:, i0:i0 + 16]
        if exact:
            # gelu_erf_f is exactly 0 at 0 and exactly x at the integers 8 .. 64 (test_gpu_fused320_matrix.py::test_gelu_premise)
            assert bool(((gate == 0) | ((gate >= 8) & (gate <= 64) & (gate == gate.round()))).all()), "exact GEGLU: gates 0 or integers 8..64"
            assert bool((gate == 0).any()) and bool((gate >= 8).any())
            assert bool((val == val.round()).all()) and float((val * gate).abs().max()) < 2 ** 24
            v = val * gate
        else:
            v = val * gelu64(gate)
    elif mut == "value_gate_exchanged_16":
        return None
    if p.get("rowvec") is not None:
        rpb = p["rows_per_batch"]
        b = rows // rpb
        if mut == "rowvec_batch_per_wave_tile":
            b = (rows // WTM * WTM) // rpb
            if bool((b == rows // rpb).all()):
                return None
        v = v + p["rowvec"][b]
    elif mut == "rowvec_batch_per_wave_tile":
        return None
    assert not (p.get("silu") and p.get("qgelu")), "one activation per launch"
    if (p.get("silu") or p.get("qgelu")) and p.get("act_exact"):
        # x / (1 + expf(-c x)), c = 1 or 1.702, on the class where fp32 leaves no choice: 0 -> 0; x >= 20 -> x (expf < 2^-25: the
        # denominator is 1); x <= -104 -> -0 (expf overflows to +inf) -- NOT the identity, so a launch without its activation differs
        assert bool(((v == 0) | (v >= 20) | (v <= -104)).all()), "exact SiLU / quick-GELU: 0, at least 20, or at most -104"
        assert bool((v == 0).any()) and bool((v >= 20).any()) and bool((v <= -104).any())
        v = torch.where(v <= -104, torch.zeros_like(v), v)
    elif p.get("silu"):
        v = v * torch.sigmoid(v)
    elif p.get("qgelu"):
        v = v * torch.sigmoid(1.702 * v)
    rot = p.get("rot")
    if mut == "rot_no_modulo" and (rot is None or M <= rot["tokens"]):
        return None
    if rot is not None:
        v = _rot_blocks(v, rot, mut == "rot_no_modulo")
    cs = p.get("col_scale")
    if mut == "colscale_whole_fragment" and (cs is None or cs[1] % 16 == 0):
        return None
    if cs is not None:
        cols = -(-cs[1] // 16) * 16 if mut == "colscale_whole_fragment" else cs[1]
        v = v.clone()
        v[:, :cols] *= cs[0]
    res = p.get("res")
    if mut == "residual_row_clamped":
        if res is None or M % BM in (0, 1):
            return None
        res = res.clone()
        res[(M - 1) // BM * BM:] = res[M - 1]
    if res is not None:
        v = v + res
    return v


def _store(pre, p, mut, geom=GEOM):
    BM, BN = geom["BM"], geom["BN"]
    if mut == "truncating_stores":
        return trunc16(pre)
    out = r16(pre)
    if mut == "tile_twice_one_missing":
        M, N = pre.shape
        if N < 2 * BN:
            return None
        out = out.clone()
        out[:BM, BN:2 * BN] = p.get("prefill", float("nan"))             # tile (0, 1) is never computed: it keeps what the buffer held
    return out


# ------------------------------------------------------------------------------------------- GEMM
def gemm(p, mut=None, exact=False, geom=GEOM):
    """p: a [M, K1], a2 [M, K - K1] or None, w [N, K] (GEGLU: NATURAL order, value rows | gate rows), bias, geglu, rowvec +
    rows_per_batch, rot (dict table, tokens, off, head_dim, rot_dim, cols), col_scale (factor, cols), res, S (K slices, for the
    slice mutations), a2_buf / a2_off / lda (the buffer a2 is a view of, for a2_read_with_lda).
    Returns dict(pre, out): the value before its store and the stored bf16 value, float64; None where `mut` does not apply"""
    a, a2, w = p["a"], p.get("a2"), p["w"]
    M, N, K = a.shape[0], w.shape[0], w.shape[1]
    if mut in ("pad_after_border_valid", "phases_swapped"):
        return None
    A = a if a2 is None else torch.cat([a, a2], 1)
    if mut == "a2_read_with_lda":
        if a2 is None:
            return None
        flat = p["a2_buf"].reshape(-1)
        idx = p["a2_off"] + torch.arange(M, device=a.device)[:, None] * p["lda"] + torch.arange(a2.shape[1], device=a.device)[None, :]
        got = torch.where(idx < flat.numel(), flat[idx.clamp_max(flat.numel() - 1)], torch.zeros((), dtype=f64, device=a.device))
        if torch.equal(got, a2):
            return None
        A = torch.cat([a, got], 1)
    if exact:
        _exact_pre(K, float(A.abs().max()), float(w.abs().max()), *[float(p[k].abs().max()) for k in ("bias", "rowvec", "res") if p.get(k) is not None])
        assert_exact_sums(A, w, *[p[k].expand(M, N) for k in ("bias", "res") if p.get(k) is not None], what="t320 gemm")
    acc = A @ w.t()
    WTM, (c0, c1), (fr0, fc0) = geom["WTM"], geom["wave_cols"], geom["frag"]
    r0 = WTM if M > WTM else 0                                             # wave (1, 1) of tile 0 (wave (0, 1) of a one-wave-row tile)
    rs = slice(r0, min(r0 + WTM, M))
    if mut == "drop_kstep_one_wave":
        acc = acc.clone()
        acc[rs, c0:c1] -= A[rs, K - BK:] @ w[c0:c1, K - BK:].t()
    S = p.get("S", 1)
    if mut in ("slice_last_twice", "slice0_skipped"):
        if S < 2:
            return None
        k0, k1 = slice_bounds(K, S, S - 1 if mut == "slice_last_twice" else 0)
        fr, fc = slice(r0 + fr0, min(r0 + fr0 + 16, M)), slice(fc0, fc0 + 16)    # quad (i 1, j 3) of that wave: a 16 x 16 fragment
        part = A[fr, k0:k1] @ w[fc, k0:k1].t()
        acc = acc.clone()
        acc[fr, fc] += part if mut == "slice_last_twice" else -part
    pre = epilogue(acc, p, mut, exact, geom)
    if pre is None:
        return None
    out = _store(pre, p, mut, geom)
    return None if out is None else dict(pre=pre, out=out)


# ------------------------------------------------------------------------------------------- conv
def _rows_cl(y):
    """[n, C, H, W] -> channels-last rows [n H W, C]"""
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def conv_gather(x, w, stride, pad_after, border_valid=False):
    """the implicit GEMM spelled out: out[(img, oy, ox)] = sum over taps of X[img, oy s + ky - pad0, ox s + kx - pad0] w[:, :, ky, kx], zero
    outside the image.  border_valid: an out-of-image tap is read where its linear address lands (the next row's first pixel, the next
    image's first row, zero behind the tensor) -- the kernel without its validity bit"""
    n, Ci, H, W = x.shape
    pad0 = 0 if pad_after else 1
    pad = 1 if pad_after else 2
    Ho, Wo = (H + pad - 3) // stride + 1, (W + pad - 3) // stride + 1
    flat = torch.cat([_rows_cl(x), torch.zeros((2 * W + 4, Ci), dtype=x.dtype, device=x.device)], 0)
    img, oy, ox = torch.meshgrid(torch.arange(n, device=x.device), torch.arange(Ho, device=x.device), torch.arange(Wo, device=x.device), indexing="ij")
    out = torch.zeros((n * Ho * Wo, w.shape[0]), dtype=x.dtype, device=x.device)
    for ky in range(3):
        for kx in range(3):
            iy, ix = oy * stride + ky - pad0, ox * stride + kx - pad0
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            if border_valid:
                ok = ok | (iy >= H) | (ix >= W)
            idx = (img * H * W + iy * W + ix).clamp(0, flat.shape[0] - 1).reshape(-1)
            out += (flat[idx] * ok.reshape(-1, 1)) @ w[:, :, ky, kx].t()
    return out


def conv(p, mut=None, exact=False, geom=GEOM):
    """p: x [n, Ci, H, W], w [Co, Ci, 3, 3], stride, pad_after, up (True: nearest-2x in front, the four phase convs of ops.conv_up2x),
    and the epilogue keys of gemm().  Returns dict(pre, out) over channels-last rows [n Ho Wo, Co]"""
    x, w = p["x"], p["w"]
    stride, pad_after, up = p.get("stride", 1), p.get("pad_after", False), p.get("up", False)
    if mut in ("drop_kstep_one_wave", "slice_last_twice", "slice0_skipped", "a2_read_with_lda", "value_gate_exchanged_16",
               "rot_no_modulo", "colscale_whole_fragment"):
        return None
    if (mut == "pad_after_border_valid" and not (pad_after and stride == 2)) or (mut == "phases_swapped" and not up):
        return None
    if exact:
        _exact_pre((4 if up else 9) * x.shape[1], float(x.abs().max()), 12.0 if up else float(w.abs().max()),
                   *[float(p[k].abs().max()) for k in ("bias", "rowvec", "res") if p.get(k) is not None])
    if up:
        full = Fn.conv2d(Fn.interpolate(x, scale_factor=2.0, mode="nearest"), w, None, padding=1)
        if mut == "phases_swapped":
            sw = full.clone()
            sw[:, :, 0::2, 1::2], sw[:, :, 1::2, 0::2] = full[:, :, 1::2, 0::2], full[:, :, 0::2, 1::2]
            full = sw
    elif pad_after:
        full = Fn.conv2d(Fn.pad(x, (0, 1, 0, 1)), w, None, stride=stride)
    else:
        full = Fn.conv2d(x, w, None, stride=stride, padding=1)
    acc = _rows_cl(full)
    if mut == "pad_after_border_valid":
        acc = conv_gather(x, w, stride, pad_after, border_valid=True)
    pre = epilogue(acc, p, mut, exact, geom)
    if pre is None:
        return None
    out = _store(pre, p, mut, geom)
    return None if out is None else dict(pre=pre, out=out)


def phase_rows(n_img, H, W, dev):
    """[4, n H W]: output row of GEMM row m of phase z = 2 a + b -- pixel (2 y + a, 2 x + b) of the 2H x 2W image"""
    img, y, x = torch.meshgrid(torch.arange(n_img, device=dev), torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    return torch.stack([((img * 2 * H + 2 * y + a) * 2 * W + 2 * x + b).reshape(-1) for a in (0, 1) for b in (0, 1)], 0)


# ------------------------------------------------------------------------------------------- column sums
def colsum_tiles(stored, rows, gemm_rows=None):
    """[z][M / rows][N][2] of the stored values (float64 holding bf16): per `rows`-row partial of the GEMM's rows; gemm_rows [z, M]
    maps them to output rows (the phase convs), else z = 1 and the rows are the output's"""
    if gemm_rows is None:
        gemm_rows = torch.arange(stored.shape[0], device=stored.device)[None]
    v = stored[gemm_rows]                                                  # [z, M, N]
    t = v.reshape(v.shape[0], -1, rows, v.shape[-1])
    return torch.stack([t.sum(2), t.pow(2).sum(2)], -1)


def colsum_fx(stored, rows, fx_rows, reps, gemm_rows=None):
    """[reps][M / fx_rows][2][N] int64: partial i (rows i rows .. of the GEMM's M) adds round(sum * 2^20) to replica i % reps of the batch
    element its first row lies in; the four phases add to the same buffer"""
    t = colsum_tiles(stored, rows, gemm_rows)                              # [z, P, N, 2]
    z, P, N, _ = t.shape
    out = torch.zeros((reps, P * rows // fx_rows, 2, N), dtype=torch.int64, device=stored.device)
    q = (t * (1 << FX_SHIFT)).round().to(torch.int64)
    for i in range(P):
        out[i % reps, i * rows // fx_rows] += q[:, i].sum(0).t()
    return out


# ------------------------------------------------------------------------------------------- the exact constructions (Part 1)
def _g(seed):
    return torch.Generator().manual_seed(seed)


def sparse_pm1(shape, dev, seed, keep):
    m = (torch.rand(shape, generator=_g(seed + 100)) < keep).to(dev)
    return _ints(shape, dev, seed, -1, 1) * m


def _epilogue_operands(p, spec, M, N, dev, seed, small=False):
    lim = 4 if small else 8
    if spec.get("bias"):
        p["bias"] = _ints((N,), dev, seed + 3, -lim, lim)
    if spec.get("rpb"):
        p["rows_per_batch"] = spec["rpb"]
        p["rowvec"] = _ints((-(-M // spec["rpb"]), N), dev, seed + 4, -lim, lim)
    if spec.get("cs"):
        p["col_scale"] = (0.5, spec["cs"])
    if spec.get("res"):
        p["res"] = _ints((M, N), dev, seed + 5, -lim, lim)
    if spec.get("rot"):
        hd, rd, tokens, off, cols = spec["rot"]
        p["rot"] = dict(table=dyadic_table(max(M, tokens) + off, rd, dev, seed + 6), tokens=tokens, off=off, head_dim=hd, rot_dim=rd, cols=cols)


def exact_gemm(spec, dev):
    """one Part 1 GEMM problem.  spec: M, N, K, k1 (two sources), splits, bias, rpb, cs, res ("lds" | "ldr4" | "base8"), rot (head_dim,
    rot_dim, tokens, off, cols), big (non-negative operands, sums near 12 000), sums (sparse +-1: |C| <= 256), geglu"""
    M, N, K = spec["M"], spec["N"], spec["K"]
    seed = spec.get("seed", 0) * 1000 + M + 7 * N + 13 * K
    p = dict(S=planned_slices(K, spec.get("splits", 1)))
    if spec.get("geglu"):
        inner = N // 2
        A = _ints((M, K), dev, seed + 1)
        g = _g(seed + 2)
        w = torch.zeros((N, K), dtype=f64)
        w[:inner] = torch.randint(-3, 4, (inner, K), generator=g).to(f64)
        b = torch.zeros((N,), dtype=f64)
        b[:inner] = torch.randint(-8, 9, (inner,), generator=g).to(f64)
        i = torch.arange(inner)
        live = (i % 8) != 5                                                # every eighth gate row is all zero with bias 0: gate exactly 0
        for e in range(2):
            k = (11 * i + 5 + e * (1 + torch.randint(0, K - 1, (inner,), generator=g))) % K
            w[inner + i[live], k[live]] += (torch.randint(0, 2, (int(live.sum()),), generator=g) * 2 - 1).to(f64)
        b[inner:][live] = 14.0                                             # 14 +- (3 + 3): gates in 8 .. 20
        p.update(a=A, w=w.to(dev), bias=b.to(dev), geglu=True)
        return p
    if spec.get("big"):
        hi = int(round((48000.0 / K) ** 0.5))
        A, w = _ints((M, K), dev, seed + 1, 0, hi), _ints((N, K), dev, seed + 2, 0, hi)
    elif spec.get("sums"):
        A, w = sparse_pm1((M, K), dev, seed + 1, 0.25), _ints((N, K), dev, seed + 2, -1, 1)
    else:
        A, w = _ints((M, K), dev, seed + 1), _ints((N, K), dev, seed + 2)
    k1 = spec.get("k1") or K
    p.update(a=A[:, :k1].contiguous(), w=w)
    if k1 < K:
        p["a2"] = A[:, k1:].contiguous()
    _epilogue_operands(p, spec, M, N, dev, seed, small=bool(spec.get("sums")))
    return p


def exact_conv(spec, dev):
    """one Part 1 conv problem.  spec: n, H, W, Ci, Co, stride, pad_after, up, splits, bias, rpb (in output rows), res, sums"""
    n, H, W, Ci, Co = spec["n"], spec["H"], spec["W"], spec["Ci"], spec["Co"]
    seed = spec.get("seed", 0) * 1000 + n + 3 * H + 5 * W + 7 * Co
    stride, pad_after, up = spec.get("stride", 1), spec.get("pad_after", False), spec.get("up", False)
    if spec.get("sums"):
        x, w = sparse_pm1((n, Ci, H, W), dev, seed + 1, 0.5 if up else 0.25), _ints((Co, Ci, 3, 3), dev, seed + 2, -1, 1)
    else:
        x, w = _ints((n, Ci, H, W), dev, seed + 1), _ints((Co, Ci, 3, 3), dev, seed + 2)
    p = dict(x=x, w=w, stride=stride, pad_after=pad_after, up=up, S=planned_slices(9 * Ci, spec.get("splits", 1)))
    pad = 1 if pad_after else 2
    Hs, Ws = (2 * H, 2 * W) if up else (H, W)
    M = n * ((Hs + pad - 3) // stride + 1) * ((Ws + pad - 3) // stride + 1)
    _epilogue_operands(p, spec, M, Co, dev, seed, small=bool(spec.get("sums")))
    return p


def _c(M, N, K, **kw):
    return dict(M=M, N=N, K=K, **kw)


ALL_TERMS = dict(bias=True, rpb=96, cs=484, res="lds")
GEMM_EXACT = (
    # ---- tile mapping: 9 row tiles (a group of 8 and a ragged group of 1) x 2 column tiles = 18 tiles, XCD remainder 2; one ragged tile
    [_c(2100, 640, 64)] + [_c(M, 320, 64) for M in (1, 100, 256, 257)]
    # ---- K loop: the ring's first wraps, both sides of the store threshold at K = 3072; two sources with lda != lda2
    + [_c(256, 320, K) for K in (64, 128, 192, 3072, 3136)]
    + [_c(256, 320, k1 + k2, k1=k1) for k1, k2 in ((64, 64), (192, 64), (64, 320))]
    # ---- rounding: sums near 12 000, where the bf16 store rounds most elements
    + [_c(300, 320, 768, big=True, splits=s) for s in (1, 3)]
    # ---- epilogue terms, unsplit and two slices
    + [_c(480, 640, 512, splits=s, **t) for s in (1, 2) for t in (
        dict(bias=True), dict(rpb=96), dict(cs=164), dict(cs=484), dict(res="lds"), dict(res="ldr4"), dict(res="base8"), ALL_TERMS)]
    # ---- rotary from a dyadic table on two thirds of N, the column scale on the first third
    + [_c(480, 960, 512, splits=s, rot=(hd, 32, 96, 16, 640), cs=320) for s in (1, 2) for hd in (40, 80, 160)]
    # ---- in-launch split-K: shares of the 40 quads that do not divide evenly
    + [_c(M, N, K, splits=S, bias=True, res="lds") for M in (256, 300) for N in (320, 640) for S, K in ((2, 512), (3, 768), (7, 1792), (16, 4096))]
    + [_c(256, 320, 1024, splits=16),                  # the host clamps to K / 256 = 4 slices
       _c(2304, 640, 4096, splits=16)]                 # 18 tiles x 16 slices > the CUs: the launch clamps; integers make S irrelevant
)
GEGLU_EXACT = [_c(300, 640, 64, geglu=True), _c(300, 2560, 320, geglu=True)]
for _i, _s in enumerate(GEMM_EXACT + GEGLU_EXACT):
    _s["seed"] = _i + 1


def _v(n, H, W, Co=320, **kw):
    return dict(n=n, H=H, W=W, Ci=64, Co=Co, **kw)


CONV_EXACT = (
    # one image, and several whose boundaries fall inside a 256-row tile; unsplit and two slices (K = 576)
    [_v(n, H, W, stride=st, pad_after=pa, splits=s)
     for (H, W, st, pa) in ((6, 10, 1, False), (20, 20, 1, False), (6, 10, 2, False), (16, 16, 2, False), (16, 24, 2, True))
     for n in (1, 3) for s in (1, 2)]
    + [_v(3, 20, 20, splits=s, bias=True, rpb=400, res="lds") for s in (1, 2)]
    + [_v(3, 6, 10, stride=2, splits=s, bias=True, rpb=15, res="ldr4") for s in (1, 2)]
)
UP_EXACT = [_v(n, H, W, Co=Co, up=True, bias=True) for (n, H, W) in ((3, 6, 10), (5, 8, 8)) for Co in (320, 640)]
for _i, _s in enumerate(CONV_EXACT + UP_EXACT):
    _s["seed"] = _i + 1


def case_id(s):
    if "n" in s:
        return (f"n{s['n']}-{s['H']}x{s['W']}-co{s['Co']}-s{s.get('stride', 1)}" + ("-padafter" if s.get("pad_after") else "") + ("-up" if s.get("up") else "")
                + f"-S{s.get('splits', 1)}" + "".join(f"-{k}" for k in ("bias", "rpb", "res") if s.get(k)))
    return (f"{s['M']}x{s['N']}x{s['K']}" + (f"-k1_{s['k1']}" if s.get("k1") else "") + f"-S{s.get('splits', 1)}"
            + "".join(f"-{k}{'' if s[k] is True else '_' + str(s[k]).replace(' ', '')}" for k in ("bias", "rpb", "cs", "res", "rot", "big", "geglu") if s.get(k)))


# ------------------------------------------------------------------------------------------- the N(0, 1) problems (Part 2)
def _randn(shape, dev, seed, scale=1.0):
    return (torch.randn(shape, generator=_g(seed), dtype=f64) * scale).to(dev)


ROWS_CASES = [(kind, M, amp) for kind in ("geglu", "rotary") for M in (300, 512) for amp in (1.0, 4.0)]


def real_rotary_table(rows, rot_dim, dev):
    freqs = 10000.0 ** (-torch.arange(0, rot_dim, 2, dtype=f64) / rot_dim)
    ang = torch.arange(rows, dtype=f64)[:, None] * freqs[None, :]
    return torch.stack([ang.cos(), ang.sin()], -1).to(f32).to(dev)


def random_problem(kind, M, amp, dev, make_table=None, N=640, K=320):
    """operands N(0, 1) x amp rounded to bf16, weights N(0, 1 / K); geglu: ff.net.0 (bias N(0, 0.5^2)); rotary: a q | k projection with
    the table a stored operand (make_table: the GPU file passes seer_rotary_table's output), tokens 96, offset 16, the q prescale"""
    seed = 31 * M + int(amp) * 1000 + (0 if kind == "geglu" else 500)
    p = dict(a=r16(_randn((M, K), dev, seed + 1, amp)), w=r16(_randn((N, K), dev, seed + 2, K ** -0.5)))
    if kind == "geglu":
        p["bias"] = _randn((N,), dev, seed + 3, 0.5).to(f32).to(f64)
        p["geglu"] = True
    else:
        tokens, off = 96, 16
        p["rot"] = dict(table=(make_table or real_rotary_table)(max(M, tokens) + off, 32, dev), tokens=tokens, off=off, head_dim=40, rot_dim=32, cols=320)
        p["col_scale"] = (float(torch.tensor(40 ** -0.5 * 1.4426950408889634, dtype=f32)), 320)
    return p


def old_problem(M, N, K, dev, seed=0, **terms):
    """the data of tests/test_gpu_t320.py: N(0, 1) activations, weights N(0, 1 / K), N(0, 1) bias, row vector and residual, bf16 storage"""
    p = dict(a=r16(_randn((M, K), dev, seed + 1)), w=r16(_randn((N, K), dev, seed + 2, K ** -0.5)))
    k1 = terms.get("k1")
    if k1:
        p["a2"] = p["a"][:, k1:].contiguous()
        p["a"] = p["a"][:, :k1].contiguous()
    if terms.get("bias"):
        p["bias"] = _randn((N,), dev, seed + 3).to(f32).to(f64)
    if terms.get("rpb"):
        p["rows_per_batch"], p["rowvec"] = terms["rpb"], _randn((-(-M // terms["rpb"]), N), dev, seed + 4).to(f32).to(f64)
    if terms.get("res"):
        p["res"] = r16(_randn((M, N), dev, seed + 5))
    if terms.get("cs"):
        p["col_scale"] = (0.125, terms["cs"])
    if terms.get("rot"):
        hd, rd, tokens, off, cols = terms["rot"]
        p["rot"] = dict(table=real_rotary_table(max(M, tokens) + off, rd, dev), tokens=tokens, off=off, head_dim=hd, rot_dim=rd, cols=cols)
    if terms.get("geglu"):
        p["geglu"] = True
    p["S"] = terms.get("S", 1)
    return p


def old_conv_problem(n, H, W, Ci, Co, dev, seed=0, **terms):
    x = r16(_randn((n, Ci, H, W), dev, seed + 1))
    w = r16(_randn((Co, Ci, 3, 3), dev, seed + 2, (9 * Ci) ** -0.5))
    return dict(x=x, w=w, stride=terms.get("stride", 1), pad_after=terms.get("pad_after", False), up=terms.get("up", False),
                bias=_randn((Co,), dev, seed + 3).to(f32).to(f64))


def old_close(got64, ref64, rtol=2e-2, atol=2e-2):
    """tests/test_gpu_t320.py::_close as a reading: (passes, worst err / (atol + rtol |ref|)); a non-finite output fails it"""
    if not bool(torch.isfinite(got64).all()):
        return False, float("inf")
    ratio = float(((got64 - ref64).abs() / (atol + rtol * ref64.abs())).max())
    return ratio <= 1.0, ratio
