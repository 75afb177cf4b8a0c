"""References, emulations and exact constructions for the two fused 320-channel launches, seer_rowchain_c320 (csrc/rowchain.hip) and
seer_ff_fused_c320 (csrc/ff_fused.hip), and their three pack entry points.  Plain torch in float64, on whatever device the operands
live; no dependency on the library and nothing here comes from a kernel's output.  Used by tests/test_gpu_fused320_matrix.py (the
kernels) and tests/test_fused320_ref_cpu.py (the preconditions and the mutation table, no GPU).

    rowchain:   h   = [GroupNorm(inp)] W1^T + b1 [+ res]
                out = LayerNorm(h) [W2_0 | ...]^T, rotary on the first rot_thirds, col_scale on the first scale_thirds
    ff_fused:   y   = x + [Wp | Wp W2] [h | g] + bcat,   g = GEGLU(LayerNorm(h) W1^T + b1),   h <- h + a Wo^T + bo with the prologue

Three modes of the same two functions:
  reference (dt = None)        the operator in float64 on the stored operands, no rounding anywhere;
  emulation (dt = bf16 / f16)  the same with ONE round-to-nearest-even to the storage type exactly where the kernels round, as read from
                               the sources: GN(x) into the tile (rowchain.hip: pack8t behind v * sc + sh), h (pack2t in the g == 0
                               epilogue: what is stored AND what LayerNorm reads), LN(h) (pack8t), the prologue's h + a Wo^T + bo
                               (ff_fused.hip, PRE), g (geglu: pack2t), and the final out / y after rotary and scale in fp32;
  exact (exact = True)         Part 1.  At the three inexact spots (rsqrtf of GroupNorm, rsqrtf of LayerNorm, gelu_erf_f) the value the
                               kernel rounds is REPLACED by the number it must round to, after asserting the preconditions: that number
                               is non-zero and representable in the storage type, and the kernel's own formula (with eps) lies within
                               2^-12 relative of it, also in float32 with rstd moved by +-4 ulp.  Every partial sum stays below 2^24
                               in units of the operands' common last bit, so the fp32 accumulators are exact.

`mut` applies one of MUTATIONS to the emulation: the kernel bugs the matrix must be able to see."""
import math

import torch

f16, bf16, f32, f64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
C, INNER, BM = 320, 1280, 96
FX_SHIFT = 20                      # SEER_GN_FX_SHIFT (include/seer_hip.h): the accumulated column sums hold value * 2^20
MUTATIONS = ["gn_first_batch", "gn_group_plus1", "rot_no_offset", "rot_no_modulo", "rot_wrong_third", "scale_wrong_third",
             "drop_last_kstep_one_wave", "pack_w_j_exchanged", "ragged_last_row_shifted", "value_gate_exchanged_16", "skip_chunk_half",
             "colsum_segment_to_first", "gn_fx_skip_replica"]


def r16(x64, dt):
    """one round-to-nearest-even to the storage type, back in float64"""
    return x64.to(dt).to(f64)


def rounded_share(x64, dt):
    """share of elements the store to `dt` changes"""
    return float((r16(x64, dt) != x64).double().mean())


def row_floor(ref64):
    """the floor of the per-row relative error, as profiles/attn_fwd_matrix.md: 2^-6 of the rms row norm of the reference"""
    return float(ref64.norm(dim=-1).pow(2).mean().sqrt()) * 2.0 ** -6


def row_err(x, ref64, floor):
    """worst own row: |x - ref|_2 / max(|ref|_2, floor)"""
    return float(((x.to(f64) - ref64).norm(dim=-1) / ref64.norm(dim=-1).clamp_min(floor)).max())


def _grid(dev, *sizes):
    return torch.meshgrid(*[torch.arange(n, device=dev) for n in sizes], indexing="ij")


# ------------------------------------------------------------------------------------------- the pack orders, from include/seer_hip.h
def rowchain_pack_index(n_mats, dev):
    """seer_rowchain_pack: out[t][K step 5][wave 4][k32 2][column fragment 5][lane 64][8] =
    W[320 t + 80 w + 16 j + (lane & 15)][64 s + 32 k32 + 8 (lane >> 4) + e]   ->   (row, column) of W per output element"""
    t, s, w, k32, j, lane, e = _grid(dev, n_mats, 5, 4, 2, 5, 64, 8)
    return (320 * t + 80 * w + 16 * j + (lane & 15)).reshape(-1), (64 * s + 32 * k32 + 8 * (lane >> 4) + e).reshape(-1)


def ff_pack_w1_index(dev):
    """seer_ff_fused_pack_w1: out[chunk 20][wave 4][K step 5][k32 2][value | gate][lane 64][8] =
    w1[128 c + 32 w + 16 f + (lane & 15)][64 ks + 32 k32 + 8 (lane >> 4) + e]"""
    c, w, ks, k32, f, lane, e = _grid(dev, 20, 4, 5, 2, 2, 64, 8)
    return (128 * c + 32 * w + 16 * f + (lane & 15)).reshape(-1), (64 * ks + 32 * k32 + 8 * (lane >> 4) + e).reshape(-1)


def ff_pack_wcat_index(dev):
    """seer_ff_fused_pack_wcat: out[K step 25][wave 4][k32 2][column fragment 5][lane 64][8] =
    wcat[80 w + 16 j + (lane & 15)][64 s + 32 k32 + 8 (lane >> 4) + e]"""
    s, w, k32, j, lane, e = _grid(dev, 25, 4, 2, 5, 64, 8)
    return (80 * w + 16 * j + (lane & 15)).reshape(-1), (64 * s + 32 * k32 + 8 * (lane >> 4) + e).reshape(-1)


def geglu_interleave_order(dev):
    """the header's "interleaved GEGLU row order: 16 value rows, 16 gate rows, ...": packed row p -> row of the natural
    [value 1280 | gate 1280] matrix"""
    p = torch.arange(2 * INNER, device=dev)
    return ((p // 16) % 2) * INNER + 16 * (p // 32) + p % 16


# ------------------------------------------------------------------------------------------- preconditions of the exact constructions
def assert_exact_sums(a64, w64, *adds, what):
    """every partial sum of a W^T (+ adds) is an integer multiple of the operands' common last bit (at most 1/8) below 2^24 of it: the
    fp32 accumulator is exact whatever the order"""
    for t in (a64, w64) + adds:
        assert bool((t * 8 == (t * 8).round()).all()), f"{what}: an operand is no multiple of 1/8"
    bound = a64.abs() @ w64.abs().t()
    for t in adds:
        bound = bound + t.abs()
    assert float(bound.max()) * 8 < 2 ** 24, f"{what}: a partial sum can reach 2^24 units"


def assert_fp32(x64, what):
    assert torch.equal(x64.to(f32).to(f64), x64), f"{what}: not exact in fp32"


def assert_absorbed(centered, rstd, gamma, beta, target, dt, what):
    """an inexact spot: the kernel stores round16((centered * rstd) * gamma + beta) with rstd = rsqrtf(var + eps).  `target` is the same
    with rstd = 1.  The rounding must absorb the difference: target non-zero and representable, the formula within 2^-12 relative of
    it, and the float32 evaluation with rstd moved by -4, 0, +4 ulp rounds to target"""
    assert bool((target != 0).all()), f"{what}: an exact value of 0 (the trap: it comes out as ~1e-5)"
    assert torch.equal(r16(target, dt), target), f"{what}: target not representable in the storage type"
    v = centered * rstd * gamma + beta
    assert bool(((v - target).abs() <= 2.0 ** -12 * target.abs()).all()), f"{what}: the formula is not within 2^-12 of its target"
    r32 = rstd.to(f32) if torch.is_tensor(rstd) else torch.tensor(rstd, dtype=f32, device=target.device)
    ulp = torch.finfo(f32).eps * r32.abs() / 2
    for k in (-4, 0, 4):
        o = (centered.to(f32) * (r32 + k * ulp)) * gamma.to(f32) + beta.to(f32)
        assert torch.equal(o.to(dt).to(f64), target), f"{what}: rstd {k:+d} ulp is not absorbed by the 16-bit rounding"


# ------------------------------------------------------------------------------------------- GroupNorm statistics, both forms
def _ulps32(x64, k):
    """x (float64 holding fp32 values) moved by k fp32 ulps"""
    x = x64.to(f32)
    for _ in range(abs(k)):
        x = torch.nextafter(x, torch.full_like(x, float("inf") if k > 0 else float("-inf")))
    return x.to(f64)


def gn_moments(gn, mode, mut=None):
    """gn_moments_plain, then in mode 'kernel' the fp32 (mean, var) moved by gn["ulps"] = (k_mean, k_var) fp32 ulps where given: the
    flip events of test_rows_gn_fx_against_gn_stats are sampled that way (var stays >= 0 as in the kernel)"""
    mom = gn_moments_plain(gn, mode, mut)
    if mom is None or mode != "kernel" or gn.get("ulps") is None:
        return mom
    return _ulps32(mom[0], gn["ulps"][0]), _ulps32(mom[1], gn["ulps"][1]).clamp_min(0)


def gn_moments_plain(gn, mode, mut=None):
    """(mean, var) [B, G] float64 from the statistics the launch is given.  gn: form 'stats' (stats [B, G, 2] = sum, sum of squares per
    group, the stored fp32 values) or 'fx' (fx [reps, B, 2, 320] int64: per-channel sums * 2^20, spread over replicas); count, groups.
    mode 'ref': float64, 1 / count exact.  mode 'kernel': rowchain.hip's arithmetic -- inv_count = (float)(1 / count); stats form in
    fp32 (mean = s inv, var = q inv - mean^2), fx form with integer adds and one conversion per group in double"""
    G, count = gn["groups"], gn["count"]
    inv32 = float(torch.tensor(1.0 / count, dtype=f32))
    if gn["form"] == "stats":
        s, q = gn["stats"][..., 0], gn["stats"][..., 1]
        if mode == "ref":
            mean = s / count
            return mean, (q / count - mean * mean).clamp_min(0)
        s32, q32, i32 = s.to(f32), q.to(f32), torch.tensor(inv32, dtype=f32, device=s.device)
        mean = s32 * i32
        var = (q32 * i32 - mean * mean).clamp_min(0)
        return mean.to(f64), var.to(f64)
    fx = gn["fx"]
    if mut == "gn_fx_skip_replica":
        if fx.shape[0] < 2:
            return None
        fx = fx[:-1]
    tot = fx.sum(0)                                                       # [B, 2, 320] int64, exact
    B = tot.shape[0]
    grp = tot.reshape(B, 2, G, C // G).sum(-1).to(f64)                    # below 2^53: exact
    k = (1.0 / count if mode == "ref" else inv32) / float(1 << FX_SHIFT)
    mean = grp[:, 0] * k
    var = (grp[:, 1] * k - mean * mean).clamp_min(0)
    if mode == "kernel":
        mean, var = mean.to(f32).to(f64), var.to(f32).to(f64)
    return mean, var


def rotary(y, table, tokens, off, head_dim, rot_dim, no_modulo=False):
    """rows of y [M, 320] as heads of head_dim channels, the first rot_dim rotated in interleaved pairs:
    (x0, x1) -> (x0 c - x1 s, x1 c + x0 s) with (c, s) = table[row % tokens + off][pair]"""
    M = y.shape[0]
    rows = torch.arange(M, device=y.device)
    pos = (rows if no_modulo else rows % tokens) + off
    cs = table[pos].to(f64)
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    v = y.reshape(M, C // head_dim, head_dim).clone()
    x0, x1 = v[:, :, 0:rot_dim:2].clone(), v[:, :, 1:rot_dim:2].clone()
    v[:, :, 0:rot_dim:2] = x0 * c - x1 * s
    v[:, :, 1:rot_dim:2] = x1 * c + x0 * s
    return v.reshape(M, C)


def _layernorm(h, gamma, beta, eps):
    mean = h.mean(-1, keepdim=True)
    d = h - mean
    rstd = (d.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    return d, rstd, d * rstd * gamma + beta


def _wj_exchanged(w):
    """the 16-row blocks of a 320-row matrix with the wave and the column-fragment index exchanged in the packed order: slot (w, j) of
    the nest [w 4][j 5] holds what a nest [j 5][w 4] puts at the same offset"""
    blk = torch.arange(20, device=w.device)
    src = (blk % 5) * 4 + blk // 5                                        # slot w * 5 + j  <-  block index j * 4 + w of the other nest
    return w.reshape(20, 16, -1)[src].reshape(w.shape)


# ------------------------------------------------------------------------------------------- rowchain
def rowchain(p, dt=None, exact=False, mut=None):
    """p: inp [M, 320], w1 [320, 320], b1, res (or None), gn (dict: see gn_moments, + gamma, beta, eps, rows_pb; or None),
    ln ((gamma, beta, eps) or None), w2 ([n2 * 320, 320] or None), col_scale, scale_thirds, rot (dict table, tokens, off, head_dim,
    rot_dim, thirds; or None) -- all float64.  Returns dict(h, out) in float64 (out None without w2), or None where `mut` does not apply"""
    assert not (exact and (dt is None or mut is not None))
    if mut in ("value_gate_exchanged_16", "skip_chunk_half", "colsum_segment_to_first"):
        return None
    rnd = (lambda x: x) if dt is None else (lambda x: r16(x, dt))
    inp, w1 = p["inp"], p["w1"]
    M, dev = inp.shape[0], inp.device
    rows = torch.arange(M, device=dev)
    ragged = M % BM != 0
    T = inp
    gn = p.get("gn")
    if mut in ("gn_first_batch", "gn_group_plus1", "gn_fx_skip_replica") and gn is None:
        return None
    if gn is not None:
        mom = gn_moments(gn, "ref" if dt is None else "kernel", mut)
        if mom is None or (mut == "gn_fx_skip_replica" and gn["form"] != "fx"):
            return None
        mean, var = mom
        G, rpb = gn["groups"], gn["rows_pb"]
        b = rows // rpb
        if mut == "gn_first_batch":
            b = (rows // BM * BM) // rpb
            if bool((b == rows // rpb).all()):
                return None
        g = torch.arange(C, device=dev) // (C // G)
        if mut == "gn_group_plus1":
            g = (g + 1) % G
        mu, vr = mean[b][:, g], var[b][:, g]
        rstd = (vr + gn["eps"]).rsqrt()
        if exact:
            assert bool((vr == 1).all()) and bool((mu == mu.round()).all()), "exact GroupNorm: mean an integer, variance 1"
            assert mean.unique().numel() == mean.numel(), "exact GroupNorm: the means of all (batch element, group) must differ"
            target = (inp - mu) * gn["gamma"] + gn["beta"]
            assert_absorbed(inp - mu, rstd, gn["gamma"].expand(M, C), gn["beta"].expand(M, C), target, dt, "GN(x)")
            # the kernel computes x * sc + (beta - mean * sc): the same number up to fp32 roundings of x * sc with |x| <= 64 -- relative
            # to |target| >= 1/2 at most 64 * 3 * 2^-23 / (1/2) = 2^-15.4, inside the 2^-12 the rounding absorbs (16-bit spacing at
            # |target| <= 16 is at least 2^-7 |target| in bf16 and 2^-10 |target| in fp16)
            assert float(inp.abs().max()) <= 64 and float(target.abs().max()) <= 16
            T = target
        else:
            sc = rstd * gn["gamma"]
            T = rnd(inp * sc + (gn["beta"] - mu * sc))
    if mut == "pack_w_j_exchanged":
        w1 = _wj_exchanged(w1)
    b1 = p.get("b1")
    res = p.get("res")
    adds = [t for t in (b1, res) if t is not None]
    h = T @ w1.t()
    if mut == "drop_last_kstep_one_wave":
        h[:, 80:160] -= T[:, 256:] @ w1[80:160, 256:].t()
    for t in adds:
        h = h + t
    if exact:
        assert_exact_sums(T, w1, *[t.expand(M, C) for t in adds], what="h")
        assert_fp32(h, "h before its store")
    hs = rnd(h)
    if mut == "ragged_last_row_shifted":
        if not ragged or M < 2:
            return None
        hs = hs.clone()
        hs[M - 2] = hs[M - 1]
    if p.get("w2") is None:
        return None if mut in ("rot_no_offset", "rot_no_modulo", "rot_wrong_third", "scale_wrong_third") else dict(h=hs, out=None, h_pre=h)
    L = hs
    if p.get("ln") is not None:
        gamma, beta, eps = p["ln"]
        d, rstd, L = _layernorm(hs, gamma, beta, eps)
        if exact:
            assert bool((hs.abs() == 1).all()) and bool((hs.sum(-1) == 0).all()), "exact LayerNorm: rows of +-1, 160 of each"
            assert bool((beta.abs() > gamma.abs()).all())
            target = hs * gamma + beta
            assert_absorbed(d, rstd.expand(M, C), gamma.expand(M, C), beta.expand(M, C), target, dt, "LN(h)")
            L = target
        else:
            L = rnd(L)
    w2 = p["w2"]
    n2 = w2.shape[0] // C
    if exact:
        assert_exact_sums(L, w2, what="out")
    out = L @ w2.t()
    rot, st, scale = p.get("rot"), p.get("scale_thirds", 0), p.get("col_scale", 1.0)
    rt = rot["thirds"] if rot is not None else 0
    if (mut in ("rot_no_offset", "rot_no_modulo", "rot_wrong_third") and rt == 0) or (mut == "scale_wrong_third" and (st == 0 or scale == 1.0)):
        return None
    if mut == "rot_no_offset" and rot["off"] == 0:
        return None
    if mut == "rot_no_modulo" and M <= rot["tokens"]:
        return None
    rot_set = {(t + 1) % n2 for t in range(rt)} if mut == "rot_wrong_third" else set(range(rt))
    scale_set = {(t + 1) % n2 for t in range(st)} if mut == "scale_wrong_third" else set(range(st))
    if (mut == "rot_wrong_third" and rot_set == set(range(rt))) or (mut == "scale_wrong_third" and scale_set == set(range(st))):
        return None
    thirds = []
    for t in range(n2):
        v = out[:, t * C:(t + 1) * C]
        if t in rot_set:
            v = rotary(v, rot["table"], rot["tokens"], 0 if mut == "rot_no_offset" else rot["off"], rot["head_dim"], rot["rot_dim"],
                       no_modulo=mut == "rot_no_modulo")
        if t in scale_set:
            v = v * scale
        thirds.append(v)
    out = torch.cat(thirds, 1)
    if exact:
        assert_fp32(out, "out before its store")
        assert float(out.abs().max()) < 60000
    outs = rnd(out)
    if mut == "ragged_last_row_shifted":
        outs = outs.clone()
        outs[M - 2] = outs[M - 1]
    return dict(h=hs, out=outs, h_pre=h, out_pre=out)


# ------------------------------------------------------------------------------------------- ff_fused
def gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def ff(p, dt=None, exact=False, mut=None, info=None):
    """p: h, x [M, 320], gamma, beta, eps, w1 [2560, 320] in the NATURAL order (value rows 0..1279 | gate rows), b1 [2560], wcat
    [320, 1600] = [Wp | Wp W2], bcat, pre ((a, wo, bo) or None) -- float64.  Returns y [M, 320] float64, or None where `mut` does not apply"""
    assert not (exact and (dt is None or mut is not None))
    rnd = (lambda x: x) if dt is None else (lambda x: r16(x, dt))
    h, x, wcat = p["h"], p["x"], p["wcat"]
    M = h.shape[0]
    if p.get("pre") is not None:
        a, wo, bo = p["pre"]
        if exact:
            assert_exact_sums(a, wo, bo.expand(M, C), h, what="prologue")
        h = rnd(h + a @ wo.t() + bo)
    d, rstd, L = _layernorm(h, p["gamma"], p["beta"], p["eps"])
    if exact:
        assert bool((h.abs() == 1).all()) and bool((h.sum(-1) == 0).all()), "exact LayerNorm: rows of +-1, 160 of each"
        assert bool((p["beta"].abs() > p["gamma"].abs()).all())
        target = h * p["gamma"] + p["beta"]
        assert_absorbed(d, rstd.expand(M, C), p["gamma"].expand(M, C), p["beta"].expand(M, C), target, dt, "LN(h)")
        L = target
    else:
        L = rnd(L)
    w1, b1 = p["w1"], p["b1"]
    if exact:
        assert_exact_sums(L, w1, b1.expand(M, 2 * INNER), what="H")
        assert bool((w1 != 0).any(0).all()) and bool((w1[:INNER] != 0).any(1).all()), "every k position and every value row is hit"
    H = L @ w1.t() + b1
    val, gate = H[:, :INNER].clone(), H[:, INNER:].clone()
    if mut == "value_gate_exchanged_16":
        i0 = 64 * 3 + 16 * 2                                              # chunk 3, wave 2
        val[:, i0:i0 + 16], gate[:, i0:i0 + 16] = H[:, INNER + i0:INNER + i0 + 16], H[:, i0:i0 + 16]
    if exact:
        # gelu_erf_f(x) = fma(-a, 2^(..), max(x, 0)) with a clamped at 5.657: exactly 0 at 0, x - 4.4e-8 -> x in fp32 from 8 up
        # (premise established on the device by test_gelu_premise); negative gates give -4e-8, not 0
        assert bool(((gate == 0) | ((gate >= 8) & (gate == gate.round()))).all()), "exact GEGLU: gates 0 or integers >= 8"
        assert bool((gate == 0).any()) and bool((gate >= 8).any())
        g = val * gate
        assert float(g.abs().max()) <= 256 and torch.equal(r16(g, dt), g), "exact GEGLU: g exact in the storage type"
    else:
        g = rnd(val * gelu64(gate))
    if mut == "skip_chunk_half":
        if M <= 48:
            return None
        g = g.clone()
        g[48:min(M, 96), 64 * 5:64 * 6] = 0                               # tile 0, rows 48..95, chunk 5
    if exact:
        assert_exact_sums(torch.cat([h, g], 1), wcat, p["bcat"].expand(M, C), x, what="y")
    y = x + h @ wcat[:, :C].t() + g @ wcat[:, C:].t() + p["bcat"]
    if exact:
        assert_fp32(y, "y before its store")
        assert float(y.abs().max()) < 60000
    if info is not None:
        info["y_pre"] = y
    y = rnd(y)
    if mut == "ragged_last_row_shifted":
        if M % BM == 0 or M < 2:
            return None
        y = y.clone()
        y[M - 2] = y[M - 1]
    elif mut not in (None, "value_gate_exchanged_16", "skip_chunk_half"):
        return None
    return y


def colsums_fx(y16, fx_rows, reps, mut=None):
    """seer_ff_fused_c320's colsum_fx [reps][M / fx_rows][2][320] int64 of the STORED y (float64 holding 16-bit values), per replica:
    96-row tile t adds to replica t % reps; its 16-row segments go to the batch element they lie in"""
    M = y16.shape[0]
    nb = M // fx_rows
    out = torch.zeros((reps, nb, 2, C), dtype=torch.int64, device=y16.device)
    moved = False
    for t in range(-(-M // BM)):
        for s in range(6):
            r0 = BM * t + 16 * s
            if r0 >= M:
                break
            seg = y16[r0:min(r0 + 16, M)]
            b = r0 // fx_rows
            if mut == "colsum_segment_to_first" and b != (BM * t) // fx_rows:
                b, moved = (BM * t) // fx_rows, True
            out[t % reps, b, 0] += (seg.sum(0) * (1 << FX_SHIFT)).round().to(torch.int64)
            out[t % reps, b, 1] += (seg.pow(2).sum(0) * (1 << FX_SHIFT)).round().to(torch.int64)
    return None if (mut is not None and not moved) else out


def colsum_tiles(y16):
    """colsum_tiles [M / 96][320][2]: (sum, sum of squares) of the stored values per 96-row tile"""
    t = y16.reshape(-1, BM, C)
    return torch.stack([t.sum(1), t.pow(2).sum(1)], -1)


# ------------------------------------------------------------------------------------------- the exact constructions (Part 1)
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, dev, seed, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).to(dev).to(f64)


def signs(shape, dev, seed):
    return (torch.randint(0, 2, shape, generator=_gen(seed)) * 2 - 1).to(dev).to(f64)


def balanced_rows(M, dev, seed):
    """[M, 320] of +-1, 160 of each per row, a random permutation per row: mean 0 and variance 1 exactly"""
    order = torch.rand((M, C), generator=_gen(seed)).argsort(-1)
    return ((order < C // 2).to(f64) * 2 - 1).to(dev)


def signed_permutation(dev, seed):
    """W [320, 320] with W[n, perm(n)] = s_n = +-1: output column n picks exactly input column perm(n)"""
    perm = torch.randperm(C, generator=_gen(seed))
    s = signs((C,), "cpu", seed + 1)
    w = torch.zeros((C, C), dtype=f64)
    w[torch.arange(C), perm] = s
    return w.to(dev), perm.to(dev), s.to(dev)


def ln_affine(dev, seed, gmax=3, extra=5):
    """gamma a signed integer in 1..gmax, beta a signed integer with |gamma| < |beta| <= |gamma| + extra"""
    gamma = ints((C,), dev, seed, 1, gmax) * signs((C,), dev, seed + 1)
    beta = (gamma.abs() + ints((C,), dev, seed + 2, 1, extra)) * signs((C,), dev, seed + 3)
    return gamma, beta


ROT_CHOICES = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0), (0.5, 0.5), (0.5, -0.5), (2.0, 1.0)]


def dyadic_table(rows, rot_dim, dev, seed):
    """[rows, rot_dim / 2, 2] fp32 of dyadic (cos, sin) pairs, a seeded choice per (position, pair); neighbours in either direction differ:
    index = (3 pos + 2 pair + r(pos)) mod 7 with r in {0, 1, 2}, so one step in pos moves it by 1..5 and one step in pair by 2"""
    r = torch.randint(0, 3, (rows,), generator=_gen(seed))
    idx = (3 * torch.arange(rows)[:, None] + 2 * torch.arange(rot_dim // 2)[None, :] + r[:, None]) % 7
    assert bool((idx[1:] != idx[:-1]).all()) and bool((idx[:, 1:] != idx[:, :-1]).all())
    return torch.tensor(ROT_CHOICES, dtype=f32)[idx].to(dev)


def exact_gn(form, B, rows_pb, groups, reps, dev, seed, half=False):
    """statistics the TEST supplies (the kernel takes them as an input): mean a distinct small integer m(b, g), variance 1, count 1024 (a
    power of two: 1 / count and every product with it are exact in fp32).  x = m + integers in [-3, 3]; gamma a signed integer, beta an
    odd multiple of 1/2: no value is 0, everything downstream a multiple of 1/2.  half: gamma = +-1, beta = +-1/2 and x chosen so that
    GN(x) = +-1/2 (for a signed permutation W1 of +-2 in front of an exact LayerNorm)"""
    count = 1024.0
    m = (torch.randperm(B * groups, generator=_gen(seed)).to(f64) - (B * groups) // 2).reshape(B, groups).to(dev)
    gn = dict(form=form, count=count, groups=groups, rows_pb=rows_pb, eps=1e-6, m=m)
    if form == "stats":
        gn["stats"] = torch.stack([m * count, (1 + m * m) * count], -1)
    else:
        cpg = C // groups
        tot = torch.stack([m * count, (1 + m * m) * count], 1) * (1 << FX_SHIFT)                   # [B, 2, G]
        parts = torch.randint(-(1 << 34), 1 << 34, (reps, B, 2, groups, cpg), generator=_gen(seed + 1)).to(dev)
        parts[0, :, :, :, 0] += tot.to(torch.int64) - parts.sum((0, 4))                            # uneven, both signs, exact totals
        gn["fx"] = parts.reshape(reps, B, 2, C)
        assert bool((gn["fx"] < 0).any()) and bool((gn["fx"] > 0).any())
    if half:
        gn["gamma"], gn["beta"] = signs((C,), dev, seed + 2), signs((C,), dev, seed + 3) * 0.5
    else:
        gn["gamma"] = ints((C,), dev, seed + 2, 1, 3) * signs((C,), dev, seed + 3)
        gn["beta"] = (2 * ints((C,), dev, seed + 4, -3, 3) + 1) * 0.5
    return gn


def exact_rowchain(spec, dt, dev):
    """one Part 1 problem from a case of ROWCHAIN_EXACT (float64 operands, every one exact in the storage type)"""
    M, n2, seed = spec["M"], spec.get("n2", 0), 100 * spec.get("seed", 0) + 100000 * spec["M"]
    p = dict(col_scale=0.5, scale_thirds=spec.get("scale_thirds", 0))
    gnspec, ln = spec.get("gn"), spec.get("ln", False)
    hi = spec.get("hi", 3)
    if gnspec is not None:
        form, B, rows_pb, groups, reps = gnspec
        assert B * rows_pb == M
        gn = exact_gn(form, B, rows_pb, groups, reps, dev, seed + 50, half=ln)
        mu = gn["m"][torch.arange(M, device=dev) // rows_pb][:, torch.arange(C, device=dev) // (C // groups)]
        p["gn"] = gn
    if ln:
        w1, perm, s = signed_permutation(dev, seed + 1)
        want_h = balanced_rows(M, dev, seed + 2)                           # h[n] = s_n t[perm(n)] * amp
        t = torch.empty((M, C), dtype=f64, device=dev)
        t[:, perm] = want_h * s
        if gnspec is not None:
            w1 = w1 * 2                                                    # GN(x) = t / 2
            p["inp"] = mu + (t / 2 - gn["beta"]) / gn["gamma"]             # gamma (x - m) + beta = t / 2: x - m in {-1, 0, 1}
        else:
            p["inp"] = t
        p["w1"], p["perm"] = w1, perm
        p["ln"] = (*ln_affine(dev, seed + 3), 1e-5)
    else:
        lo = 0 if spec.get("big") else -hi
        p["inp"] = ints((M, C), dev, seed + 1, lo, hi) + (mu if gnspec is not None else 0)
        p["w1"] = ints((C, C), dev, seed + 2, lo, hi)
        p["b1"] = ints((C,), dev, seed + 3, -8, 8)
        if spec.get("res"):
            p["res"] = ints((M, C), dev, seed + 4, -8, 8)
    if n2:
        p["w2"] = ints((n2 * C, C), dev, seed + 5, -spec.get("w2hi", 3), spec.get("w2hi", 3))
        if spec.get("rot_thirds", 0):
            hd, rd, tokens, off = spec["rot"]
            p["rot"] = dict(table=dyadic_table(max(M, tokens) + off, rd, dev, seed + 6), tokens=tokens, off=off, head_dim=hd, rot_dim=rd,
                            thirds=spec["rot_thirds"])
    for k in ("inp", "w1", "res", "w2"):
        if p.get(k) is not None:
            assert torch.equal(r16(p[k], dt), p[k]), f"{k} not exact in the storage type"
    return p


R0, R1, R2, R3, R4 = (40, 32, 56, 0), (40, 32, 56, 24), (80, 32, 200, 8), (160, 64, 96, 0), (64, 64, 40, 3)


def _c(M, n2=0, res=None, h_out=True, rt=0, st=0, rot=R0, **kw):
    return dict(M=M, n2=n2, res=res, h_out=h_out, rot_thirds=rt, scale_thirds=st, rot=rot, **kw)


# big: non-negative operands up to 6 -- h sits near 2900, where its store rounds most elements (the n2 = 0 cases: h is all they store)
# res: None, "sep" (its own tensor) or "alias" (h is written over it).  h_out False: h is not stored (the non-FULL instantiation).
ROWCHAIN_EXACT = [
    # ---- the chain without norms
    _c(1, big=True, hi=6), _c(1, 1, h_out=False, rt=1, st=1), _c(1, 3, "sep", rt=3, st=0, rot=R3),
    _c(95, 1, "sep", rt=1, st=0), _c(95, 2, "alias", rt=0, st=0), _c(95, 3, h_out=False, rt=2, st=2, rot=R4),
    _c(96, 0, "alias", big=True, hi=6), _c(96, 3, "alias", rt=2, st=1), _c(96, 3, h_out=False, rt=0, st=3), _c(96, 2, "sep", rt=2, st=1, rot=R4),
    _c(97, 0, big=True, hi=6), _c(97, 2, "sep", rt=2, st=2, rot=R1), _c(97, 3, "sep", h_out=False, rt=1, st=2, rot=R1), _c(97, 1, "alias", rt=1, st=1, rot=R2),
    _c(192, 0, big=True, hi=6), _c(192, 3, "sep", rt=3, st=1, rot=R2), _c(192, 3, "sep", h_out=False, rt=3, st=1, rot=R2),
    _c(192, 1, "alias", rt=0, st=1), _c(192, 2, h_out=False, rt=1, st=2, rot=R3), _c(192, 3, rt=1, st=3, rot=R1),
    _c(200, 0, "sep", big=True, hi=6), _c(200, 3, "sep", rt=2, st=1, rot=R1), _c(200, 3, "alias", rt=1, st=3, rot=R4),
    _c(200, 2, h_out=False, rt=2, st=0, rot=R2), _c(200, 1, rt=1, st=0, rot=R3),
    # ---- GroupNorm, both forms: (form, B, rows_per_batch, groups, replicas)
    _c(96, 1, gn=("stats", 1, 96, 32, 1)), _c(96, 1, gn=("fx", 1, 96, 8, 3), st=1),
    _c(192, 2, gn=("stats", 2, 96, 8, 1), rt=1, st=1), _c(192, 1, gn=("fx", 2, 96, 32, 1)),
    _c(200, 1, gn=("stats", 2, 100, 32, 1), st=1), _c(200, 2, gn=("fx", 2, 100, 8, 3), rt=2, st=1, rot=R1), _c(200, 1, gn=("fx", 2, 100, 32, 1), h_out=False),
    _c(312, 1, gn=("stats", 3, 104, 8, 1), h_out=False), _c(312, 3, gn=("fx", 3, 104, 32, 3), rt=2, st=1, rot=R2, w2hi=2),      # (W2 in [-2, 2]: the rotation by (2, 1) of 300 000 elements would pass 60 000)
    _c(384, 1, gn=("stats", 2, 192, 32, 1), res="sep"), _c(384, 1, gn=("fx", 2, 192, 8, 3), h_out=False, st=1),
    # ---- LayerNorm behind a signed-permutation W1
    _c(96, 3, ln=True, rt=2, st=1, w2hi=31), _c(97, 3, ln=True, rt=2, st=1, rot=R1, w2hi=31), _c(200, 3, ln=True, h_out=False, rt=1, st=2, rot=R4, w2hi=31),
    # ---- GroupNorm, LayerNorm, rotary and scale together: the engine's first chain
    _c(200, 3, gn=("stats", 2, 100, 32, 1), ln=True, rt=2, st=1, rot=R1, w2hi=31),
    _c(312, 3, gn=("fx", 3, 104, 32, 3), ln=True, rt=2, st=1, w2hi=31),
]


for _i, _s in enumerate(ROWCHAIN_EXACT):
    # a seed per case; the FULL / non-FULL pair at M = 192 (n2 = 3, same rotary) keeps identical operands on purpose
    _s["seed"] = 7 if (_s["M"], _s["n2"], _s["rot_thirds"], _s["res"]) == (192, 3, 3, "sep") else 10 + _i


def rowchain_id(s):
    gn = s.get("gn")
    return (f"M{s['M']}-n{s['n2']}-res_{s['res']}-h{int(s['h_out'])}-rot{s['rot_thirds']}x{'_'.join(map(str, s['rot']))}-sc{s['scale_thirds']}"
            + (f"-gn_{gn[0]}_{gn[1]}x{gn[2]}_g{gn[3]}_r{gn[4]}" if gn else "") + ("-ln" if s.get("ln") else "") + ("-big" if s.get("big") else ""))


def exact_ff(spec, dt, dev):
    """one Part 1 problem of ff_fused.  h: balanced +-1 rows (directly, or through the prologue: Wo a signed permutation, a = 2 s p,
    h = -p - bo, so h + a Wo^T + bo = p).  LN(h) = +-gamma + beta: integers of magnitude 1..4.  W1 value rows hold `nv` entries of +-1 and
    a bias in [-2, 2]; gate rows hold `ng` entries of +-1 and a bias of 8 + 4 ng (gates >= 8), except every eighth, which is all zero
    with bias 0 (gate exactly 0).  small: |y| <= 256 and an integer (the column sums are exact integers)"""
    M, seed, small = spec["M"], 7000 + spec["M"], spec.get("small", False)
    nv, ng = (1, 0) if small else (2, 2)
    p = dict(eps=1e-5)
    pat = balanced_rows(M, dev, seed)
    if spec.get("pre"):
        wo, perm, s = signed_permutation(dev, seed + 1)
        bo = ints((C,), dev, seed + 2, -2, 2)
        a = torch.empty((M, C), dtype=f64, device=dev)
        a[:, perm] = 2 * pat * s
        p["pre"], p["h"] = (a, wo, bo), -pat - bo
    else:
        p["h"] = pat
    gamma = signs((C,), dev, seed + 3)
    p["gamma"], p["beta"] = gamma, ints((C,), dev, seed + 4, 2, 3) * signs((C,), dev, seed + 5)
    g = _gen(seed + 6)
    w1 = torch.zeros((2 * INNER, C), dtype=f64)
    b1 = torch.zeros((2 * INNER,), dtype=f64)
    i = torch.arange(INNER)
    for e in range(nv):
        k = (7 * i + 3) % C if e == 0 else ((7 * i + 3) + 1 + torch.randint(0, C - 1, (INNER,), generator=g)) % C
        w1[i, k] += (torch.randint(0, 2, (INNER,), generator=g) * 2 - 1).to(f64)
    b1[:INNER] = torch.randint(-2, 3, (INNER,), generator=g).to(f64)
    live = (i % 8) != 5
    for e in range(ng):
        k = (11 * i + 5) % C if e == 0 else ((11 * i + 5) + 1 + torch.randint(0, C - 1, (INNER,), generator=g)) % C
        w1[INNER + i[live], k[live]] += (torch.randint(0, 2, (int(live.sum()),), generator=g) * 2 - 1).to(f64)
    b1[INNER:][live] = 8.0 + 4 * ng
    p["w1"], p["b1"] = w1.to(dev), b1.to(dev)
    if small:
        wcat = torch.zeros((C, C + INNER), dtype=f64)
        n = torch.arange(C)
        for e in range(2):
            wcat[n, torch.randint(0, C, (C,), generator=g)] = (torch.randint(0, 2, (C,), generator=g) * 2 - 1).to(f64)
        for e in range(4):                                                 # column 320 + 4 n + e: every inner column is read once
            wcat[n, C + 4 * n + e] = (torch.randint(0, 2, (C,), generator=g) * 2 - 1).to(f64)
        p["wcat"] = wcat.to(dev)
    else:
        p["wcat"] = ints((C, C + INNER), dev, seed + 7)
    p["bcat"], p["x"] = ints((C,), dev, seed + 8, -8, 8), ints((M, C), dev, seed + 9, -8, 8)
    return p


# ------------------------------------------------------------------------------------------- the N(0, 1) problems (Part 2)
def _randn(shape, dev, seed, scale=1.0):
    return (torch.randn(shape, generator=_gen(seed), dtype=f64) * scale).to(dev)


def batch_rows(B, rows_pb, dev, seed, amp):
    """[B * rows_pb, 320]: batch element b is N(b, (2^b)^2) * amp, so foreign statistics are an O(1) error in a row"""
    return torch.cat([(_randn((rows_pb, C), dev, seed + b) * 2.0 ** b + b) * amp for b in range(B)], 0)


def stats_of(x16, B, rows_pb, groups, form, reps, dev, seed):
    """the statistics a producer would leave for x (float64 holding 16-bit values): per-group (sum, sum of squares) stored as fp32, or
    per-channel fixed-point sums spread over `reps` replicas unevenly, parts of both signs"""
    xb = x16.reshape(B, rows_pb, C)
    gn = dict(form=form, count=float(rows_pb * (C // groups)), groups=groups, rows_pb=rows_pb, eps=1e-6)
    if form == "stats":
        s = xb.sum(1).reshape(B, groups, -1).sum(-1)
        q = xb.pow(2).sum(1).reshape(B, groups, -1).sum(-1)
        gn["stats"] = torch.stack([s, q], -1).to(f32).to(f64)
    else:
        tot = torch.stack([xb.sum(1), xb.pow(2).sum(1)], 1)                # [B, 2, 320]
        tot = (tot * (1 << FX_SHIFT)).round().to(torch.int64)
        r = torch.randint(1 << 24, 1 << 28, (B, 2, C), generator=_gen(seed)).to(dev)
        gn["fx"] = torch.stack([tot + r, -2 * r, r][:reps] if reps == 3 else [tot], 0)
    return gn


def random_rowchain(dt, dev, *, M, gn=None, ln=True, n2=3, res=False, amp=1.0, rot=None, seed=0, same_dist=False):
    """a Part 2 problem: operands N(0, 1) x amp rounded to the storage type, weights N(0, 1/320); gn = (form, B, rows_pb, groups, reps).
    same_dist: every batch element N(0.3, 1.5^2), the data of tests/test_gpu_rowchain.py (the mutation table's contrast)"""
    p = dict(col_scale=40 ** -0.5 * 1.4426950408889634, scale_thirds=1)
    if gn is not None:
        form, B, rows_pb, groups, reps = gn
        p["inp"] = r16(_randn((M, C), dev, seed + 1, 1.5) + 0.3 if same_dist else batch_rows(B, rows_pb, dev, seed + 1, amp), dt)
        p["gn"] = stats_of(p["inp"], B, rows_pb, groups, form, reps, dev, seed + 20)
        p["gn"]["gamma"] = 1.0 + 0.2 * _randn((C,), dev, seed + 2)
        p["gn"]["beta"] = 0.2 * _randn((C,), dev, seed + 3)
        for k in ("gamma", "beta"):
            p["gn"][k] = p["gn"][k].to(f32).to(f64)
    else:
        p["inp"] = r16(_randn((M, C), dev, seed + 1, amp), dt)
    p["w1"] = r16(_randn((C, C), dev, seed + 4, C ** -0.5), dt)
    p["b1"] = (0.1 * _randn((C,), dev, seed + 5)).to(f32).to(f64)
    if res:
        p["res"] = r16(_randn((M, C), dev, seed + 6, amp), dt)
    if ln:
        p["ln"] = ((1.0 + 0.2 * _randn((C,), dev, seed + 7)).to(f32).to(f64), (0.2 * _randn((C,), dev, seed + 8)).to(f32).to(f64), 1e-5)
    p["w2"] = r16(_randn((n2 * C, C), dev, seed + 9, C ** -0.5), dt)
    if rot is not None:
        p["rot"] = rot
    return p


def random_ff(dt, dev, *, M, pre=False, amp=1.0, B=1, seed=0):
    p = dict(eps=1e-5)
    p["h"] = r16(batch_rows(B, M // B, dev, seed + 1, amp), dt)
    p["x"] = r16(_randn((M, C), dev, seed + 2, amp), dt)
    if pre:
        p["pre"] = (r16(_randn((M, C), dev, seed + 11, amp), dt), r16(_randn((C, C), dev, seed + 12, C ** -0.5), dt),
                    (0.1 * _randn((C,), dev, seed + 13)).to(f32).to(f64))
    p["gamma"] = (1.0 + 0.2 * _randn((C,), dev, seed + 3)).to(f32).to(f64)
    p["beta"] = (0.1 * _randn((C,), dev, seed + 4)).to(f32).to(f64)
    p["w1"] = r16(_randn((2 * INNER, C), dev, seed + 5, C ** -0.5), dt)
    p["b1"] = (0.2 * _randn((2 * INNER,), dev, seed + 6)).to(f32).to(f64)
    p["wcat"] = r16(_randn((C, C + INNER), dev, seed + 7, (C + INNER) ** -0.5), dt)
    p["bcat"] = (0.2 * _randn((C,), dev, seed + 8)).to(f32).to(f64)
    return p


def real_rotary_table(rows, rot_dim, dev):
    """cos / sin of pos * 10000^(-2 i / rot_dim) as fp32, what seer_rotary_table holds up to its own rounding (tested elsewhere); the
    tests pass THIS tensor to the kernel, so it is a stored operand"""
    freqs = 10000.0 ** (-torch.arange(0, rot_dim, 2, dtype=f64) / rot_dim)
    ang = torch.arange(rows, dtype=f64)[:, None] * freqs[None, :]
    return torch.stack([ang.cos(), ang.sin()], -1).to(f32).to(dev)


ROWCHAIN_ROWS = [   # Part 2: (gn or None, M, res in place, rotary offset)
    (("stats", 1, 96, 32, 1), 96, False, 0), (("fx", 1, 96, 32, 3), 96, False, 24),
    (("stats", 3, 104, 32, 1), 312, False, 24), (("fx", 3, 104, 32, 3), 312, False, 0),
    (("stats", 2, 200, 32, 1), 400, False, 0), (("fx", 2, 200, 32, 3), 400, False, 24),
    (None, 97, True, None), (None, 1000, True, None),
]
FF_EXACT = [  # Part 1: M, prologue, y aliasing x, column sums: None | ("fx", rows per batch element, replicas) | "tiles"
    (1, False, False, None), (1, True, True, None), (96, False, True, None), (96, True, False, None), (97, False, False, None), (97, True, True, None),
    (200, False, True, None), (200, True, False, None), (288, False, False, None), (288, True, True, None), (336, True, False, None),
    (1008, False, False, None),
    (336, False, False, ("fx", 112, 8)),      # boundaries inside tiles 1 and 2 at different 16-row segments, a ragged last tile
    (336, True, True, ("fx", 112, 3)),
    (1008, False, True, ("fx", 112, 8)),      # 11 tiles: the 8 replicas wrap
    (1008, True, False, ("fx", 1008, 2)),
    (96, False, False, "tiles"), (288, True, True, "tiles"),
]


def rows_rowchain_problem(dt, dev, gn, M, res, off, amp, table_rows=None, make_table=None):
    """one case of ROWCHAIN_ROWS: with GroupNorm the engine's first chain (q | k | v, rotary on two thirds from a real table, the q
    prescale), without it the second (to_out + residual in place -> norm2 -> to_q).  make_table(rows, rot_dim, dev): the GPU file passes
    seer_rotary_table's output, the CPU file takes real_rotary_table; either way the table is a stored operand"""
    rot = None
    if gn is not None:
        tokens = gn[2]
        rot = dict(table=(make_table or real_rotary_table)(table_rows or tokens + off, 32, dev), tokens=tokens, off=off, head_dim=40, rot_dim=32, thirds=2)
    return random_rowchain(dt, dev, M=M, gn=gn, n2=3 if gn is not None else 1, res=res, amp=amp, rot=rot, seed=int(amp) * 100 + M)


FF_ROWS = [(96, False), (96, True), (200, False), (200, True), (336, False), (336, True)]


# ------------------------------------------------------------------------------------------- gn_fx chain against gn_stats chain
FX_STATS_CASES = [(B, rows_pb, amp) for B, rows_pb in ((1, 96), (3, 104), (2, 200)) for amp in (1.0, 4.0)]
_ULPS = [(km, kv) for km in (-1, 0, 1) for kv in (-1, 0, 1) if (km, kv) != (0, 0)]
_yardstick = {}


def fx_stats_problems(dt, dev, B, rows_pb, amp, make_table=None):
    """the same x through the chain with (sum, sum of squares) per group and with the producer's fixed-point sums in 3 replicas"""
    ps = rows_rowchain_problem(dt, dev, ("stats", B, rows_pb, 32, 1), B * rows_pb, False, 0, amp, make_table=make_table)
    pf = dict(ps)
    pf["gn"] = dict(stats_of(ps["inp"], B, rows_pb, 32, "fx", 3, dev, 77), gamma=ps["gn"]["gamma"], beta=ps["gn"]["beta"])
    return ps, pf


def row_diff(a, b, ref64):
    """worst own row of |a - b|_2 over max(|ref|_2, floor)"""
    return float(((a.to(f64) - b.to(f64)).norm(dim=-1) / ref64.norm(dim=-1).clamp_min(row_floor(ref64))).max())


def fx_stats_yardstick(dt, dev, make_table=None):
    """{"h", "out"}: how far two correct realisations of the statistics' fp32 arithmetic can put a row apart, from the emulation alone.
    The two forms give scale and shift that differ by a relative 1e-7; that moves an output only where it flips a 16-bit rounding of
    GN(x), and the flip then moves its whole row.  Flips are rare events (none at all in most single cases), so they are SAMPLED: per
    case the fx emulation and the stats emulation with its fp32 (mean, var) moved by every combination of -1, 0, +1 ulp, each against
    the unmoved stats emulation, and the worst row over all FX_STATS_CASES of the storage type.  Computed once per storage type"""
    key = (dt, str(dev))
    if key not in _yardstick:
        worst = dict(h=0.0, out=0.0)
        for B, rows_pb, amp in FX_STATS_CASES:
            ps, pf = fx_stats_problems(dt, dev, B, rows_pb, amp, make_table)
            ref, base = rowchain(ps), rowchain(ps, dt)
            variants = [rowchain(pf, dt)]
            for u in _ULPS:
                pu = dict(ps)
                pu["gn"] = dict(ps["gn"], ulps=u)
                variants.append(rowchain(pu, dt))
            for v in variants:
                for k in worst:
                    worst[k] = max(worst[k], row_diff(v[k], base[k], ref[k]))
        _yardstick[key] = worst
    return _yardstick[key]
