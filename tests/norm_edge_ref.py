"""References, emulations and exact constructions for csrc/norm.hip (the GroupNorm entry points, seer_layernorm, seer_softmax_rows) and
csrc/elementwise.hip (rotary, timestep embedding, seer_linear_smallm, seer_conv_in / seer_conv_out, cast and layout,
seer_conv1x1_nchw_f32, seer_clamp01, seer_gaussian_sample) with the DDIM step boundary of csrc/sampler_step.hip.  Plain torch in float64 on whatever device the operands live; no
dependency on the library and nothing here comes from a kernel's output.  Used by tests/test_gpu_norm_matrix.py and
tests/test_gpu_edge_matrix.py (the kernels) and tests/test_norm_edge_ref_cpu.py (the preconditions and the mutation table, no GPU).

Every function has up to three modes, as tests/fused320_ref.py:
  reference (dt = None)        the operator in float64 on the stored operands;
  emulation (dt = bf16 / f16)  the same with one rounding to fp32 or to the storage type exactly where the kernels round, as read from
                               the sources: GroupNorm's one-pass q / n - mean^2 in fp32 (gn_apply_kernel) or through one conversion
                               from the 64-bit sums in double (gn_apply_cs_kernel<FX>), scale = rstd * gamma and shift = beta - mean *
                               scale in fp32; LayerNorm's two passes with the rounded 1 / C; softmax's exp of the scaled difference
                               and ONE reciprocal of the row sum;
  exact (Part 1)               integer or dyadic operands on which the fp32 arithmetic is exact, and at rsqrtf the absorption
                               construction of fused320_ref.assert_absorbed; every precondition is asserted here, case by case.

`mut` applies one of MUTATIONS to the emulation: the kernel bugs the matrices must be able to see."""
import math

import torch

from tests import fused320_ref as R

f16, bf16, f32, f64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
i64 = torch.int64
FX_SHIFT = R.FX_SHIFT
MUTATIONS = ["stats_miss_last_row_block", "count_off_by_one_row", "neighbour_batch_stats", "neighbour_group_stats", "straddle_to_first_group",
             "skip_replica_or_phase", "skip_second_column_pass", "ln_stats_miss_last_8", "ln_neighbour_row_stats", "softmax_sum_miss_chunk",
             "softmax_max_first_512", "rot_no_offset", "rot_no_modulo", "rot_pair_plus1", "cfg_offset_fp", "cfg_no_cond_f",
             "conv_in_frame_batch_exchanged", "smallm_tail_row_stored"]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def r32(x64):
    """one round-to-nearest-even to fp32, back in float64"""
    return x64.to(f32).to(f64)


def ulps32(x64, k):
    """x (float64 holding fp32 values) moved by k fp32 ulps"""
    x = x64.to(f32)
    for _ in range(abs(k)):
        x = torch.nextafter(x, torch.full_like(x, float("inf") if k > 0 else float("-inf")))
    return x.to(f64)


def silu64(x):
    return x / (1.0 + torch.exp(-x))


# =========================================================================================== GroupNorm: the launch geometries
def gn_geom(C, B, rows):
    """gn_geom of csrc/norm.hip: (columns per pass, row lanes, rows per block, row blocks per batch element)"""
    ncols = C // 8
    cpp = min(ncols, 256)
    rows_par = 256 // cpp
    rpb = (rows * B + 1023) // 1024
    rpb = max(-(-rpb // rows_par) * rows_par, rows_par)
    if rpb > 64:
        rpb = 64 // rows_par * rows_par
    rpb = max(rpb, 1)
    return cpp, rows_par, rpb, -(-rows // rpb)


def gn_cs_geom(C, G, B, rows, target=512):
    """gn_cs_geom: (slice channels, row lanes, rows per block, row blocks) or None where the one-launch forms refuse the layout"""
    cpg = C // G
    sc = next((k * cpg for k in range(1, 128 // cpg + 1) if k * cpg >= 64 and k * cpg % 8 == 0 and G % k == 0), 0)
    if not sc or sc // cpg > 16:
        return None
    nrb = max(target // (B * (C // sc)), 1)
    rows_par = 256 // (sc // 8)
    rpb = max(-(-(-(-rows // nrb)) // rows_par) * rows_par, rows_par)
    return sc, rows_par, rpb, -(-rows // rpb)


def fx_rows_per_block(C, B, rows):
    """seer_groupnorm_stats_fx's rows per block"""
    rpb = 256
    while rpb > 16 and B * (-(-rows // rpb)) * ((C // 8 + 63) // 64) < 512:
        rpb >>= 1
    while -(-rows // rpb) > 64:
        rpb <<= 1
    return rpb


# =========================================================================================== GroupNorm statistics (Part 1)
# (B, rows, C1, C2, G)
GN_STATS_SHAPES = [(1, 1, 64, 0, 8), (2, 7, 128, 0, 32), (2, 100, 320, 0, 32), (3, 45, 640, 320, 32), (1, 9, 2560, 0, 32), (1, 5, 2056, 0, 8),
                   (1, 2100, 64, 0, 8), (2, 33, 512, 0, 64)]
GN_APPLY_EXTRA = [(2, 96, 1280, 1280, 32), (2, 61, 288, 0, 32), (2, 40, 512, 0, 32)]
GN_APPLY_SHAPES = GN_STATS_SHAPES + GN_APPLY_EXTRA


def gn_id(s):
    return "B{}-r{}-C{}+{}-G{}".format(*s)


def gn_means(B, G, dev, seed):
    """m(b, g): distinct integers around 0"""
    return (torch.randperm(B * G, generator=_gen(seed)).to(f64) - (B * G) // 2).reshape(B, G).to(dev)


def gn_exact_x(B, rows, C, G, dev, seed):
    """x [B, rows, C] = integers in [-3, 3] + m(b, g): a wrong batch element or group changes both sums"""
    m = gn_means(B, G, dev, seed)
    x = R.ints((B, rows, C), dev, seed + 1) + m.repeat_interleave(C // G, 1)[:, None, :]
    q = x.pow(2).reshape(B, rows, G, -1).sum((1, 3))
    assert float(q.max()) < 2 ** 24, "GroupNorm statistics: a sum of squares reaches 2^24 (and the sums lie below it)"
    assert float(x.abs().max()) <= 256, "x not exact in bf16"
    return x, m


def gn_sums(x, G, mut=None, last_block=None):
    """[B, G, 2] float64 (sum, sum of squares) of x [B, rows, C]; `mut`: what a wrong statistics kernel would leave.  last_block: first
    row of the last row block (from the launch geometry).  None where the mutation does not apply"""
    B, rows, C = x.shape
    cpg = C // G
    if mut == "stats_miss_last_row_block":
        x = x[:, :last_block]
    elif mut == "skip_second_column_pass":
        if C <= 2048:
            return None
        x = torch.cat([x[..., :2048], torch.zeros_like(x[..., 2048:])], -1)
    ch = torch.arange(C, device=x.device)
    grp = ch // cpg
    if mut == "straddle_to_first_group":
        if cpg % 8 == 0:
            return None
        grp = (ch // 8 * 8) // cpg
    onehot = torch.zeros((C, G), dtype=f64, device=x.device)
    onehot[ch, grp] = 1.0
    st = torch.stack([x.sum(1) @ onehot, x.pow(2).sum(1) @ onehot], -1)
    if mut == "neighbour_batch_stats":
        return None if B == 1 else st.roll(1, 0)
    if mut == "neighbour_group_stats":
        return st.roll(1, 1)
    if mut in (None, "stats_miss_last_row_block", "skip_second_column_pass", "straddle_to_first_group"):
        return st
    return None


COLSUM_LAYOUTS = [(1, 1), (4, 3), (1, 40), (2, 17)]       # (phases, tiles per batch element)


def colsum_partials(phases, tpb, B, C, G_hint, dev, seed):
    """synthetic [phases][B * tpb][C][2] integer partials in the layout of seer_gemm_desc::colsum (include/seer_hip.h): batch element b
    owns tiles b * tpb .. (b + 1) * tpb - 1 of every phase; values are small integers + a distinct offset per (b, 8-channel block)"""
    v = R.ints((phases, B, tpb, C, 2), dev, seed, -3, 3)
    off = gn_means(B, C // 8, dev, seed + 1).repeat_interleave(8, 1)
    v = v + off[None, :, None, :, None]
    return v.reshape(phases, B * tpb, C, 2)


def colsums_to_stats(sources, B, G, mut=None, exact=True):
    """stats [B, G, 2] from a list of partial tensors (concatenated along the channels), float64; every partial sum stays below 2^24.
    skip_replica_or_phase drops the last phase of every source that has two, else its last tile per batch element"""
    if mut not in (None, "skip_replica_or_phase", "neighbour_batch_stats", "neighbour_group_stats"):
        return None
    tot, bound, dropped = [], [], False
    for cs in sources:
        ph, tiles, C, _ = cs.shape
        v = cs.reshape(ph, B, tiles // B, C, 2)
        bound.append(v.abs().sum((0, 2)))
        if mut == "skip_replica_or_phase" and ph > 1:
            v, dropped = v[:-1], True
        elif mut == "skip_replica_or_phase" and tiles // B > 1:
            v, dropped = v[:, :, :-1], True
        tot.append(v.sum((0, 2)))
    if mut == "skip_replica_or_phase" and not dropped:
        return None
    assert not exact or float(torch.cat(bound, 1).reshape(B, G, -1, 2).sum(2).max()) < 2 ** 24, "a partial sum of the column sums can reach 2^24"
    st = torch.cat(tot, 1).reshape(B, G, -1, 2).sum(2)
    if mut == "neighbour_batch_stats":
        return None if B == 1 else st.roll(1, 0)
    if mut == "neighbour_group_stats":
        return st.roll(1, 1)
    return st


FX_SHAPES = [(8, 1, 1), (72, 100, 3), (520, 300, 2), (320, 16385, 1)]      # (C, rows, B)


def fx_sums(x, mut=None, last_block=None):
    """[B, 2, C] int64: sums of round(v 2^20) and round(v v 2^20) per (batch element, column) of x [B, rows, C] (float64 holding 16-bit
    values: v v is exact in fp32 and in float64, the products with 2^20 are exact, the rounding is to nearest even in both)"""
    if mut == "stats_miss_last_row_block":
        x = x[:, :last_block]
    elif mut == "neighbour_batch_stats":
        if x.shape[0] == 1:
            return None
        x = x.roll(1, 0)
    elif mut is not None:
        return None
    k = float(1 << FX_SHIFT)
    return torch.stack([(x * k).round().to(i64).sum(1), (x * x * k).round().to(i64).sum(1)], 1)


# =========================================================================================== GroupNorm apply
def exact_gn(form, B, G, C, dev, seed, reps=1, parts=1, m=None, splits=None):
    """fused320_ref.exact_gn for any C: statistics the TEST supplies -- mean m(b, g) a distinct integer, variance 1, count 1024 (1 / count
    and every product with it exact in fp32).  gamma a signed integer 1..3, beta an odd multiple of 1/2.
    form 'stats': stats [B, G, 2] = (m count, (1 + m^2) count);
    form 'fx':    fx [reps, B, 2, C] int64, uneven parts of both signs that add to the same totals times 2^20;
    form 'cs':    cs [1, B * parts, C, 2] float64 integer partials of both signs that add to them, every partial sum below 2^24.
    splits: channel counts of the sources (C1, C2): fx and cs are returned as one tensor per source"""
    count, cpg = 1024.0, C // G
    if m is None:
        m = gn_means(B, G, dev, seed)
    tot = torch.stack([m * count, (1 + m * m) * count], -1)               # [B, G, 2]
    assert float(tot.abs().max()) < 2 ** 24
    gn = dict(form=form, count=count, groups=G, eps=1e-6, m=m, totals=tot)
    gn["gamma"] = R.ints((C,), dev, seed + 2, 1, 3) * R.signs((C,), dev, seed + 3)
    gn["beta"] = (2 * R.ints((C,), dev, seed + 4, -3, 3) + 1) * 0.5
    cuts = [0, C] if not splits or not splits[1] else [0, splits[0], C]
    if form == "stats":
        gn["stats"] = tot
    elif form == "fx":
        p = torch.randint(-(1 << 34), 1 << 34, (reps, B, 2, G, cpg), generator=_gen(seed + 1)).to(dev)
        p[0, :, :, :, 0] += (tot.transpose(1, 2) * (1 << FX_SHIFT)).to(i64) - p.sum((0, 4))
        p = p.reshape(reps, B, 2, C)
        assert bool((p < 0).any()) and bool((p > 0).any())
        gn["fx"] = [p[..., a:b].contiguous() for a, b in zip(cuts[:-1], cuts[1:])]
    else:
        p = torch.randint(-1024, 1025, (B, parts, G, cpg, 2), generator=_gen(seed + 1)).to(dev).to(f64)
        p[:, 0, :, 0, :] += tot - p.sum((1, 3))
        assert float(p.abs().sum((1, 3)).max()) < 2 ** 24, "a partial sum of the column sums can reach 2^24"
        p = p.reshape(1, B * parts, C, 2)
        gn["cs"] = [p[:, :, a:b].contiguous() for a, b in zip(cuts[:-1], cuts[1:])]
    return gn


def gn_moments(gn, mode, mut=None, cpg=None):
    """(mean, var) [B, G] float64 from the statistics a launch is given.  mode 'ref': float64, 1 / count exact.  mode 'kernel':
    inv_count = (float)(1 / count); forms 'stats' and 'cs' in fp32 (mean = s inv, var = q inv - mean^2), form 'fx' with one conversion per
    group in double.  None where `mut` does not apply"""
    count = gn["count"]
    if mut == "count_off_by_one_row":
        count = count - cpg
    inv32 = float(torch.tensor(1.0 / count, dtype=f32))
    B, G = gn["m"].shape if "m" in gn else gn["shape"]
    if gn["form"] == "fx":
        srcs = gn["fx"]
        if mut == "skip_replica_or_phase":
            if all(s.shape[0] < 2 for s in srcs):
                return None
            srcs = [s[:-1] if s.shape[0] > 1 else s for s in srcs]
        tot = torch.cat([s.sum(0) for s in srcs], -1)                        # [B, 2, C] int64
        grp = tot.reshape(B, 2, G, -1).sum(-1).to(f64)
        k = (1.0 / count if mode == "ref" else inv32) / float(1 << FX_SHIFT)
        mean = grp[:, 0] * k
        var = (grp[:, 1] * k - mean * mean).clamp_min(0)
        if mode == "kernel":
            mean, var = r32(mean), r32(var)
    else:
        if gn["form"] == "cs":
            st = colsums_to_stats(gn["cs"], B, G, mut if mut == "skip_replica_or_phase" else None, exact=False)
            if st is None:
                return None
        else:
            if mut == "skip_replica_or_phase":
                return None
            st = gn["stats"]
        s, q = st[..., 0], st[..., 1]
        if mode == "ref":
            mean = s / count
            var = (q / count - mean * mean).clamp_min(0)
        else:
            mean = r32(r32(s) * inv32)
            var = r32(r32(r32(q) * inv32) - r32(mean * mean)).clamp_min(0)
    if mut == "neighbour_batch_stats":
        if B == 1:
            return None
        mean, var = mean.roll(1, 0), var.roll(1, 0)
    if mut == "neighbour_group_stats":
        mean, var = mean.roll(1, 1), var.roll(1, 1)
    return mean, var


GN_MUTS = ("count_off_by_one_row", "neighbour_batch_stats", "neighbour_group_stats", "skip_replica_or_phase", "skip_second_column_pass")


def gn_apply(x, gn, dt=None, silu=False, exact=False, mut=None, info=None):
    """GroupNorm of x [B, rows, C] with the statistics of `gn`, float64.  emulation: scale = rstd gamma, shift = beta - mean scale,
    x scale + shift, each rounded to fp32, SiLU in float64, one rounding to the storage type.  exact: the preconditions of the
    absorption construction are asserted and the target returned.  skip_second_column_pass (seer_groupnorm_apply only: the caller
    decides) leaves NaN, the prefill, in the columns from 2048 on"""
    assert not (exact and (dt is None or mut is not None or silu))
    if mut is not None and mut not in GN_MUTS:
        return None
    B, rows, C = x.shape
    G = gn["groups"]
    cpg = C // G
    if mut == "skip_second_column_pass" and C <= 2048:
        return None
    mom = gn_moments(gn, "ref" if dt is None else "kernel", None if mut == "skip_second_column_pass" else mut, cpg)
    if mom is None:
        return None
    mean, var = [t.repeat_interleave(cpg, 1)[:, None, :] for t in mom]
    gamma, beta = gn["gamma"], gn["beta"]
    if exact:
        assert bool((var == 1).all()) and bool((mean == mean.round()).all()), "exact GroupNorm: mean an integer, variance 1"
        assert mom[0].unique().numel() == mom[0].numel(), "exact GroupNorm: the means of all (batch element, group) must differ"
        rstd = (var + gn["eps"]).rsqrt().expand_as(x)
        target = (x - mean) * gamma + beta
        R.assert_absorbed(x - mean, rstd, gamma.expand_as(x), beta.expand_as(x), target, dt, "GN(x)")
        # the kernel computes x sc + (beta - mean sc), not (x - mean) sc + beta: its own order is evaluated below in float32, with the
        # product and the sum rounded separately and fused, and must round to the same target
        assert float(x.abs().max()) <= 256 and float(target.abs().max()) <= 16
        for k in (-4, 0, 4):
            sc = r32(ulps32(r32(rstd), k) * gamma)
            for o in (r32(r32(x * sc) + r32(beta - r32(mean * sc))), r32(x * sc + r32(beta - r32(mean * sc)))):      # separate and fused
                assert torch.equal(R.r16(o, dt), target), f"GN(x): the kernel's own order with rstd {k:+d} ulp is not absorbed"
        return target
    rstd = (var + gn["eps"]).rsqrt()
    if dt is None:
        o = (x - mean) * rstd * gamma + beta
        return silu64(o) if silu else o
    sc = r32(r32(rstd) * gamma)
    sh = r32(beta - r32(mean * sc))
    o = r32(r32(x * sc) + sh)
    if info is not None:
        info["pre"] = o
    o = R.r16(silu64(o) if silu else o, dt)
    if mut == "skip_second_column_pass":
        o = o.clone()
        o[..., 2048:] = float("nan")
    return o


def seg_err(got, ref, cpg):
    """Part 2's judged unit for GroupNorm: the worst (row, group) segment, |got - ref|_2 / max(|ref|_2, floor)"""
    g, r = got.to(f64).reshape(-1, cpg), ref.reshape(-1, cpg)
    return R.row_err(g, r, R.row_floor(r))


def gn_random(B, rows, C, G, dt, dev, seed, amp, ratio=None):
    """x [B, rows, C] rounded to the storage type: batch element b is N(b, 4^b) amp, group g gets the offset (g % 5 - 2) 2^b amp; with
    `ratio` every group sits at mean = ratio sd instead (the cancellation of q / n - mean^2).  gamma 1 + 0.2 N, beta 0.2 N as fp32"""
    cpg = C // G
    x = torch.stack([(R._randn((rows, C), dev, seed + b) * 2.0 ** b + b) * amp for b in range(B)], 0)
    goff = ((torch.arange(G, device=dev) % 5 - 2).to(f64)).repeat_interleave(cpg)
    x = x + goff * amp * (2.0 ** torch.arange(B, device=dev, dtype=f64))[:, None, None]
    if ratio is not None:
        x = torch.stack([(R._randn((rows, C), dev, seed + b) + ratio) * amp * 2.0 ** b for b in range(B)], 0)
    gamma = r32(1.0 + 0.2 * R._randn((C,), dev, seed + 50))
    beta = r32(0.2 * R._randn((C,), dev, seed + 51))
    return R.r16(x, dt), gamma, beta


def stats_of(x16, G, form, dev, seed, reps=3, tile_rows=16):
    """the statistics a producer leaves for x16 [B, rows, C] (float64 holding 16-bit values): 'stats' as fp32, 'fx' spread unevenly over
    `reps` replicas, 'cs' per tile of `tile_rows` rows as fp32"""
    B, rows, C = x16.shape
    gn = dict(form=form, count=float(rows * (C // G)), groups=G, eps=1e-6, shape=(B, G))
    if form == "stats":
        gn["stats"] = r32(gn_sums(x16, G))
    elif form == "fx":
        tot = fx_sums(x16)
        r = torch.randint(1 << 24, 1 << 28, tuple(tot.shape), generator=_gen(seed)).to(dev)
        gn["fx"] = [torch.stack([tot + r, -2 * r, r][:reps] if reps == 3 else [tot], 0)]
    else:
        pad = (-rows) % tile_rows
        xp = torch.cat([x16, torch.zeros((B, pad, C), dtype=f64, device=dev)], 1).reshape(B, -1, tile_rows, C)
        gn["cs"] = [r32(torch.stack([xp.sum(2), xp.pow(2).sum(2)], -1).reshape(1, -1, C, 2))]
    return gn


# =========================================================================================== LayerNorm
LN_CS = [8, 64, 320, 504, 512, 520, 1024, 1032, 1280, 1536]
LN_ROWS = [1, 5, 1000]
LN_LONG = [(16389, 8), (16389, 520)]          # blocks are capped at 4096: four rows per block, so rows above 16384 take the grid-stride loop


def ln_affine(C, dev, seed, gmax=3, extra=5):
    """fused320_ref.ln_affine for any C: gamma a signed integer in 1..gmax, beta a signed integer with |gamma| < |beta| <= |gamma| + extra"""
    gamma = R.ints((C,), dev, seed, 1, gmax) * R.signs((C,), dev, seed + 1)
    beta = (gamma.abs() + R.ints((C,), dev, seed + 2, 1, extra)) * R.signs((C,), dev, seed + 3)
    return gamma, beta


def ln_exact_x(rows, C, dev, seed):
    """row r = m(r) +- 1, C / 2 of each at seeded places; m(r) = r % 251 - 125: distinct among any 251 consecutive rows (m +- 1 has to stay
    exact in bf16, so no more distinct values exist)"""
    order = torch.rand((rows, C), generator=_gen(seed)).argsort(-1)
    pm = ((order < C // 2).to(f64) * 2 - 1).to(dev)
    m = (torch.arange(rows, device=dev) % 251 - 125).to(f64)
    return pm + m[:, None], pm, m


def layernorm(x, gamma, beta, eps, dt=None, exact=False, mut=None, k_mean=0, k_rstd=0, info=None):
    """LayerNorm of the rows of x, float64.  emulation (layernorm_kernel): invC = (float)(1 / C); mean = fl(sum) invC; d = x - mean;
    rstd = rsqrt(fl(sum d^2) invC + eps); ((d rstd) gamma) + beta, each step rounded to fp32 (the sums themselves in float64: their order
    is the kernel's business), one rounding to the storage type.  k_mean / k_rstd move the fp32 mean and rstd by that many ulps"""
    assert not (exact and (dt is None or mut is not None))
    rows, C = x.shape
    if mut not in (None, "ln_stats_miss_last_8", "ln_neighbour_row_stats"):
        return None
    if dt is None:
        mean = x.mean(-1, keepdim=True)
        d = x - mean
        return d * (d.pow(2).mean(-1, keepdim=True) + eps).rsqrt() * gamma + beta
    invC = float(torch.tensor(1.0, dtype=f32) / torch.tensor(float(C), dtype=f32))
    xs = x[:, :C - 8] if mut == "ln_stats_miss_last_8" else x
    if mut == "ln_stats_miss_last_8" and C == 8:
        return None
    mean = ulps32(r32(r32(xs.sum(-1, keepdim=True)) * invC), k_mean)
    d = r32(x - mean)
    ds = d[:, :C - 8] if mut == "ln_stats_miss_last_8" else d
    rstd = ulps32(r32((r32(r32(r32(ds * ds).sum(-1, keepdim=True)) * invC) + float(torch.tensor(eps, dtype=f32))).rsqrt()), k_rstd)
    if mut == "ln_neighbour_row_stats":
        if rows == 1:
            return None
        mean, rstd = mean.roll(1, 0), rstd.roll(1, 0)
        d = r32(x - mean)
    o = r32(r32(r32(d * rstd) * gamma) + beta)
    if info is not None:
        info["pre"] = o
    return R.r16(o, dt)


def ln_exact(x, pm, gamma, beta, eps, dt):
    """the Part 1 target +-gamma + beta with its preconditions: non-zero, representable, and the kernel's fp32 order -- rounded 1 / C
    included -- with mean and rstd each moved by -4, 0, +4 ulp rounds to it"""
    rows, C = x.shape
    target = pm * gamma + beta
    assert bool((beta.abs() > gamma.abs()).all()) and bool((target != 0).all())
    assert torch.equal(R.r16(target, dt), target) and torch.equal(R.r16(x, dt), x)
    assert bool((pm.sum(-1) == 0).all()) and float(x.abs().sum(-1).max()) < 2 ** 24
    sample = x if rows <= 64 else x[torch.linspace(0, rows - 1, 64).long().to(x.device)]     # (rows differ by m(r) only: 64 spread rows carry every |m| class)
    tsample = target if rows <= 64 else target[torch.linspace(0, rows - 1, 64).long().to(x.device)]
    for km in (-4, 0, 4):
        for kr in (-4, 0, 4):
            assert torch.equal(layernorm(sample, gamma, beta, eps, dt, k_mean=km, k_rstd=kr), tsample), \
                f"LayerNorm C{C}: mean {km:+d} ulp, rstd {kr:+d} ulp (with the rounded 1 / C) is not absorbed by the 16-bit rounding"
    return target


def ln_random(rows, C, dt, dev, seed, amp):
    """rows N(r % 7 - 3, 4^(r % 3)) amp: neighbouring rows differ in mean and spread"""
    r = torch.arange(rows, device=dev)
    x = (R._randn((rows, C), dev, seed) * (2.0 ** (r % 3).to(f64))[:, None] + (r % 7 - 3).to(f64)[:, None]) * amp
    return R.r16(x, dt), r32(1.0 + 0.2 * R._randn((C,), dev, seed + 1)), r32(0.2 * R._randn((C,), dev, seed + 2))


# =========================================================================================== softmax rows
SM_NS = [8, 64, 520, 1024, 1032, 2048, 2056, 4096]
SM_ROWS = [1, 5, 300]
SM_LOW = -32768.0


def softmax_exact(rows, n, dev, seed):
    """x [rows, n]: row r holds k = 2^(r % (log2 n + 1)) entries 0 at seeded places and -32768 elsewhere; row 0 (k = 1) has its entry in
    the LAST column, so a sum that misses the last chunk or a maximum over a prefix cannot pass.  -> x, the exact result"""
    jmax = int(math.log2(n))
    j = torch.arange(rows) % (jmax + 1)
    order = torch.rand((rows, n), generator=_gen(seed)).argsort(-1)
    order[0] = torch.arange(n - 1, -1, -1)
    hit = order < (2 ** j)[:, None]
    x = torch.where(hit, 0.0, SM_LOW).to(f64).to(dev)
    want = torch.where(hit, (0.5 ** j.to(f64))[:, None], 0.0).to(f64).to(dev)
    return x, want


def softmax_rows(x, scale, dt=None, mut=None):
    """softmax(x scale) per row, float64.  emulation (softmax_rows_kernel): v = fl(x scale), e = fl(exp(v - max)), inv = fl(1 / fl(sum e)),
    fl(e inv), one rounding to the storage type"""
    if mut not in (None, "softmax_sum_miss_chunk", "softmax_max_first_512"):
        return None
    rows, n = x.shape
    if dt is None:
        return torch.softmax(x * scale, -1)
    v = r32(x * r32(torch.tensor(scale, dtype=f64)))
    if mut == "softmax_max_first_512":
        if n <= 512:
            return None
        mx = v[:, :512].max(-1, keepdim=True).values
    else:
        mx = v.max(-1, keepdim=True).values
    e = r32(torch.exp(r32(v - mx)))
    if mut == "softmax_sum_miss_chunk":
        if n == 8:
            return None
        s = r32(e[:, :n - 8].sum(-1, keepdim=True))
    else:
        s = r32(e.sum(-1, keepdim=True))
    return R.r16(r32(e * r32(1.0 / s)), dt)


def softmax_random(rows, n, spread, in_dt, dev, seed):
    """scores whose SCALED values (scale 0.125) have standard deviation `spread`, row r shifted by 3 (r % 5 - 2) spreads, the LAST column
    raised by 2 spreads (so that the last chunk carries weight at either spread); stored as in_dt"""
    r = torch.arange(rows, device=dev)
    x = R._randn((rows, n), dev, seed) + 3.0 * (r % 5 - 2).to(f64)[:, None]
    x[:, -1] += 2.0
    x = x * spread * 8.0
    return x.to(in_dt).to(f64)


# =========================================================================================== rotary in place
# (rows, heads, head_dim, rot_dim, tokens_per_batch, pos_offset, ld)
ROTARY_CASES = [(7, 8, 40, 32, 7, 0, 960), (10, 12, 40, 32, 4, 3, 1448 + 8), (5, 5, 64, 64, 5, 0, 968), (9, 8, 160, 8, 3, 5, 3848)]
ROT_COL0 = 8


def rotary_inplace(buf, case, table, mut=None):
    """buf [rows * ld + tail] (flat, float64): the q and k thirds start at column 8 and 8 + heads head_dim of every row; the first rot_dim
    channels of every head are rotated in interleaved pairs by table[row % tokens + off].  Returns the whole buffer: everything else
    keeps its value"""
    rows, heads, hd, rd, tokens, off, ld = case
    if mut not in (None, "rot_no_offset", "rot_no_modulo", "rot_pair_plus1"):
        return None
    if (mut == "rot_no_offset" and off == 0) or (mut == "rot_no_modulo" and rows <= tokens):
        return None
    out = buf.clone()
    r = torch.arange(rows, device=buf.device)
    pos = (r if mut == "rot_no_modulo" else r % tokens) + (0 if mut == "rot_no_offset" else off)
    cs = table[pos].to(f64)                                                # [rows, rd / 2, 2]
    if mut == "rot_pair_plus1":
        cs = cs.roll(-1, 1)
    c, s = cs[:, None, :, 0], cs[:, None, :, 1]
    for col0 in (ROT_COL0, ROT_COL0 + heads * hd):
        idx = (r[:, None, None] * ld + col0 + torch.arange(heads, device=buf.device)[None, :, None] * hd
               + torch.arange(0, rd, 2, device=buf.device)[None, None, :])
        x0, x1 = buf[idx], buf[idx + 1]
        out[idx] = x0 * c - x1 * s
        out[idx + 1] = x1 * c + x0 * s
    return out


def unet_freqs(half, dev):
    """the UNet's rotary frequencies 10000^(-2 j / rot_dim) as fp32"""
    return (10000.0 ** (-torch.arange(0, 2 * half, 2, dtype=f32) / (2 * half))).to(dev)


def rotary_table_ref(freqs32, T):
    """(float64 cos | sin of the fp32 product float(pos) freqs[j], the angle): one IEEE multiplication, formed here as the kernel forms it"""
    ang = (torch.arange(T, dtype=f32, device=freqs32.device)[:, None] * freqs32[None, :]).to(f64)
    return torch.stack([ang.cos(), ang.sin()], -1), ang


def sincos_allowance(ang64):
    """4 x the worst error of torch's own float32 sin / cos on these angles (on the CPU) against float64, not below 2^-23"""
    a = ang64.cpu()
    a32 = a.to(f32)
    worst = max(float((a32.sin().to(f64) - a.sin()).abs().max()), float((a32.cos().to(f64) - a.cos()).abs().max()))
    return max(4 * worst, 2.0 ** -23), worst


# =========================================================================================== timestep embedding
TE_DIMS, TE_TS = [2, 320, 1280], [0, 1, 751, 999]
LN10000 = 9.210340371976184


def timestep_embedding(t, dim, flip, shift):
    """diffusers get_timestep_embedding in float64 -> (out [B, dim], |arg| [B, half], |expo| [half]); the constant is the kernel's fp32 one"""
    half = dim // 2
    c = float(torch.tensor(-LN10000, dtype=f32))
    expo = c * torch.arange(half, dtype=f64, device=t.device) / (half - shift)
    arg = t.to(f64)[:, None] * torch.exp(expo)[None, :]
    out = torch.cat([arg.cos(), arg.sin()] if flip else [arg.sin(), arg.cos()], -1)
    return out, arg.abs(), expo.abs()


def timestep_allowance(arg, expo):
    """|arg| (|expo| + 4) 2^-23 + 2^-22 per element: two roundings on the exponent amplified by exp, expf, the product, sincosf"""
    a = arg * (expo[None, :] + 4) * 2.0 ** -23 + 2.0 ** -22
    return torch.cat([a, a], -1)


def timestep_embedding_f32(t, dim, flip, shift):
    """a float32 emulation in the kernel's order (torch's float32 exp / sin / cos on the CPU stand in for expf / sincosf)"""
    half = dim // 2
    j = torch.arange(half, dtype=f32)
    expo = (torch.tensor(-LN10000, dtype=f32) * j) / (torch.tensor(float(half), dtype=f32) - torch.tensor(float(shift), dtype=f32))
    arg = t.cpu().to(f32)[:, None] * torch.exp(expo)[None, :]
    return torch.cat([arg.cos(), arg.sin()] if flip else [arg.sin(), arg.cos()], -1)


# =========================================================================================== seer_linear_smallm
SMALLM_CASES = [(1, 8, 1), (2, 320, 1280), (2, 520, 777), (3, 320, 7), (5, 1280, 1283), (8, 1032, 16), (8, 8, 9)]      # (B, K, N)
GUARD = 64


def smallm_exact(B, K, N, dev, seed):
    x, w, b = R.ints((B, K), dev, seed), R.ints((N, K), dev, seed + 1), R.ints((N,), dev, seed + 2, -8, 8)
    assert K * 9 + 8 < 2 ** 24 and (B == 1 or x.unique(dim=0).shape[0] == B or K < 16)
    return x, w, b


def linear_smallm(x, w, bias, silu_in=False, silu_out=False, mut=None):
    """[B * N + GUARD] float64: the output arena (NaN prefill kept in the guard).  smallm_tail_row_stored: a wave whose ROWS output
    features reach past N stores the clamped feature N - 1 at the index past the row -- into the next batch row, and behind the last
    one into the guard"""
    B, K = x.shape
    N = w.shape[0]
    if mut not in (None, "smallm_tail_row_stored"):
        return None
    y = (silu64(x) if silu_in else x) @ w.t() + (bias if bias is not None else 0)
    if silu_out:
        y = silu64(y)
    arena = torch.full((B * N + GUARD,), float("nan"), dtype=f64, device=x.device)
    arena[:B * N] = y.reshape(-1)
    if mut is not None:
        rows_per_wave = 4 if B <= 2 else 2
        if N % rows_per_wave == 0:
            return None
        for n in range(N, -(-N // rows_per_wave) * rows_per_wave):
            arena[(B - 1) * N + n] = y[B - 1, N - 1]
    return arena


# =========================================================================================== conv_in / conv_out
CONV_IN_CASES = [(2, 4, 3, 5, 7, 320), (1, 3, 1, 1, 9, 128), (1, 4, 2, 6, 1, 8), (1, 2, 1, 3, 3, 1824), (1, 4, 1, 3, 3, 1104), (2, 1, 2, 4, 4, 2048)]
CONV_IN_REFUSED = (1, 4, 1, 3, 3, 1824)       # 9 Cin Cout floats of weights alone are 256.5 KiB: above the 160 KiB a workgroup can have
CONV_OUT_CASES = [(2, 8, 3, 5, 7), (1, 128, 1, 1, 9), (2, 320, 2, 6, 1), (1, 64, 1, 3, 3)]


def conv_in_lds_bytes(Cin, Cout):
    return (9 * Cin * Cout + 32 * 9 * Cin) * 4


def conv_in(x, w_khwc, bias, mut=None):
    """x [B, Cin, F, H, W], weights [3][3][Cin][Cout], float64 -> channels-last [B F H W, Cout]"""
    B, Cin, F, H, W = x.shape
    if mut not in (None, "conv_in_frame_batch_exchanged"):
        return None
    img = x.permute(0, 2, 1, 3, 4).reshape(B * F, Cin, H, W)
    if mut is not None:
        if B == 1 or F == 1:
            return None
        i = torch.arange(B * F, device=x.device)
        img = x[i % B, :, i // B]                                         # image b F + f read as (b, f) = (i % B, i / B)
    y = torch.nn.functional.conv2d(img, w_khwc.permute(3, 2, 0, 1), bias, padding=1)
    return y.permute(0, 2, 3, 1).reshape(B * F * H * W, -1)


def conv_out(x, w_ohwc, bias, B, F, H, W):
    """x channels-last [B F H W, C0], weights [Cout][3][3][C0], float64 -> [B, Cout, F, H, W]"""
    C0 = x.shape[1]
    y = torch.nn.functional.conv2d(x.reshape(B * F, H, W, C0).permute(0, 3, 1, 2), w_ohwc.permute(0, 3, 1, 2), bias, padding=1)
    return y.reshape(B, F, -1, H, W).permute(0, 2, 1, 3, 4).contiguous()


# =========================================================================================== the DDIM step boundary
STEP_BEGIN_CASES = [(1, 4, 0, 3, 5, 1), (2, 4, 2, 3, 6, 2), (3, 1, 1, 1, 1, 2), (2, 4, 1, 5, 300, 2)]      # (b, C, f1, Fp, HW, reps)
CFG_CASES = [(1, 4, 3, 0, 5), (2, 4, 7, 2, 64), (3, 1, 2, 1, 1), (2, 4, 5, 2, 300)]                       # (b, C, Ft, cond_f, HW)
CFG_EXACT_COEF = [(1.0, 1.0, 0.0, 1.0), (1.0, 0.0, 0.0, 1.0), (1.0, 0.0, 1.0, 0.0), (0.25, 1.0, 0.0, 2.0)]


def cfg_problem(case, cfg, dev, seed, exact=True):
    """eps [reps b, C, Ft, HW] with NaN in the conditioning frames, x and noise [b, C, Fp, HW]"""
    b, C, Ft, cond_f, HW = case
    reps, Fp = (2 if cfg else 1), Ft - cond_f
    if exact:
        eps, x, noise = R.ints((reps * b, C, Ft, HW), dev, seed, -8, 8), R.ints((b, C, Fp, HW), dev, seed + 1, -8, 8), R.ints((b, C, Fp, HW), dev, seed + 2, -8, 8)
    else:
        eps, x, noise = R._randn((reps * b, C, Ft, HW), dev, seed), R._randn((b, C, Fp, HW), dev, seed + 1), R._randn((b, C, Fp, HW), dev, seed + 2)
        eps, x, noise = r32(eps), r32(x), r32(noise)
    eps[:, :, :cond_f] = float("nan")
    return eps, x, noise


def cfg_ddim(eps, x, noise, coef_row, cfg, scale, case, mut=None):
    """(x_prev, pred_x0) of seer_cfg_ddim_step in float64; the mutations gather eps from the flat buffer as a wrong kernel would"""
    b, C, Ft, cond_f, HW = case
    Fp = Ft - cond_f
    if mut not in (None, "cfg_offset_fp", "cfg_no_cond_f"):
        return None
    if (mut == "cfg_offset_fp" and (not cfg or cond_f == 0)) or (mut == "cfg_no_cond_f" and cond_f == 0):
        return None
    flat = eps.reshape(-1)
    bi, c, f, hw = torch.meshgrid(*[torch.arange(n, device=x.device) for n in (b, C, Fp, HW)], indexing="ij")
    eoff = ((bi * C + c) * Ft + f + (0 if mut == "cfg_no_cond_f" else cond_f)) * HW + hw
    e = flat[eoff]
    if cfg:
        ec = flat[eoff + b * C * (Fp if mut == "cfg_offset_fp" else Ft) * HW]
        e = e + scale * (ec - e)
    a_t, a_prev, sigma, s1m = [float(v) for v in coef_row]
    x0 = (x - s1m * e) / math.sqrt(a_t)
    xp = math.sqrt(a_prev) * x0 + math.sqrt(max(1.0 - a_prev - sigma * sigma, 0.0)) * e + (sigma * noise if noise is not None else 0.0)
    return xp, x0


def cfg_ddim_allowance(eps, x, noise, coef_row, cfg, scale, case):
    """per element, from the fp32 operations of the formula.  Each of the three terms of x_prev -- sqrt(a_prev) x0, the direction term and
    sigma noise -- is reached through a chain of at most 11 roundings (the CFG pair's difference, product and sum; s1m e, x - ., the
    division, sqrtf(a_t); the coefficient of the direction term, 1 - a_prev - sigma^2 and its sqrtf, at 0.35 of its operands; the
    products and the two final sums), each at most 2^-24 of a magnitude that the sum of the operands' magnitudes bounds:
    12 x 2^-24 x that sum, for x_prev and for pred_x0"""
    b, C, Ft, cond_f, HW = case
    ev = eps[:, :, cond_f:]
    a_t, a_prev, sigma, s1m = [float(v) for v in coef_row]
    mag = (ev[:b].abs() + (scale + 1) * (ev[b:] - ev[:b]).abs() + ev[b:].abs()) if cfg else ev.abs()
    x0m = (x.abs() + s1m * mag) / math.sqrt(a_t)
    tot = math.sqrt(a_prev) * x0m + math.sqrt(max(1.0 - a_prev - sigma * sigma, 0.0)) * mag + (sigma * noise.abs() if noise is not None else 0.0)
    return 12 * 2.0 ** -24 * tot + 2.0 ** -126, 12 * 2.0 ** -24 * x0m + 2.0 ** -126


def gaussian_sample(mom, noise):
    """DiagonalGaussianDistribution.sample: mean + exp(0.5 clamp(logvar, -30, 20)) noise, float64; moments [N, 2 C, HW]"""
    C = mom.shape[1] // 2
    mean, logvar = mom[:, :C], mom[:, C:]
    return mean if noise is None else mean + torch.exp(0.5 * logvar.clamp(-30.0, 20.0)) * noise


# =========================================================================================== what the oldest tests read
def old_close(got, ref, atol=2e-2, rtol=2e-2):
    """tests/test_gpu_kernels.py::_close: the number of elements outside atol + rtol |ref| (NaN counts as outside)"""
    err = (got - ref).abs()
    return int((~(err <= atol + rtol * ref.abs())).sum())
