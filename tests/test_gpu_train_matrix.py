"""The training kernels (csrc/attention_bwd.hip, csrc/gemm_tn.hip, csrc/train.hip) tested as hard as the inference ones in
test_gpu_f16_matrix.py.  tests/test_train_kernels.py compares one relative L2 number per tensor against fp32 autograd on the GPU: a
wrong tail tile seen by four queries of a thousand, one wrong output column or one wrong image row is invisible there.  Three parts:

1. EXACT arithmetic: integer inputs keep every product and partial sum an integer (or an integer multiple of a power of two) below
   2^24, so the fp32 result is exact whatever the slice order and the one rounding of a bf16 output is fully determined.  Zero
   tolerance for gemm_tn (single and grouped), colsum, sumpool2x, zero_insert2x, add, colfinal_grouped, and for seer_attn_bwd on a
   uniform softmax (Q = 0: P = 1/Sk, dK = 0, dV and dQ one rounding each).
2. Attention backward PER OWN ROW -- one (batch, head, token) vector of head_dim values -- against float64 autograd.  The allowance is
   derived, not guessed: a float64 emulation that rounds where the kernels round (O to bf16 before delta, P and dS to bf16 before the
   second pair of products, the outputs to bf16; and the two roundings of the FORWARD launch that O and lse come from: its P to bf16
   before P V, and at head_dim 40 q * scale * log2(e) to bf16 before the scores, include/seer_hip.h at SEER_ATTN_Q_PRESCALED) is
   measured against the unrounded gradient, and the kernel gets 2x the emulation's worst row (the project's margin for bf16
   emulations, tests/test_gpu_clip_text.py).  Nothing in the bound comes from the kernel.
3. The remaining train.hip kernels element by element against float64 with derived bounds: one bf16 rounding of the output
   (2^-8 |ref|) plus the fp32 accumulation term (additions on the longest path x 2^-24 x the sum of the magnitudes added).

Arguments the trainer passes, or the entry points accept, that no other kernel test passes -- each is in an assertion below:
  dres2 (test_groupnorm_bwd_elementwise, test_groupnorm_bwd_dres2_alone) . strided dres and dout (test_layernorm_bwd_strided,
  test_geglu_strided) . the unclipped AdamW step, p_bf16 = None, grad_sumsq = None, weight_decay = 0, a late step
  (test_adamw_against_float64) . H != W (test_conv_out_bwd_elementwise, test_exact_sumpool_zero_insert) . cond_f = 0
  (test_mse_loss_grad_elementwise) . causal_offset > 0 (test_attn_bwd_rows_causal_offset) . the NaN sentinels (_attn_run: every
  Part 2 case; test_exact_gemm_tn*, test_layernorm_bwd_strided, test_geglu_strided).

All references are plain torch in float64 on inputs already rounded to their storage type.  Measured values, the file's run time and
the mutation table: profiles/train_matrix.md."""
import math

import pytest
import torch
import torch.nn.functional as Fn

from tests.test_gpu_f16_matrix import _eq, _exact_pre, _ints, _rand, _store

pytestmark = pytest.mark.gpu

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
U16 = 2.0 ** -8          # unit roundoff of bf16 (8 significand bits, round to nearest even)
U32 = 2.0 ** -24         # ... of fp32
LOG2E = 1.4426950408889634
NAN16 = 0x7FC0           # the bits torch.full(..., nan, dtype=bfloat16) writes
HEAD_DIMS = [40, 80, 96, 160]
EINVAL, ENOSYS = r"\(-22\)", r"\(-38\)"


def _r16(x64):
    """one round-to-nearest-even to bf16, back in float64"""
    return x64.to(bf16).to(f64)


def _bound(got, ref64, allow, what):
    """|got - ref| <= allow element by element (allow: float64 tensor like ref, derived by the caller)"""
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    g = got.to(f64)
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    err = (g - ref64).abs()
    bad = err > allow
    if bool(bad.any()):
        idx, flat = [], int((err - allow).flatten().argmax())
        for n in reversed(err.shape):
            idx.insert(0, flat % n)
            flat //= n
        idx = tuple(idx)
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements outside the bound; worst at {idx}: got {g[idx].item()!r} "
                             f"ref {ref64[idx].item()!r} allowed {allow[idx].item():.3g}")
    return float((err / allow.clamp_min(1e-300)).max())


def _gapped(t, fill=float("nan")):
    """t [rows, cols] -> (buffer [rows + 1, cols + 16] of `fill`, its view [:rows, 8:8 + cols] holding t): a row-strided column slice
    with a column offset, spare columns on both sides and a guard row behind the last one"""
    rows, cols = t.shape
    buf = torch.full((rows + 1, cols + 16), fill, device=t.device, dtype=t.dtype)
    view = buf[:rows, 8:8 + cols]
    view.copy_(t)
    return buf, view


def _gaps_hold(buf, rows, cols, what):
    """everything of a _gapped NaN buffer outside the view still holds its NaN bits"""
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    keep[:rows, 8:8 + cols] = False
    bits = buf.view(torch.int16)[keep] if buf.dtype == bf16 else None
    if bits is not None:
        assert bool((bits == NAN16).all()), f"{what}: a store outside the slice ({int((bits != NAN16).sum())} elements)"
    else:
        assert bool(buf[keep].isnan().all()), f"{what}: a store outside the slice"


# =========================================================================================== 1. exact arithmetic
GUARD = 64
_TN_SHAPES = [  # M, N, K, split
    (64, 128, 128, False),       # all four wave quadrants of one 128 x 128 tile
    (1000, 136, 72, True),       # ragged N and K, four slices with a ragged last one
    (72, 8, 264, False),         # ragged, three column tiles
    (1, 136, 72, False), (63, 72, 136, False), (65, 136, 72, False), (129, 8, 264, False),     # around the 64-row LDS tile
    (520, 136, 72, True),        # three slices of 192, 192 and 136 rows
]


def _tn_problem(dev, M, N, K, seed, colsum=True):
    """operands as row-strided views with a column offset; out and colsum NaN-filled slices of ONE arena with a neighbour tensor directly
    behind each"""
    a64f, b64f = _ints((M, N + 8), dev, seed), _ints((M, K + 16), dev, seed + 1)
    a, b = _store(a64f, bf16)[:, :N], _store(b64f, bf16)[:, 8:8 + K]
    arena = torch.full((N * K + GUARD + N + GUARD,), float("nan"), device=dev, dtype=f32)
    out = arena[:N * K].view(N, K)
    cs = arena[N * K + GUARD:N * K + GUARD + N]
    arena[N * K:N * K + GUARD] = -7.25
    arena[-GUARD:] = -7.25
    _exact_pre(M, 3, 3)
    return dict(a=a, b=b, out=out, cs=cs if colsum else None, arena=arena, ref=a64f[:, :N].t() @ b64f[:, 8:8 + K], ref_cs=a64f[:, :N].sum(0),
                shape=(M, N, K))


def _tn_check(p, what):
    M, N, K = p["shape"]
    _eq(p["out"], p["ref"], bf16, f"{what} {p['shape']} out")
    if p["cs"] is not None:
        _eq(p["cs"], p["ref_cs"], bf16, f"{what} {p['shape']} colsum")
    else:
        assert bool(p["arena"][N * K + GUARD:N * K + GUARD + N].isnan().all()), f"{what} {p['shape']}: colsum = NULL was written"
    g1, g2 = p["arena"][N * K:N * K + GUARD], p["arena"][-GUARD:]
    assert bool((g1 == -7.25).all()) and bool((g2 == -7.25).all()), f"{what} {p['shape']}: the neighbour behind out / colsum changed"


@pytest.mark.parametrize("M,N,K,split", _TN_SHAPES)
def test_exact_gemm_tn(device, M, N, K, split):
    """dW = dY^T X and the bias gradient bit for bit: a dropped or doubled contraction row, a slice that is not added, a store past N or
    K cannot hide"""
    from seervideoldm_amd import _lib, train_ops
    assert (_lib.load().seer_gemm_tn_workspace_bytes(M, N, K) != 0) == split, "the shape no longer takes the path it was chosen for"
    p = _tn_problem(device, M, N, K, 1)
    train_ops.gemm_tn(p["a"], p["b"], out=p["out"], colsum=p["cs"])
    _tn_check(p, "gemm_tn")
    p = _tn_problem(device, M, N, K, 3, colsum=False)
    train_ops.gemm_tn(p["a"], p["b"], out=p["out"])
    _tn_check(p, "gemm_tn, no colsum")


@pytest.mark.parametrize("group_rows", [None, 64, 128])
def test_exact_gemm_tn_grouped(device, monkeypatch, group_rows):
    """the same problems alone and together, at the library's group_rows and at 64 / 128 rows per workgroup (slices of every problem
    above that meet in the workspace), plus one whose contraction exceeds the default 16384.  Exact, hence equal to the single form"""
    from seervideoldm_amd import train_ops
    if group_rows is None:
        monkeypatch.delenv("SEER_TN_GROUP_ROWS", raising=False)
    else:
        monkeypatch.setenv("SEER_TN_GROUP_ROWS", str(group_rows))
    shapes = [s[:3] for s in _TN_SHAPES] + [(16500, 8, 8)]
    for M, N, K in shapes:                                                   # alone
        p = _tn_problem(device, M, N, K, 5)
        train_ops.gemm_tn_grouped([(p["a"], p["b"], p["out"], p["cs"])])
        _tn_check(p, f"grouped alone, group_rows {group_rows}")
    probs = [_tn_problem(device, M, N, K, 7 + 2 * i, colsum=i % 2 == 0) for i, (M, N, K) in enumerate(shapes)]
    train_ops.gemm_tn_grouped([(p["a"], p["b"], p["out"], p["cs"]) for p in probs])
    for p in probs:
        _tn_check(p, f"grouped together, group_rows {group_rows}")


@pytest.mark.parametrize("rows,cols", [(1, 8), (7, 8), (77, 72), (1000, 136), (130, 2056)])
def test_exact_colsum(device, rows, cols):
    """bias gradients: one row, fewer rows than row lanes, ragged chunks, two column blocks (2056 = 257 owners of 8 columns)"""
    from seervideoldm_amd import train_ops
    x64 = _ints((rows, cols + 16), device, 1)
    x = _store(x64, bf16)[:, 8:8 + cols]
    _exact_pre(rows, 3, 1)
    out = torch.full((cols,), float("nan"), device=device, dtype=f32)
    train_ops.colsum(x, out=out)
    _eq(out, x64[:, 8:8 + cols].sum(0), bf16, f"colsum {rows}x{cols}")


@pytest.mark.parametrize("n_img,H,W,C", [(3, 4, 6, 64), (2, 1, 5, 8), (2, 5, 1, 8), (1, 1, 1, 8), (2, 3, 2, 72)])
def test_exact_sumpool_zero_insert(device, n_img, H, W, C):
    """H != W, H = 1, W = 1, C = 8.  sumpool2x on integers in [128, 255]: the sums lie in [512, 1020] where a bf16 ulp is 4, so three in
    four elements are rounded and one in four is a tie -- pins round-to-nearest-even.  zero_insert2x moves bits"""
    from seervideoldm_amd import train_ops
    du64 = _ints((n_img * 4 * H * W, C), device, 1, 128, 255)
    ref = du64.reshape(n_img, H, 2, W, 2, C).sum((2, 4)).reshape(n_img * H * W, C)
    if ref.numel() >= 64:
        assert (_r16(ref) != ref).double().mean() > 0.5, "the store must round most elements"
    _eq(train_ops.sumpool2x(_store(du64, bf16), n_img, H, W), ref, bf16, f"sumpool2x {n_img}x{H}x{W}x{C}")
    d = _rand((n_img * H * W, C), device, 2).to(bf16)
    z = train_ops.zero_insert2x(d, n_img, H, W).reshape(n_img, 2 * H, 2 * W, C)
    want = torch.zeros_like(z)
    want[:, ::2, ::2] = d.reshape(n_img, H, W, C)
    assert torch.equal(z.view(torch.int16), want.view(torch.int16)), f"zero_insert2x {n_img}x{H}x{W}x{C}"


@pytest.mark.parametrize("rows,cols", [(1, 8), (300, 640), (33, 72)])
def test_exact_add(device, rows, cols):
    """gradient fan-in on strided views, into a strided view: integers up to 255 (exact in bf16), sums up to 510 (ulp 2: odd sums round)"""
    from seervideoldm_amd import train_ops
    a64, b64 = _ints((rows, cols), device, 1, -255, 255), _ints((rows, cols), device, 2, -255, 255)
    _, a = _gapped(_store(a64, bf16))
    _, b = _gapped(_store(b64, bf16))
    obuf, out = _gapped(torch.zeros((rows, cols), device=device, dtype=bf16))
    if a64.numel() >= 64:
        assert (_r16(a64 + b64) != a64 + b64).double().mean() > 0.1
    train_ops.add(a, b, out=out)
    _eq(out, a64 + b64, bf16, f"add {rows}x{cols}")
    _gaps_hold(obuf, rows, cols, "add")


def test_exact_colfinal_grouped(device):
    """the slab sums of many norms in one launch, NV = 1 and 2, one slab, 16 and 17 (the k lanes), C off the 64-column block; an
    output that is NULL is skipped and its neighbour is still right"""
    from seervideoldm_amd import train_ops
    items, want = [], []
    for i, (n, NV, Cc) in enumerate([(1, 1, 8), (16, 1, 200), (17, 2, 64), (37, 2, 200), (100, 2, 8), (3, 1, 72), (5, 2, 136)]):
        s64 = _ints((n, NV, Cc), device, i, -1000, 1000)
        _exact_pre(n, 1000, 1)
        outs = [torch.full((Cc,), float("nan"), device=device, dtype=f32) for _ in range(NV)]
        if i == 4:
            outs[0] = None
        items.append((s64.to(f32).reshape(-1), n, NV, Cc, outs[0], outs[1] if NV == 2 else None))
        want.append((outs, s64.sum(0)))
    train_ops.colfinal_grouped(items)
    for (outs, ref), it in zip(want, items):
        for v, o in enumerate(outs):
            if o is not None:
                _eq(o, ref[v], bf16, f"colfinal_grouped n{it[1]} NV{it[2]} C{it[3]} v{v}")


@pytest.mark.parametrize("Sq,Sk", [(100, 64), (200, 256)])
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_exact_attn_bwd_uniform_softmax(device, d, Sq, Sk):
    """Q = 0, not causal, Sk a power of two: lse2 = log2(Sk) and P = 1/Sk exactly.  dK = 0; dV[j] = (1/Sk) sum_i dO[i] for every key, one
    bf16 rounding (dO in [0, 7] so that the sums need more than 8 bits); with scale = 1/8 and V = c + (w, -w) pairs (integer column
    mean c, so O = c and delta = <dO, c> are integers) dS = (dP - delta) / (8 Sk) is exact in bf16 and dQ = dS K is one rounding too.  A
    dropped or doubled 64-query tile, or a clamped duplicate row that escaped its mask, changes an integer"""
    from seervideoldm_amd import ops, train_ops
    B, Hh, scale = 2, 2, 0.125
    C = Hh * d
    kw = dict(batch=B, heads=Hh, head_dim=d, Sq=Sq, Sk=Sk, causal=False, scale=scale)
    to4 = lambda t, S: t.reshape(B, S, Hh, d).permute(0, 2, 1, 3)
    to2 = lambda t, S: t.permute(0, 2, 1, 3).reshape(B * S, C)
    q = torch.zeros((B * Sq, C), device=device, dtype=bf16)
    k64 = _ints((B * Sk, C), device, 1)
    c64 = _ints((B, 1, C), device, 2, -1, 1)
    w64 = _ints((B, Sk // 2, C), device, 3, -1, 1)
    v64 = (c64 + torch.stack([w64, -w64], 2).reshape(B, Sk, C)).reshape(B * Sk, C)
    k, v = _store(k64, bf16), _store(v64, bf16)
    for leg, (lo, hi) in (("dV", (0, 7)), ("dQ", (-1, 1))):
        do64 = _ints((B * Sq, C), device, 4, lo, hi)
        do = _store(do64, bf16)
        out = torch.full((B * Sq, C), float("nan"), device=device, dtype=bf16)
        lse = train_ops.attn_lse_buffer(B, Hh, Sq, device)
        ops.attention(q, k, v, out, lse=lse, **kw)
        assert bool((lse == math.log2(Sk)).all()), "forward: lse2 of a uniform softmax over 2^n keys is not exactly n"
        _eq(out, c64.expand(B, Sq, C).reshape(B * Sq, C), bf16, "forward: O of a uniform softmax is not the column mean")
        dq, dk, dv = [torch.full_like(t, float("nan")) for t in (q, k, v)]
        train_ops.attention_bwd(q, k, v, out, lse, do, dq, dk, dv, **kw)
        do4, k4, v4 = to4(do64, Sq), to4(k64, Sk), to4(v64, Sk)
        _exact_pre(Sq, hi, 1)
        ref_dv = (do4.sum(2, keepdim=True) / Sk).expand(B, Hh, Sk, d)
        if leg == "dV":
            assert (_r16(ref_dv) != ref_dv).double().mean() > 0.25, "the dV store must round"
        _eq(dv, to2(ref_dv, Sk), bf16, f"uniform softmax d{d} {Sq}x{Sk} dV ({leg} leg)")
        assert bool((dk == 0).all()), f"uniform softmax d{d} {Sq}x{Sk}: dK != 0 with Q = 0 ({int((dk != 0).sum())} elements)"
        dp = do4 @ v4.transpose(-1, -2)
        delta = (do4 * to4(c64.expand(B, Sq, C).reshape(B * Sq, C), Sq)).sum(-1, keepdim=True)
        if leg == "dQ":
            assert (dp - delta).abs().max() <= 256, "dP - delta must be exact in bf16"
            _exact_pre(Sk, 256, 3)
            ref_dq = ((dp - delta) * (scale / Sk)) @ k4
            assert ref_dq.abs().max() > 0
            _eq(dq, to2(ref_dq, Sq), bf16, f"uniform softmax d{d} {Sq}x{Sk} dQ")
        else:
            assert bool(torch.isfinite(dq.float()).all())


# =========================================================================================== 2. attention backward, per own row
class _Plain:
    """sequences stored one after the other: rows (batch, token)"""
    def __init__(self, B, Hh, d):
        self.B, self.Hh, self.d = B, Hh, d

    def to4(self, t, S):
        return t.reshape(self.B, S, self.Hh, self.d).permute(0, 2, 1, 3)

    def to2(self, t, S):
        return t.permute(0, 2, 1, 3).reshape(self.B * S, self.Hh * self.d)


class _Strided:
    """FSTextTransformer's attention over frames: rows ordered (frame, token), one sequence per token"""
    def __init__(self, Fr, L, Hh, d):
        self.Fr, self.L, self.Hh, self.d = Fr, L, Hh, d

    def to4(self, t, S):
        return t.reshape(self.Fr, self.L, self.Hh, self.d).permute(1, 2, 0, 3)

    def to2(self, t, S):
        return t.permute(2, 0, 1, 3).reshape(self.Fr * self.L, self.Hh * self.d)


class _Window:
    """temporal window form: rows (batch, frame, y, x), one sequence per (window, batch element)"""
    def __init__(self, B, Fr, H, W, ws, Hh, d):
        self.a = (B, Fr, H, W, ws, Hh, d)

    def to4(self, t, S):
        B, Fr, H, W, ws, Hh, d = self.a
        return t.reshape(B, Fr, H // ws, ws, W // ws, ws, Hh, d).permute(2, 4, 0, 6, 1, 3, 5, 7).reshape(-1, Hh, Fr * ws * ws, d)

    def to2(self, t, S):
        B, Fr, H, W, ws, Hh, d = self.a
        return t.reshape(H // ws, W // ws, B, Hh, Fr, ws, ws, d).permute(2, 4, 0, 5, 1, 6, 3, 7).reshape(B * Fr * H * W, Hh * d)


def _attn_run(dev, lay, Hh, d, tq, tk, kw, seed, qamp=1.0):
    """forward + backward on the sentinel layout: q, k, v, dq, dk, dv are column slices of [tokens + 1, 3C + 16] buffers -- q | 8 spare | k |
    8 spare | v -- whose spare columns, unused slices and guard row hold NaN.  After the call every one of them still holds its NaN bits
    and every gradient element is finite.  Returns the inputs (float64) and the gradients (bf16), all token-major [tokens, C]"""
    from seervideoldm_amd import ops, train_ops
    C = Hh * d
    LD = 3 * C + 16
    cols = [slice(0, C), slice(C + 8, 2 * C + 8), slice(2 * C + 16, 3 * C + 16)]
    nanbuf = lambda tokens: torch.full((tokens + 1, LD), float("nan"), device=dev, dtype=bf16)
    in_q, in_kv, g_q, g_kv = nanbuf(tq), nanbuf(tk), nanbuf(tq), nanbuf(tk)
    q, k, v = in_q[:tq, cols[0]], in_kv[:tk, cols[1]], in_kv[:tk, cols[2]]
    q.copy_((_rand((tq, C), dev, seed) * qamp).to(bf16))
    k.copy_(_rand((tk, C), dev, seed + 1).to(bf16))
    v.copy_(_rand((tk, C), dev, seed + 2).to(bf16))
    do = _rand((tq, C), dev, seed + 3).to(bf16)
    dq, dk, dv = g_q[:tq, cols[0]], g_kv[:tk, cols[1]], g_kv[:tk, cols[2]]
    out = torch.full((tq, C), float("nan"), device=dev, dtype=bf16)
    lse = train_ops.attn_lse_buffer(kw["batch"], Hh, kw["Sq"], dev, window=kw.get("window"))
    before = [t.clone() for t in (in_q, in_kv)]
    ops.attention(q, k, v, out, lse=lse, **kw)
    train_ops.attention_bwd(q, k, v, out, lse, do, dq, dk, dv, **kw)
    for t, b in zip((in_q, in_kv), before):
        assert torch.equal(t.view(torch.int16), b.view(torch.int16)), "the backward wrote into its inputs"
    for buf, tokens, own in ((g_q, tq, cols[:1]), (g_kv, tk, cols[1:])):
        keep = torch.ones(buf.shape, dtype=torch.bool, device=dev)
        for c in own:
            keep[:tokens, c] = False
        bits = buf.view(torch.int16)[keep]
        assert bool((bits == NAN16).all()), f"{int((bits != NAN16).sum())} stores outside the gradient slices (gap columns / guard row)"
    for t, n in ((dq, "dq"), (dk, "dk"), (dv, "dv")):
        assert bool(torch.isfinite(t.float()).all()), f"{n}: non-finite (an element not written, or a read of a spare column)"
    return [t.to(f64) for t in (q, k, v, do)], (dq, dk, dv)


def _attn_f64(q, k, v, do, d, scale, causal, off):
    """[B', heads, S, d] float64 -> (the unrounded gradient by autograd, the emulation that rounds where the kernels round)"""
    Sq, Sk = q.shape[2], k.shape[2]
    vis = None
    if causal:
        i = torch.arange(Sq, device=q.device)[:, None] + off
        vis = torch.arange(Sk, device=q.device)[None, :] <= i
    mask = lambda s: s if vis is None else s.masked_fill(~vis, float("-inf"))
    ql, kl, vl = [t.clone().requires_grad_(True) for t in (q, k, v)]
    (mask(ql @ kl.transpose(-1, -2) * scale).softmax(-1) @ vl).backward(do)
    exact = (ql.grad, kl.grad, vl.grad)
    s2 = mask(q @ k.transpose(-1, -2) * (scale * LOG2E))                      # log2 domain, what the backward rebuilds
    s2f = s2
    if d == 40:     # the d = 40 forward multiplies q by fp32(scale * log2 e) and rounds to bf16 before its scores
        qs = (q.to(f32) * torch.tensor(scale * LOG2E, dtype=f32)).to(bf16).to(f64)
        s2f = mask(qs @ k.transpose(-1, -2))
    m = s2f.max(-1, keepdim=True).values
    p0 = torch.exp2(s2f - m)
    l = p0.sum(-1, keepdim=True)
    lse2 = m + torch.log2(l)
    o = _r16((_r16(p0) @ v) / l)                                              # the forward's P to bf16 before P V; O to bf16 before delta
    delta = (do * o).sum(-1, keepdim=True)
    p = torch.exp2(s2 - lse2)                                                 # masked scores: exp2(-inf) = 0
    ds = p * (do @ v.transpose(-1, -2) - delta) * scale
    pb, dsb = _r16(p), _r16(ds)                                               # P and dS to bf16 before the second pair of products
    emu = (_r16(dsb @ k), _r16(dsb.transpose(-1, -2) @ q), _r16(pb.transpose(-1, -2) @ do))
    return exact, emu


def _row_err(x, ref, floor):
    """worst own row: |x - ref|_2 over max(|ref|_2, floor)"""
    return float(((x - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(floor)).max())


def _attn_rows(dev, lay, Hh, d, tq, tk, kw, label, seed=11, qamp=1.0):
    """one Part 2 case: run, reference, emulation, per-row bound: the kernel's worst row within 2x the emulation's.
    dq, dk, dv: the absolute floor is the tensor's rms row norm: a row below it is judged against it, as in |err| <= rtol (|ref| + rms).
    Such rows are where P (dP - delta) cancels, their error is delta's (one number per query, the rounding of O), and the worst of a few
    such numbers is no stable yardstick: relative to the row's own norm two correct realisations of the same roundings differ by
    more than 2x.  dv own: dV = P^T dO has no such cancellation, so dV is ALSO checked against each row's own norm, with a floor of
    2^-6 of the rms: a key seen by one query of two hundred (the tail of a causal diagonal) has to be right to its own scale.
    One key (P = 1): dQ = dK = 0 exactly, in the reference and in the emulation; the kernel leaves dS = (dP - delta) scale with dP and
    delta two fp32 dot products of head_dim terms summed in different orders, each within head_dim 2^-24 sum |dO_e V_e| of the same
    number.  That bound, through dQ_i = dS_i K and dK = sum_i dS_i Q_i, is the allowance there (absolute; 1 % for the two bf16 roundings)"""
    (q, k, v, do), grads = _attn_run(dev, lay, Hh, d, tq, tk, kw, seed, qamp)
    Sq, Sk = kw["Sq"], kw["Sk"]
    scale = d ** -0.5
    q4, k4, v4, do4 = lay.to4(q, Sq), lay.to4(k, Sk), lay.to4(v, Sk), lay.to4(do, Sq)
    exact, emu = _attn_f64(q4, k4, v4, do4, d, scale, kw["causal"], kw.get("causal_offset", 0))
    fails = []
    for n, got, ex, em, S in zip(("dq", "dk", "dv"), grads, exact, emu, (Sq, Sk, Sk)):
        got4 = lay.to4(got.to(f64), S)
        if not bool(ex.any()):
            assert Sk == 1 and n != "dv" and not bool(em.any())
            noise = 2 * d * U32 * (do4.abs() * v4.abs()).sum(-1)                               # [B', heads, Sq]
            allow = 1.01 * scale * (noise * k4.norm(dim=-1) if n == "dq" else (noise * q4.norm(dim=-1)).sum(-1, keepdim=True))
            ratio = float((got4.norm(dim=-1) / allow).max())
            print(f"train_matrix part2 | {label} d{d} | {n} | reference 0: worst |row| / fp32 allowance {ratio:.3e}")
            if ratio > 1:
                fails.append(f"{n}: a row of {ratio:.3g} x the fp32 noise allowance where the gradient is exactly zero")
            continue
        rms = float(ex.norm(dim=-1).pow(2).mean().sqrt())
        checks = [(n, rms)] + ([("dv own", 2.0 ** -6 * rms)] if n == "dv" else [])
        for name, floor in checks:
            e_emu, e_got = _row_err(em, ex, floor), _row_err(got4, ex, floor)
            print(f"train_matrix part2 | {label} d{d} | {name} | emulation {e_emu:.3e} | kernel {e_got:.3e}")
            if not e_got <= 2 * e_emu:
                fails.append(f"{name}: worst row {e_got:.4g} > 2 x emulation = {2 * e_emu:.4g}")
    assert not fails, f"{label} d{d}: " + "; ".join(fails)
    return grads


@pytest.mark.parametrize("Sq", [1, 31, 33, 100, 129])
@pytest.mark.parametrize("Sk", [1, 63, 65, 77, 130])
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_attn_bwd_rows_ragged(device, d, Sq, Sk):
    """ragged own and streamed edges, not causal: one row, one short of / one past the 32-row wave, the 64-row tile and the 128-row block"""
    B, Hh = 2, 2
    _attn_rows(device, _Plain(B, Hh, d), Hh, d, B * Sq, B * Sk, dict(batch=B, heads=Hh, head_dim=d, Sq=Sq, Sk=Sk, causal=False), f"ragged {Sq}x{Sk}")


@pytest.mark.parametrize("S", [1, 65, 129, 200])
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_attn_bwd_rows_causal_square(device, d, S):
    B, Hh = 2, 2
    _attn_rows(device, _Plain(B, Hh, d), Hh, d, B * S, B * S, dict(batch=B, heads=Hh, head_dim=d, Sq=S, Sk=S, causal=True), f"causal {S}")


@pytest.mark.parametrize("Sq,Sk,off", [(64, 192, 128), (100, 130, 30), (1, 77, 76), (64, 192, 100)])
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_attn_bwd_rows_causal_offset(device, d, Sq, Sk, off):
    """causal with Sq < Sk: query i sees the keys up to i + causal_offset (forward and backward run with the same offset).  The first
    three cases end at the last key (causal_offset = Sk - Sq); in the last one the keys from Sq + causal_offset on are visible to nobody
    and must get exactly zero dK and dV"""
    B, Hh = 2, 2
    kw = dict(batch=B, heads=Hh, head_dim=d, Sq=Sq, Sk=Sk, causal=True, causal_offset=off)
    lay = _Plain(B, Hh, d)
    _, dk, dv = _attn_rows(device, lay, Hh, d, B * Sq, B * Sk, kw, f"causal offset {Sq}x{Sk}+{off}")
    unseen = slice(Sq + off, Sk)
    for n, t in (("dK", dk), ("dV", dv)):
        assert bool((lay.to4(t, Sk)[:, :, unseen] == 0).all()), f"{n} of a key beyond the last visible position is not zero"


def test_attn_bwd_causal_offset_past_the_keys_is_refused(device):
    """Sq + causal_offset > Sk: SEER_EINVAL before any launch, nothing written"""
    from seervideoldm_amd import train_ops
    from seervideoldm_amd._lib import SeerHipError
    B, Hh, d, Sq, Sk = 1, 2, 40, 64, 192
    C = Hh * d
    q, do, out = [torch.zeros((B * Sq, C), device=device, dtype=bf16) for _ in range(3)]
    k, v = [torch.zeros((B * Sk, C), device=device, dtype=bf16) for _ in range(2)]
    lse = train_ops.attn_lse_buffer(B, Hh, Sq, device)
    dq, dk, dv = [torch.full_like(t, float("nan")) for t in (q, k, v)]
    with pytest.raises(SeerHipError, match=EINVAL):
        train_ops.attention_bwd(q, k, v, out, lse, do, dq, dk, dv, batch=B, heads=Hh, head_dim=d, Sq=Sq, Sk=Sk, causal=True, causal_offset=Sk - Sq + 1)
    assert all(bool(t.isnan().all()) for t in (dq, dk, dv))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", HEAD_DIMS)
def test_attn_bwd_rows_sharp_softmax(device, d, causal):
    """q scaled so that the scores have amplitude 6 in log2 units (as test_attention_sharp_softmax does for the forward): P spans many
    binades, a few keys carry a row"""
    B, Hh, Sq, Sk = 2, 2, 100, 130
    kw = dict(batch=B, heads=Hh, head_dim=d, Sq=Sq, Sk=Sk, causal=causal, causal_offset=Sk - Sq if causal else 0)
    _attn_rows(device, _Plain(B, Hh, d), Hh, d, B * Sq, B * Sk, kw, f"sharp causal={causal}", qamp=6.0 / LOG2E)


@pytest.mark.parametrize("d", HEAD_DIMS)
def test_attn_bwd_rows_window(device, d):
    """the temporal window form, ws 4, F 3, 8 x 8 (four windows of 48 tokens), causal"""
    B, Hh, Fr, H, W, ws = 1, 2, 3, 8, 8, 4
    T = B * Fr * H * W
    kw = dict(batch=B, heads=Hh, head_dim=d, Sq=Fr * ws * ws, Sk=Fr * ws * ws, causal=True, window=(ws, Fr, H, W))
    _attn_rows(device, _Window(B, Fr, H, W, ws, Hh, d), Hh, d, T, T, kw, "window ws4 F3 8x8")


@pytest.mark.parametrize("d", HEAD_DIMS)
def test_attn_bwd_rows_strided_sequences(device, d):
    """the FSText layout, F 5, L 9: rows ordered (frame, token), nine sequences of five read through strides, causal"""
    Fr, L, Hh = 5, 9, 2
    kw = dict(batch=L, heads=Hh, head_dim=d, Sq=Fr, Sk=Fr, causal=True, seq_stride_rows=L, batch_stride_rows=1)
    _attn_rows(device, _Strided(Fr, L, Hh, d), Hh, d, Fr * L, Fr * L, kw, "strided F5 L9")


# =========================================================================================== 3. the remaining train.hip kernels
def _gn_case(dev, B, rows, C1, C2, G, silu, seed=0):
    C = C1 + C2
    x1 = _rand((B * rows, C1), dev, seed + 1, 1.5).to(bf16)
    x2 = _rand((B * rows, C2), dev, seed + 2, 0.7).to(bf16) if C2 else None
    dy = _rand((B * rows, C), dev, seed + 3).to(bf16)
    gamma, beta = 1 + 0.2 * _rand((C,), dev, seed + 4), 0.1 * _rand((C,), dev, seed + 5)
    x64 = (torch.cat([x1, x2], 1) if C2 else x1).to(f64)
    xg = x64.reshape(B, rows, G, C // G)
    stats = torch.stack([xg.sum((1, 3)), xg.pow(2).sum((1, 3))], -1).to(f32).contiguous()        # what the forward pair hands over
    return x1, x2, dy, gamma, beta, x64, stats


def _gn_f64(x64, dy, gamma, beta, B, rows, G, silu, eps=1e-5):
    """float64 autograd of GroupNorm (+ SiLU) on [B, C, rows], and the fp32 part of the bound for dx, dgamma, dbeta"""
    C = x64.shape[1]
    xr = x64.reshape(B, rows, C).permute(0, 2, 1).contiguous().requires_grad_(True)
    gr, br = gamma.to(f64).requires_grad_(True), beta.to(f64).requires_grad_(True)
    y = Fn.group_norm(xr, G, gr, br, eps)
    if silu:
        y = Fn.silu(y)
    y.backward(dy.to(f64).reshape(B, rows, C).permute(0, 2, 1))
    dx = xr.grad.permute(0, 2, 1).reshape(B * rows, C)
    # first-order propagation of the kernel's fp32 roundings (absolute bounds; e = GN_DEPTH 2^-24 for the sums)
    e, cpg = GN_DEPTH * U32, C // G
    xg = x64.reshape(B, rows, G, cpg)
    mean, var = xg.mean((1, 3), keepdim=True), xg.var((1, 3), unbiased=False, keepdim=True)
    rstd = (var + eps).rsqrt()
    xh = (xg - mean) * rstd
    gam, bet, dyg = gamma.to(f64).reshape(1, 1, G, cpg), beta.to(f64).reshape(1, 1, G, cpg), dy.to(f64).reshape(B, rows, G, cpg)
    # mean = sum / count (3 roundings); var = sumsq / count - mean^2 cancels: 4 roundings relative to E x^2 + mean^2; rsqrt 2
    r = 4 * U32 * (xg.pow(2).mean((1, 3), keepdim=True) + mean * mean) / (2 * (var + eps)) + 2 * U32
    # xhat = fma(x, rstd, -mean rstd): the shift's rounding and the fma's are relative to |x| + |mean|, rstd's to |xhat|
    dxh = rstd * U32 * (5 * mean.abs() + 2 * xg.abs()) + r * xh.abs()
    z = xh * gam + bet
    sg = torch.sigmoid(z)
    gy = dyg * (sg * (1 + z * (1 - sg)) if silu else 1.0)
    # silu'(z): fma, __expf (2 ulp and its argument's rounding: |z| 2^-24), add, rcp, three more operations; |silu''| <= 1/2
    dgy = (8 * U32 * (1 + z.abs()) * gy.abs() + 0.5 * dyg.abs() * (gam.abs() * dxh + 2 * U32 * z.abs())) if silu else torch.zeros_like(gy)
    gg, dgg = (gy * gam).abs(), dgy * gam.abs()
    gm = lambda t: t.mean((1, 3), keepdim=True)
    p1, p2 = gm(gy * gam).abs(), gm(gy * gam * xh).abs()
    dp1 = e * gm(gg) + gm(dgg)
    dp2 = e * gm(gg * xh.abs()) + gm(dgg * xh.abs() + gg * dxh)
    own = gg + p1 + xh.abs() * p2
    fp_dx = (rstd * ((e + r) * own + dgg + dp1 + dxh * p2 + (xh.abs() + dxh) * dp2)).reshape(B * rows, C)
    flat = lambda t: t.reshape(B * rows, C)
    fp_dg = flat(dgy * xh.abs() + gy.abs() * dxh).sum(0) + e * flat(gy * xh).abs().sum(0)
    fp_db = flat(dgy).sum(0) + e * flat(gy).abs().sum(0)
    return dx, gr.grad, br.grad, fp_dx, fp_dg, fp_db


# additions on the longest path of the GroupNorm backward sums at these sizes (one row lane, one chunk per batch element): 7 rows of a
# chunk + 4 tree levels over the chunk lanes + 2 channel halves + 6 wave levels + 3 batch items = 22; the product with gamma, 1 / count,
# and the two subtractions, the product and the fma of the output: 30
GN_DEPTH = 32


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("rows", [1, 7])
@pytest.mark.parametrize("C1,C2", [(640, 640), (1280, 640), (2560, 1280), (4096, 0)])
def test_groupnorm_bwd_elementwise(device, C1, C2, rows, silu):
    """32 groups of 40 (640 + 640), 60 (1280 + 640) and 120 channels (2560 + 1280) -- in the last two group 21 straddles the two sources -- and
    the widest accepted group (128); batch 3, one row and seven per batch element; dres1 AND dres2; every dx, dgamma, dbeta element"""
    from seervideoldm_amd import train_ops
    B, G = 3, 32
    C = C1 + C2
    x1, x2, dy, gamma, beta, x64, stats = _gn_case(device, B, rows, C1, C2, G, silu)
    dres1 = _rand((B * rows, C1), device, 6).to(bf16)
    dres2 = _rand((B * rows, C2), device, 7).to(bf16) if C2 else None
    dg, db = [torch.full((C,), float("nan"), device=device) for _ in range(2)]
    dx1, dx2 = train_ops.groupnorm_bwd(x1, x2, B, G, stats, rows * (C // G), 1e-5, gamma, beta, silu, dy, dres1=dres1, dres2=dres2, dgamma=dg, dbeta=db)
    dx, dg_ref, db_ref, fp_dx, fp_dg, fp_db = _gn_f64(x64, dy, gamma, beta, B, rows, G, silu)
    dres = torch.cat([dres1, dres2], 1).to(f64) if C2 else dres1.to(f64)
    ref = dx + dres
    allow = U16 * ref.abs() + (1 + U16) * (fp_dx + U32 * (dx.abs() + dres.abs()))
    what = f"gn bwd {C1}+{C2} rows {rows} silu {silu}"
    _bound(dx1, ref[:, :C1], allow[:, :C1], what + " dx1")
    if C2:
        _bound(dx2, ref[:, C1:], allow[:, C1:], what + " dx2")
    print("train_matrix part3 | " + what + " | dgamma, dbeta: worst error / allowance",
          _bound(dg, dg_ref, fp_dg + 1e-30, what + " dgamma"), _bound(db, db_ref, fp_db + 1e-30, what + " dbeta"))


def test_groupnorm_bwd_dres2_alone(device):
    """dres1 = None, dres2 set (the skip-concat gradient arriving at the second source only).  With dy = 0 the norm's own gradient is
    exactly zero: dx2 IS dres2 and dx1 is zero, bit for bit.  With a random dy, dx2 differs from the run without dres2 by dres2 up to
    the two roundings involved, and dx1 is the same bits"""
    from seervideoldm_amd import train_ops
    B, G, rows, C1, C2 = 3, 32, 7, 1280, 640
    x1, x2, dy, gamma, beta, x64, stats = _gn_case(device, B, rows, C1, C2, G, True)
    dres2 = _rand((B * rows, C2), device, 7).to(bf16)
    args = (x1, x2, B, G, stats, rows * ((C1 + C2) // G), 1e-5, gamma, beta, True)
    z1, z2 = train_ops.groupnorm_bwd(*args, torch.zeros_like(dy), dres2=dres2)
    assert bool((z1 == 0).all()), "dx1 with dy = 0 and no dres1"
    assert torch.equal(z2, dres2), "dx2 with dy = 0 is not dres2"
    a1, a2 = train_ops.groupnorm_bwd(*args, dy)
    b1, b2 = train_ops.groupnorm_bwd(*args, dy, dres2=dres2)
    assert torch.equal(a1, b1)
    # a2 = o (1 + e1), b2 = (o + dres2)(1 + e2), |e| <= 2^-8: |b2 - a2 - dres2| <= 2^-8 (|a2| / (1 - 2^-8) + |b2| / (1 - 2^-8))
    slack = U16 / (1 - U16) * (a2.to(f64).abs() + b2.to(f64).abs())
    _bound(b2, a2.to(f64) + dres2.to(f64), slack + 1e-30, "dx2 with dres2 against dx2 without + dres2")
    assert not torch.equal(a2, b2)


def test_groupnorm_bwd_group_width_limit(device):
    """136 channels per group: SEER_ENOSYS, decided before any launch (128 is accepted: test_groupnorm_bwd_elementwise)"""
    from seervideoldm_amd import train_ops
    from seervideoldm_amd._lib import SeerHipError
    B, G, rows, C1 = 1, 32, 2, 32 * 136
    x1, _, dy, gamma, beta, _, stats = _gn_case(device, B, rows, C1, 0, G, False)
    with pytest.raises(SeerHipError, match=ENOSYS):
        train_ops.groupnorm_bwd(x1, None, B, G, stats, rows * 136, 1e-5, gamma, beta, False, dy)


# additions on the longest path of a LayerNorm backward row sum: 24 elements of a lane (C = 1536) + 6 wave levels = 30; 1 / C, and the two
# subtractions and two products of the output: 36.  d gamma / d beta add at most 3 rows per wave + 4 waves + 2 slabs: fewer
LN_DEPTH = 40


def _ln_f64(x64, dy64, gamma, eps=1e-5):
    """float64 autograd of LayerNorm, and the fp32 part of the bound for dx, dgamma, dbeta: first-order propagation of the kernel's
    roundings.  xhat = (x - mean) rstd cancels, so its error is NOT relative to |xhat|: the mean's is e mean |x|, the subtraction's
    2^-24 |x - mean|, both times rstd.  On a constant row (variance 0, rstd = eps^-1/2 = 316) that leaves |delta xhat| ~ 1e-3 and
    a bound on dx that is the row's one bf16 rounding plus ~1e-3: the row has to MATCH rstd (g - mean g) + dres"""
    C = x64.shape[1]
    xr = x64.clone().requires_grad_(True)
    gr, br = gamma.to(f64).requires_grad_(True), torch.zeros(C, device=x64.device, dtype=f64, requires_grad=True)
    Fn.layer_norm(xr, (C,), gr, br, eps).backward(dy64)
    e = LN_DEPTH * U32
    rm = lambda t: t.mean(1, keepdim=True)
    xm = x64 - rm(x64)
    rstd = (rm(xm * xm) + eps).rsqrt()
    xh = xm * rstd
    # the variance is a sum of non-negative terms (relative e) of (x - mean)^2 with the mean's error in it; rsqrt 2 ulp
    dmean = e * rm(x64.abs())
    r = 0.5 * (e * rm(xm * xm) + 2 * rm(xm.abs()) * dmean) / (rm(xm * xm) + eps) + 2 * U32
    dxh = rstd * (dmean + U32 * xm.abs()) + (r + U32) * xh.abs()
    g = (dy64 * gamma.to(f64)).abs()
    c2 = rm(dy64 * gamma.to(f64) * xh).abs()
    dc1 = e * rm(g)
    dc2 = e * rm(g * xh.abs()) + rm(g * dxh)
    fp_dx = rstd * ((e + r) * (g + rm(g) + xh.abs() * c2) + dc1 + dxh * c2 + (xh.abs() + dxh) * dc2)
    fp_dg = (dy64.abs() * dxh).sum(0) + e * (dy64 * xh).abs().sum(0)
    return xr.grad, gr.grad, br.grad, fp_dx, fp_dg, e * dy64.abs().sum(0)


@pytest.mark.parametrize("with_w", [False, True])
@pytest.mark.parametrize("rows,C", [(1, 8), (9, 8), (1, 1536), (9, 1536), (21, 520), (5, 1032)])
def test_layernorm_bwd_strided(device, rows, C, with_w):
    """x, dy, dres and dx are row-strided column slices of NaN buffers (the trainer's both[:, :C]); C = 8 and the widest C; one row; with
    more rows the last one is CONSTANT (variance 0: eps alone keeps rstd finite).  Every dx, dgamma, dbeta element; the gaps keep their NaN"""
    from seervideoldm_amd import train_ops
    x = _rand((rows, C), device, 1, 2.0).to(bf16)
    if rows > 1:
        x[-1] = 1.5
    dy, dres = _rand((rows, C), device, 2).to(bf16), _rand((rows, C), device, 5).to(bf16)
    gamma = 1 + 0.2 * _rand((C,), device, 3)
    bufs = [_gapped(t) for t in (x, dy, dres)]
    dxbuf, dx = _gapped(torch.zeros((rows, C), device=device, dtype=bf16))
    dg, db = ([torch.full((C,), float("nan"), device=device) for _ in range(2)]) if with_w else (None, None)
    train_ops.layernorm_bwd(bufs[0][1], bufs[1][1], gamma, dres=bufs[2][1], dx=dx, dgamma=dg, dbeta=db)
    for (buf, _), n in zip(bufs, ("x", "dy", "dres")):
        _gaps_hold(buf, rows, C, f"ln bwd {n}")
    _gaps_hold(dxbuf, rows, C, "ln bwd dx")
    own, dg_ref, db_ref, fp_dx, fp_dg, fp_db = _ln_f64(x.to(f64), dy.to(f64), gamma)
    ref = own + dres.to(f64)
    allow = U16 * ref.abs() + (1 + U16) * (fp_dx + U32 * (own.abs() + dres.to(f64).abs()))
    if rows > 1:        # the constant row: finite, and held to (almost) its one rounding, not to a bound of its own size
        assert bool(torch.isfinite(dx[-1].float()).all()), "the constant row"
        assert float((allow[-1] - U16 * ref[-1].abs()).max()) < 1e-2 and float(ref[-1].abs().max()) > 100
    _bound(dx, ref, allow, f"ln bwd {rows}x{C} dx")
    if with_w:
        print(f"train_matrix part3 | ln bwd {rows}x{C} | dgamma, dbeta: worst error / allowance",
              _bound(dg, dg_ref, fp_dg + 1e-30, f"ln bwd {rows}x{C} dgamma"), _bound(db, db_ref, fp_db + 1e-30, f"ln bwd {rows}x{C} dbeta"))


def test_layernorm_bwd_width_limit(device):
    """C = 1544 is one chunk past the three per lane: SEER_ENOSYS before any launch, dx untouched"""
    from seervideoldm_amd import train_ops
    from seervideoldm_amd._lib import SeerHipError
    x, dy = _rand((3, 1544), device, 1).to(bf16), _rand((3, 1544), device, 2).to(bf16)
    dx = torch.full_like(x, float("nan"))
    with pytest.raises(SeerHipError, match=ENOSYS):
        train_ops.layernorm_bwd(x, dy, torch.ones(1544, device=device), dx=dx)
    assert bool(dx.isnan().all())


@pytest.mark.parametrize("rows,inner", [(1, 16), (5, 16), (3, 48), (40, 1280)])
def test_geglu_strided(device, rows, inner):
    """pre, dout, out and dpre as row-strided slices of NaN buffers (the trainer's both[:, C:]); inner = 16; one row; gates cover
    [-8, 8] where erf saturates.  Forward: the documented accuracy of gelu_erf_f (3.1e-7 absolute on [-9, 9]) + one rounding; backward:
    erff / __expf to a few fp32 ulp of the cdf + one rounding.  No NaN, and at gate <= -6 the gate gradient is ~0 within that bound"""
    from seervideoldm_amd import _lib
    from seervideoldm_amd.ops import _p, _stream
    from seervideoldm_amd.weights import geglu_row_order
    order = geglu_row_order(inner).to(device)
    pre_ref = _rand((rows, 2 * inner), device, 1, 1.5)
    g = torch.Generator().manual_seed(9)
    pre_ref[:, inner:] = (torch.rand((rows, inner), generator=g) * 16 - 8).to(device)
    pre_ref[0, inner:inner + 8] = torch.tensor([-8.0, -7.0, -6.0, -5.5, 5.5, 6.0, 7.0, 8.0], device=device)
    pre_ref = pre_ref.to(bf16)
    dout = _rand((rows, inner), device, 2).to(bf16)
    (pbuf, pre), (dbuf, do) = _gapped(pre_ref[:, order].contiguous()), _gapped(dout)
    obuf, out = _gapped(torch.zeros((rows, inner), device=device, dtype=bf16))
    gbuf, dpre = _gapped(torch.zeros((rows, 2 * inner), device=device, dtype=bf16))
    lib = _lib.load()
    _lib.check(lib.seer_geglu_fwd(_p(pre), rows, inner, pre.stride(0), _p(out), out.stride(0), _stream()), "seer_geglu_fwd")
    _lib.check(lib.seer_geglu_bwd(_p(pre), _p(do), rows, inner, pre.stride(0), do.stride(0), _p(dpre), dpre.stride(0), _stream()), "seer_geglu_bwd")
    for buf, r, c, n in ((pbuf, rows, 2 * inner, "pre"), (dbuf, rows, inner, "dout"), (obuf, rows, inner, "out"), (gbuf, rows, 2 * inner, "dpre")):
        _gaps_hold(buf, r, c, f"geglu {n}")
    val, gate = pre_ref.to(f64).chunk(2, dim=-1)
    cdf = 0.5 * (1 + torch.erf(gate / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * gate * gate) / math.sqrt(2 * math.pi)
    d64 = dout.to(f64)
    ref = val * gate * cdf
    _bound(out, ref, U16 * ref.abs() + 4e-7 * val.abs() + 1e-30, f"geglu fwd {rows}x{inner}")
    dval, dgate = d64 * gate * cdf, d64 * val * (cdf + gate * pdf)
    ref_b = torch.cat([dval, dgate], 1)[:, order]
    # cdf = 0.5 (1 + erff(x / sqrt 2)): the argument's rounding moves erf by < 1/2 ulp of 1, erff itself is within 4, the add 1: 6 x 2^-24
    # ABSOLUTE (cdf <= 1); x pdf: x^2, the scale, __expf (2 ulp + 2^-24 of an argument of x^2 / 2) and two products: (6 + x^2 / 2) 2^-24 relative
    # of |x| pdf <= 0.25, at most 3 x 2^-24 absolute anywhere; their sum 1; the two products with d and x (or v) 2 more of a factor <= 1.13
    fp = torch.cat([10 * U32 * (d64 * gate).abs(), 14 * U32 * (d64 * val).abs()], 1)[:, order]
    _bound(dpre, ref_b, U16 * ref_b.abs() + fp + 1e-30, f"geglu bwd {rows}x{inner}")
    sat = gate <= -6
    got_dgate = dpre.to(f64)[:, torch.argsort(order)][:, inner:]
    assert bool(sat.any()) and float(got_dgate[sat].abs().max()) < 1e-4, "the gate gradient where erf has saturated"


@pytest.mark.parametrize("B,Fr,H,W,C0", [(2, 3, 3, 5, 320), (2, 1, 1, 4, 16), (2, 3, 5, 3, 40), (2, 1, 4, 1, 8)])
def test_conv_out_bwd_elementwise(device, B, Fr, H, W, C0):
    """H != W both ways round, H = 1, W = 1, F = 1 and 3: every element, so every image border.  36 products per element in fp32 + one
    rounding"""
    from seervideoldm_amd import train_ops
    Cc = 4
    dpred = _rand((B, Cc, Fr, H, W), device, 1)
    w = _rand((Cc, C0, 3, 3), device, 3, 0.05)
    got = train_ops.conv_out_bwd(dpred, w.permute(0, 2, 3, 1).contiguous())

    def dx_of(dp, ww):
        x = torch.zeros((B * Fr, C0, H, W), device=device, dtype=f64, requires_grad=True)
        Fn.conv2d(x, ww, padding=1).backward(dp.permute(0, 2, 1, 3, 4).reshape(B * Fr, Cc, H, W))
        return x.grad.permute(0, 2, 3, 1).reshape(B * Fr * H * W, C0)
    ref, mag = dx_of(dpred.to(f64), w.to(f64)), dx_of(dpred.to(f64).abs(), w.to(f64).abs())
    _bound(got, ref, U16 * ref.abs() + 40 * U32 * mag + 1e-30, f"conv_out bwd {B}x{Fr}x{H}x{W}x{C0}")


def _two_stage_depth(total, blocks, per_block=256):
    """additions on the longest path of the block-partial sums: a thread's elements, the 8-level tree, the ordered sum of the blocks"""
    return -(-total // (blocks * per_block)) + 8 + blocks


@pytest.mark.parametrize("B,Cc,Ft,cond,H,W", [(2, 4, 5, 0, 3, 5), (2, 4, 5, 4, 3, 5), (1, 4, 3, 0, 1, 1), (2, 4, 2, 1, 1, 1), (2, 4, 5, 2, 81, 101)])
def test_mse_loss_grad_elementwise(device, B, Cc, Ft, cond, H, W):
    """cond_f = 0 and F_total - 1, HW = 1 and odd; the last case makes every thread of the capped grid take two elements.  The loss is
    the mean over all B C (F_total - cond_f) HW elements; dpred is EXACTLY zero on the conditioning frames"""
    from seervideoldm_amd import train_ops
    pred = _rand((B, Cc, Ft, H, W), device, 1)
    target = _rand((B, Cc, Ft - cond, H, W), device, 2)
    loss, dpred = train_ops.mse_loss_grad(pred, target, cond)
    n = B * Cc * (Ft - cond) * H * W
    diff = pred.to(f64)[:, :, cond:] - target.to(f64)
    ref_loss = diff.pow(2).sum() / n
    total = B * Cc * Ft * H * W
    depth = _two_stage_depth(total, min(1024, -(-total // 256)))
    # every d^2 carries the rounding of d (twice) and of the square; the sum of non-negative terms adds `depth` more, 1/n two
    assert abs(loss.item() - ref_loss.item()) <= (depth + 6) * U32 * ref_loss.item(), (loss.item(), ref_loss.item(), depth)
    assert bool((dpred[:, :, :cond] == 0).all()), "dpred on the conditioning frames"
    ref_g = 2 * diff / n
    # d = pred - target is ONE rounding relative to |d| (both operands are fp32 values); 1/n, and the two products
    _bound(dpred[:, :, cond:], ref_g, 4 * U32 * ref_g.abs() + 1e-45, f"mse grad cond {cond} HW {H * W}")


@pytest.mark.parametrize("b,Fr,L,Cc", [(1, 1, 1, 8), (1, 1, 77, 192), (2, 3, 1, 8), (2, 5, 3, 72)])
def test_text_loss_grad_elementwise(device, b, Fr, L, Cc):
    """F = 1, b = 1, LC = 8: the gradient 2 (mean_f y - t) / (b L C F) is ADDED to a dy of its own magnitude, one rounding"""
    from seervideoldm_amd import train_ops
    y = _rand((b * Fr * L, Cc), device, 1).to(bf16)
    t = _rand((b, L, Cc), device, 2)
    n = b * L * Cc
    dy0 = (_rand((b * Fr * L, Cc), device, 3) * (2.0 / (n * Fr))).to(bf16)
    dy = dy0.clone()
    loss = train_ops.text_loss_grad(y, t, b, Fr, dy)
    y64 = y.to(f64).reshape(b, Fr, L, Cc)
    diff = y64.mean(1) - t.to(f64)
    ref_loss = diff.pow(2).sum() / n
    total8 = b * L * Cc // 8
    depth = 8 * -(-total8 // (min(1024, -(-total8 // 256)) * 256)) + 8 + min(1024, -(-total8 // 256))
    # d = mean_f y - t: the frame sum (F additions), 1/F and the difference leave |delta d| <= (F + 2) 2^-24 (mean_f |y| + |t|), which
    # moves d^2 by 2 |d| |delta d|; then the two-stage sum of non-negative terms
    dd = (Fr + 2) * U32 * (y64.abs().mean(1) + t.to(f64).abs())
    allow_loss = ((depth + 6) * U32 * diff.pow(2).sum() + (2 * diff.abs() * dd).sum()) / n
    assert abs(loss.item() - ref_loss.item()) <= allow_loss.item(), (loss.item(), ref_loss.item(), allow_loss.item())
    g = (2.0 / (n * Fr)) * diff
    ref = dy0.to(f64).reshape(b, Fr, L, Cc) + g[:, None]
    # delta d as above, the scale (its rounding and the product's), the add
    fp = (2.0 / (n * Fr)) * (dd + 2 * U32 * diff.abs())[:, None] + U32 * ref.abs()
    _bound(dy.reshape(b, Fr, L, Cc), ref, U16 * ref.abs() + fp + 1e-30, f"text loss grad b{b} F{Fr} L{L} C{Cc}")


@pytest.mark.parametrize("n", [1, 3, 4099, 1024 * 4096 + 5])
def test_sumsq_exact_and_bounded(device, n):
    """n = 1, 3, two blocks, and past the 1024-block cap (every thread takes 17 elements).  Integers in [-1, 1]: exact.  Random data:
    within the two-stage sum's derived bound (the terms are non-negative: the bound is relative)"""
    from seervideoldm_amd import train_ops
    g64 = _ints((n,), device, 1, -1, 1)
    _exact_pre(n, 1, 1)
    _eq(train_ops.sumsq(g64.to(f32)), g64.pow(2).sum().reshape(1), bf16, f"sumsq n {n}")
    g = _rand((n,), device, 2, 3.0)
    ref = g.to(f64).pow(2).sum().item()
    depth = _two_stage_depth(n, min(1024, max(1, -(-n // 4096))))
    got = train_ops.sumsq(g).item()
    assert abs(got - ref) <= (depth + 2) * U32 * ref, (got, ref, depth)


@pytest.mark.parametrize("n", [4, 100004, 4 * 1024 * 1024 + 8])
def test_axpby_alias_and_beta_zero(device, n):
    """y aliasing x; beta = 0 over NaN in y: the kernel documents that it does not read y then.  Powers of two on integers: exact"""
    from seervideoldm_amd import train_ops
    x64 = _ints((n,), device, 1, -1000, 1000)
    y = x64.to(f32)
    train_ops.axpby(y, y, 0.5, 0.25)                                         # y = 0.25 y + 0.5 y
    _eq(y, 0.75 * x64, bf16, "axpby, y aliasing x")
    x = x64.to(f32)
    y = torch.full((n,), float("nan"), device=device)
    train_ops.axpby(y, x, 0.5, 0.0)
    assert bool(torch.isfinite(y).all()), "beta = 0 read y"
    _eq(y, 0.5 * x64, bf16, "axpby, beta = 0 over NaN")
    y2 = _ints((n,), device, 2, -1000, 1000)
    y = y2.to(f32)
    train_ops.axpby(y, x, 2.0, -1.0)
    _eq(y, 2.0 * x64 - y2, bf16, "axpby, beta = -1")


def _f32v(x):
    """a hyper-parameter as the ABI receives it: rounded to fp32"""
    return torch.tensor(x, dtype=f32).item()


@pytest.mark.parametrize("n", [1, 1000])
@pytest.mark.parametrize("step", [1, 10000])
@pytest.mark.parametrize("mode", ["unclipped", "clipped", "no_sumsq"])
@pytest.mark.parametrize("wd,with_bf16", [(1e-2, True), (0.0, False)])
def test_adamw_against_float64(device, n, step, mode, wd, with_bf16):
    """torch.optim.AdamW stepped in float64 (hyper-parameters as the ABI receives them: fp32 values) against seer_adamw_step: p, m AND v
    element by element.  unclipped: grad_sumsq given and max_norm above the norm, the coefficient is exactly 1 (what most steps of
    a run are); clipped; grad_sumsq = None.  weight_decay 0 and p_bf16 = None (trainer.py passes no p_bf16); step 1 and step 10000 (the
    bias corrections), the latter on warm m and v; n = 1 and n off a multiple of 256"""
    from seervideoldm_amd import train_ops
    lr, b1, b2, eps, wdf = _f32v(1e-3), _f32v(0.9), _f32v(0.999), _f32v(1e-8), _f32v(wd)
    p0, g = _rand((n,), device, 1), _rand((n,), device, 2, 3.0)
    m0 = _rand((n,), device, 3, 0.5) if step > 1 else torch.zeros(n, device=device)
    v0 = _rand((n,), device, 4).pow(2) if step > 1 else torch.zeros(n, device=device)
    ss = g.to(f64).pow(2).sum().to(f32).reshape(1)
    norm = math.sqrt(ss.item())
    max_norm = {"unclipped": _f32v(2.0 * norm + 1.0), "clipped": _f32v(0.3 * norm), "no_sumsq": _f32v(0.3 * norm)}[mode]
    coef = 1.0 if mode == "no_sumsq" else min(1.0, max_norm / (norm + _f32v(1e-6)))
    assert (coef == 1.0) == (mode != "clipped")
    # reference
    rp = torch.nn.Parameter(p0.to(f64))
    opt = torch.optim.AdamW([rp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wdf)
    if step > 1:
        opt.state[rp] = dict(step=torch.tensor(float(step - 1)), exp_avg=m0.to(f64).clone(), exp_avg_sq=v0.to(f64).clone())
    gc = g.to(f64) * coef
    rp.grad = gc.clone()
    opt.step()
    rm, rv = opt.state[rp]["exp_avg"], opt.state[rp]["exp_avg_sq"]
    assert int(opt.state[rp]["step"]) == step
    # kernel
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    pb = torch.full((n,), float("nan"), device=device, dtype=bf16) if with_bf16 else None
    train_ops.adamw_step(p, g, m, v, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wdf, step=step, grad_sumsq=None if mode == "no_sumsq" else ss,
                         max_norm=max_norm, p_bf16=pb)
    what = f"adamw n{n} step{step} {mode} wd{wd}"
    # m' = b1 m + (1 - b1) g coef: the clip coefficient (3 roundings), two products, one sum
    allow_m = 6 * U32 * (b1 * m0.to(f64).abs() + (1 - b1) * gc.abs()) + 1e-38
    _bound(m, rm, allow_m, what + " m")
    # v' = b2 v + (1 - b2) (g coef)^2: all terms non-negative
    _bound(v, rv, 12 * U32 * rv + 1e-38, what + " v")
    # p' = p (1 - lr wd) - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps): the decay (3 roundings of p), the update u with the relative errors
    # of m' (allow_m / |m'|), of sqrt(v') (half of v's 12), and of the two rounded constants and the seven operations around them: 24
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = rv.sqrt() / math.sqrt(bc2) + eps
    u = (lr / bc1) * rm / denom
    allow_p = 4 * U32 * p0.to(f64).abs() + (lr / bc1) * allow_m / denom + 24 * U32 * u.abs() + 1e-38
    _bound(p, rp.detach(), allow_p, what + " p")
    if with_bf16:
        assert torch.equal(pb, p.to(bf16)), what + ": the bf16 working copy is not the rounded parameter"
