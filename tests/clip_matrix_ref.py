"""TEST INFRASTRUCTURE ONLY -- the two kernels of the CLIP text tower (csrc/clip_text.hip: seer_attn_causal64, seer_embed_tokens) restated
in float64 torch on the CPU, independently of the product (no import from seervideoldm_amd), for tests/test_gpu_clip_matrix.py (the
kernels) and tests/test_clip_matrix_ref_cpu.py (the constructions and the mutation table, without a GPU).  No tests here.

1. The cases: LENGTHS x MASKS, the (batch, heads) layout each one runs in (`layout`), the masks (`mask`: the six kinds of
   test_gpu_clip_text._mask restated for any batch, and three more that aim at the 16-key tile and the 32-key P V step).
2. The SELECTOR construction (`selector_qk`, `selector_want`): scores 256 (t^2 - (j - t)^2), integers below 2^24, so that P is one-hot on the
   visible key nearest to the target t (or 1/2, 1/2 on two of them) and O[i] is a row of V bit for bit.
3. The UNIFORM construction (`uniform_v`): Q = 0, every visible P = 2^0, O[i] = (sum of the visible V) / n_i with V built per sample from
   the RANK of a key among the visible ones, so that the quotient is exact for EVERY row of EVERY mask, holes included:
     RAMP     V = 2 a (rank - r0) + lift, O = a (n - 1 - 2 r0) + lift (a in +-1, +-1/2, +-1/4 by column; a masked key holds 32 |a| more);
     BALANCE  (+w, -w) on ranks (2k, 2k + 1) with w = (2k + 1) u_k: O = 0 after an even count and u_k after 2k + 1 (a masked key holds 64);
     LEVEL    V = c, |c| in [128, 255], O = c: one more key with V = 0 in the denominator gives c n / (n + 1), another bf16 value
              (a masked key holds 0, so that admitting it is that case too).
   The kinds are interleaved column by column, so every 8-column load and every 16-column tile of O holds all three.
4. `emulate`: the float64 softmax formula (the reference) and the emulation that rounds only where the kernel rounds -- inputs already
   bf16, P to bf16 for the P V product, the denominator from the unrounded P, O to bf16 -- laid out as the kernel works: per 16-query
   tile, over the staged keys 0 .. 32 nk32 - 1, keys at and past L being the clamped duplicate of row L - 1 (K) and zeros (V).  With the
   MUTATIONS of the mutation table applied to the emulation on request.
5. The embedding: tables of arbitrary finite bf16 bit patterns with planted rounding ties, and the reference sum.
"""
from __future__ import annotations

import torch

from tests.attn_fwd_ref import RAMP_A, rnd, row_floor  # noqa: F401  (row_floor: re-exported for the two test files)
from tests.test_gpu_f16_matrix import _ints, _rand, _store

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
HD, LMAX = 64, 128
PRESCALE = 64 ** -0.5 * 1.4426950408889634                  # what ops.qk_prescale(64) returns (asserted in the GPU file)
LENGTHS = (1, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 77, 96, 97, 127, 128)
MASKS = ("null", "ones", "len1", "len20", "holes", "zero", "last", "tile", "even", "comb")
LAYOUTS = ((1, 1), (2, 2), (3, 3))
ROW_LENGTHS = (1, 17, 33, 77, 128)
ROW_MASKS = ("null", "len20", "holes", "zero")
MUTATIONS = ("drop_last", "admit_masked", "admit_clamped", "diag+1", "diag-1", "pos_swap", "other_sample_v", "l_rounded", "skip_p_round")
NUMERIC_ONLY = ("l_rounded", "skip_p_round")


def layouts(L, kind):
    """(batch, heads) cycles through (1, 1), (2, 2), (3, 3) over lengths AND masks, so that every length and every mask meets all three;
    CLIP's own 77 also runs at (1, 12)"""
    out = [LAYOUTS[(LENGTHS.index(L) + MASKS.index(kind)) % 3]]
    return out + [(1, 12)] if L == 77 else out


def mask(kind, batch, L):
    """uint8 [batch, L], 0 = hidden, or None.  null .. zero: the kinds of tests/test_gpu_clip_text.py for any batch (zero: every odd sample
    sees nothing at all; sample 0 hides key 0, so its query 0 sees nothing either).  last: the only hidden key is the last one.  tile: one
    whole 16-key tile is hidden, another one per sample.  even: the even tile of a 32-key pair is hidden and its odd tile visible (a pair
    that has an odd tile, where there is one).  comb (not asked for by the issue): every other key is hidden, the odd ones in even samples: a
    hidden target between two visible keys is a TIE of the selector at every length, where holes has one such key, and none below 20"""
    if kind == "null":
        return None
    m = torch.ones((batch, L), dtype=torch.uint8)
    nt = (L + 15) // 16
    if kind == "len1":
        m[:, 1:] = 0
    elif kind == "len20":
        m[:, 20:] = 0
    elif kind == "holes":
        m[:, 5:9] = 0
        m[0, L // 2] = 0
    elif kind == "zero":
        m[1::2] = 0
        m[0, 0] = 0
    elif kind == "last":
        m[:, L - 1] = 0
    elif kind == "tile":
        for b in range(batch):
            t = (b + 1) % nt
            m[b, 16 * t:16 * t + 16] = 0
    elif kind == "even":
        for b in range(batch):
            p = b % max(1, nt // 2)
            m[b, 32 * p:32 * p + 16] = 0
    elif kind == "comb":
        for b in range(batch):
            m[b, (b + 1) % 2::2] = 0
    else:
        assert kind == "ones", kind
    return m


def to4(x2, batch, heads, L):
    """token-major [batch * L, heads * 64] -> [batch, heads, L, 64]"""
    return x2.reshape(batch, L, heads, HD).transpose(1, 2)


def to2(x4):
    b, h, L, _ = x4.shape
    return x4.transpose(1, 2).reshape(b * L, h * HD)


def key_visible(m, batch, L):
    """[batch, L] bool: the padding mask alone"""
    return torch.ones((batch, L), dtype=torch.bool) if m is None else (m != 0)


def visible(m, batch, L):
    """[batch, L (query), L (key)] bool: key <= query and not hidden"""
    return torch.tril(torch.ones(L, L, dtype=torch.bool))[None] & key_visible(m, batch, L)[:, None, :]


# ------------------------------------------------------------------------------------------- the selector construction
def selector_cols(h):
    """the three columns of head h that carry the score: in both 32-wide K steps of the S^T product, moving through the 8-column loads"""
    return (5 * h + 1) % HD, (5 * h + 34) % HD, (5 * h + 63) % HD


def targets(kind, batch, heads, L, seed=0):
    """int64 [batch, heads, L]: diag t = i (key <= q, not <); beyond t = i + 1 (the result must be the diagonal key instead); spread: any
    t <= i, another one per (sample, head)"""
    i = torch.arange(L)
    if kind == "diag":
        return i.expand(batch, heads, L).clone()
    if kind == "beyond":
        return (i + 1).expand(batch, heads, L).clone()
    assert kind == "spread"
    u = torch.rand((batch, heads, L), generator=torch.Generator().manual_seed(seed + 7 * L), dtype=f64)
    return (u * (i + 1).to(f64)).floor().long().clamp_max(i)


def selector_qk(t):
    """t int64 [batch, heads, L] -> (q4, k4) float64, exact in bf16.  K holds j, j^2 // 256, j^2 % 256 and Q holds 512 t, -65536, -256 in
    three columns, zeros elsewhere: q . k = 256 (2 t j - j^2), every product and every partial sum a multiple of 256 below 2^24"""
    batch, heads, L = t.shape
    assert L <= LMAX and int(t.max()) <= LMAX and int(t.min()) >= 0
    q4, k4 = torch.zeros((batch, heads, L, HD), dtype=f64), torch.zeros((batch, heads, L, HD), dtype=f64)
    j = torch.arange(L, dtype=f64)
    for h in range(heads):
        c0, c1, c2 = selector_cols(h)
        k4[:, h, :, c0], k4[:, h, :, c1], k4[:, h, :, c2] = j, (j * j / 256).floor(), (j * j) % 256
        q4[:, h, :, c0], q4[:, h, :, c1], q4[:, h, :, c2] = 512.0 * t[:, h].to(f64), -65536.0, -256.0
    _store(q4, bf16), _store(k4, bf16)
    assert 512 * LMAX * (LMAX - 1) + 65536 * ((LMAX - 1) ** 2 // 256) + 256 * 255 < 2 ** 24      # the sum of the three |products|
    return q4, k4


def selector_sel(t, vis):
    """[batch, heads, L, L] float64: 1 on the visible key(s) nearest to the target -- one, or t - d and t + d"""
    L = t.shape[-1]
    d = (torch.arange(L)[None, None, None, :] - t[..., None]).abs().to(f64).masked_fill(~vis[:, None], float("inf"))
    dmin = d.min(-1, keepdim=True).values
    return ((d == dmin) & vis[:, None]).to(f64)


def no_ties(t, vis):
    """the same targets with every two-key tie moved to the query's own diagonal target (which cannot tie: nothing beyond it is visible)"""
    tie = selector_sel(t, vis).sum(-1) > 1
    return torch.where(tie, torch.arange(t.shape[-1]).expand_as(t), t)


def selector_want(t, vis, v4):
    """the expected O in float64: V of the nearest visible key, the mean of two where they tie, zeros for a query that sees nothing"""
    sel = selector_sel(t, vis)
    n = sel.sum(-1, keepdim=True)
    want = (sel @ v4) / n.clamp_min(1.0)
    if bool((n > 1).any()):
        _store(want, bf16)                                                  # a mean of two must be exact
    return want


def arbitrary_v(batch, heads, L, seed=0):
    """[batch, heads, L, 64] float64 holding arbitrary finite bf16 bit patterns (zeros, subnormals and 3e38 among them; an all-ones exponent
    loses its lowest exponent bit).  Asserted: inside every 16-column tile of O the rows of two keys of one (sample, head) differ"""
    g = torch.Generator().manual_seed(1000 + seed + L)
    bits = torch.randint(0, 65536, (batch, heads, L, HD), generator=g, dtype=torch.int32)
    bits = torch.where((bits & 0x7F80) == 0x7F80, bits & ~0x0080, bits)
    v = (bits - ((bits & 0x8000) << 1)).to(torch.int16).view(bf16).to(f64)
    assert bool(torch.isfinite(v).all())
    for dt in range(4):
        tile = v[..., 16 * dt:16 * dt + 16]
        same = (tile[:, :, :, None, :] == tile[:, :, None, :, :]).all(-1).sum((-1, -2))
        assert bool((same == L).all()), "two keys hold the same V in a 16-column tile"
    return v


def dyadic_v(batch, heads, L, seed=0):
    """multiples of 1/4 up to 32: the mean of any two is exact in bf16"""
    return _store(_ints((batch, heads, L, HD), "cpu", 2000 + seed + L, -128, 128) / 4, bf16).to(f64)


def tie_targets(batch, heads, L, m, seed=1):
    """spread targets, and on every even query past it the last hidden key whose two neighbours are visible: t - 1 and t + 1 tie there"""
    t = targets("spread", batch, heads, L, seed)
    kv = key_visible(m, batch, L)
    for b in range(batch):
        lone = [h for h in range(1, L - 1) if not kv[b, h] and kv[b, h - 1] and kv[b, h + 1]]
        for i in range(0, L, 2):
            at = [h for h in lone if h + 1 <= i]
            if at:
                t[b, :, i] = at[-1]
    return t


# ------------------------------------------------------------------------------------------- the uniform construction
BAL_U =(1.0, -1.0, 0.5, -0.5, 2.0, -2.0)


def uniform_v(batch, heads, L, m, seed=0):
    """-> (v4, want4, n) float64 [batch, heads, L, 64] twice and the visible count per query [batch, L]; see the module docstring.  Every V
    and every expected O is asserted exact in bf16; partial sums are multiples of 1/4 below 2^17"""
    kv = key_visible(m, batch, L)
    n = (kv[:, None, :] & torch.tril(torch.ones(L, L, dtype=torch.bool))[None]).sum(-1)           # [batch, L]
    rank = (kv.long().cumsum(1) - kv.long()).to(f64)[:, None, :, None]                            # visible keys before this one
    n4 = n.to(f64)[:, None, :, None]
    nmax = kv.sum(1).to(f64)[:, None, None, None]
    e = torch.arange(HD)
    kind = e % 4                                                                                  # 0, 2 RAMP . 1 BALANCE . 3 LEVEL
    a = torch.tensor(RAMP_A, dtype=f64)[(e // 2) % 6]
    hidden = (~kv)[:, None, :, None]
    sign = 1.0 - 2.0 * ((torch.arange(batch)[:, None] + torch.arange(heads)[None, :]) % 2).to(f64)[:, :, None, None]
    # RAMP
    r0 = (nmax / 2).floor()
    lift = torch.where(nmax <= 64, 128.0 * a.abs(), torch.zeros_like(a))
    v_ramp = 2 * a * (rank - r0) + lift + 32.0 * a.abs() * hidden
    w_ramp = a * (n4 - 1 - 2 * r0) + lift
    # BALANCE
    u_of = lambda k: torch.tensor(BAL_U, dtype=f64)[(k.long() + (e // 4)) % 6]
    k_key = (rank / 2).floor()
    v_bal = (2 * k_key + 1) * u_of(k_key) * (1.0 - 2.0 * (rank % 2))
    v_bal = torch.where(hidden, torch.full_like(v_bal, 64.0), v_bal)
    w_bal = torch.where(n4 % 2 == 1, u_of(((n4 - 1) / 2).floor().clamp_min(0)), torch.zeros((), dtype=f64))
    # LEVEL
    c = _ints((batch, heads, 1, HD), "cpu", 3000 + seed + L, 128, 255)
    v_lev = torch.where(hidden, torch.zeros((), dtype=f64), c.expand(batch, heads, L, HD))
    pick = lambda r, b, l: torch.where(kind == 3, l, torch.where(kind == 1, b, r))
    v = (sign * pick(v_ramp, v_bal, v_lev)).expand(batch, heads, L, HD).contiguous()
    want = (sign * pick(w_ramp, w_bal, c)).expand(batch, heads, L, HD) * (n4 > 0)
    want = want.contiguous()
    _store(v, bf16), _store(want, bf16)
    moved = rnd(c * LMAX / (LMAX + 1), bf16) != c
    assert bool(moved.all()), "a level column would not see one more key in the denominator"
    return v, want, n


def exact_runs(L, kind, batch, heads):
    """the Part 1 runs of one case: (name, q4, k4, v4, want4, m), float64 [batch, heads, L, 64] holding bf16 values.  Three selector runs on
    arbitrary bit patterns (diag, beyond, spread with its ties moved to the diagonal), one on dyadic V with ties, the uniform one"""
    m = mask(kind, batch, L)
    vis = visible(m, batch, L)
    va, vd = arbitrary_v(batch, heads, L), dyadic_v(batch, heads, L)
    for tk in ("diag", "beyond", "spread"):
        t = no_ties(targets(tk, batch, heads, L), vis)
        q4, k4 = selector_qk(t)
        yield f"selector {tk}", q4, k4, va, selector_want(t, vis, va), m
    t = tie_targets(batch, heads, L, m)
    q4, k4 = selector_qk(t)
    yield "selector ties", q4, k4, vd, selector_want(t, vis, vd), m
    v4, want4, _ = uniform_v(batch, heads, L, m)
    yield "uniform", torch.zeros((batch, heads, L, HD), dtype=f64), _ints((batch, heads, L, HD), "cpu", 3), v4, want4, m


# ------------------------------------------------------------------------------------------- reference and emulation
class Emu:
    """o_ref: the float64 formula; o: the emulation, rounded to bf16; n: visible keys per query [batch, L]"""


def _default_swap(L):
    """two keys of one 32-key block of the V order: the first key of the last block and the last key; where the last block holds one key
    alone, the two ends of the block before it"""
    a = (L - 1) // 32 * 32
    return (a, L - 1) if L - 1 > a else (a - 32, a - 1)


def emulate(q4, k4, v4, m, *, mut=None, swap=None):
    """q4, k4, v4: [batch, heads, L, 64] float64 holding bf16 values; m: uint8 [batch, L] or None.  `mut`: one of MUTATIONS, applied to the
    EMULATION only (the reference stays the operation asked for); returns None where the mutation does not apply:
      drop_last        the last key the padding mask leaves visible is dropped, per sample (a mask that hides everything has none)
      admit_masked     the first key the mask hides is seen by every query at or past it (no mask, or nothing hidden: not applicable)
      admit_clamped    the key at position L -- the clamped duplicate of row L - 1, V = 0 -- is seen by the queries of the last tile
                       (L a whole number of 16-key tiles: there is no such key; no query of that tile sees a key: zeros stay zeros)
      diag+1, diag-1   key <= q + 1 inside the query's own key tiles / key <= q - 1 (one key: +1 changes nothing)
      pos_swap         the V rows of two keys of one 32-key block change places in the staged order, P stays (`swap`, or _default_swap)
      other_sample_v   staged keys at and past L hold the rows that follow in the buffer -- the next sample's, then the NaN guard row and
                       what lies behind it -- not zeros; their P is 0 (L a whole number of 32-key steps: nothing is staged past L)
      l_rounded        the denominator is the sum of the ROUNDED P
      skip_p_round     P enters the P V product unrounded"""
    assert mut is None or mut in MUTATIONS, mut
    B, H, L, _ = q4.shape
    nt = (L + 15) // 16
    key = torch.arange(LMAX)
    i, j = torch.arange(L)[:, None], key[None, :]
    kx = k4[:, :, key.clamp_max(L - 1)]
    vx = torch.cat([v4, torch.zeros((B, H, LMAX - L, HD), dtype=f64)], 2)
    kv = torch.ones((B, LMAX), dtype=torch.bool)
    kv[:, :L] = key_visible(m, B, L)
    own_tiles = j < 16 * (i // 16 + 1)                                  # key tiles 0 .. t: all a query tile computes
    vis_ref = ((j <= i) & (j < L))[None] & kv[:, None, :]               # [B, L, 128]
    adm = vis_ref.clone()
    if mut == "drop_last":
        any_vis = kv[:, :L].any(1)
        if not bool(any_vis.any()):
            return None
        last = L - 1 - kv[:, :L].flip(1).long().argmax(1)
        for b in range(B):
            if bool(any_vis[b]):
                adm[b, :, last[b]] = False
    elif mut == "admit_masked":
        hid = ~kv[:, :L]
        if not bool(hid.any()):
            return None
        for b in range(B):
            if bool(hid[b].any()):
                jm = int(hid[b].long().argmax())
                adm[b, jm:, jm] = True
    elif mut == "admit_clamped":
        if L % 16 == 0 or not bool(vis_ref[:, 16 * (nt - 1):].any()):
            return None
        adm[:, 16 * (nt - 1):, L] = True
    elif mut in ("diag+1", "diag-1"):
        adm = ((j <= i + (1 if mut == "diag+1" else -1)) & (j < L) & own_tiles)[None] & kv[:, None, :]
        if torch.equal(adm, vis_ref):
            return None
    elif mut == "pos_swap":
        if L < 2:
            return None
        a, b = swap if swap is not None else _default_swap(L)
        assert a // 32 == b // 32 and a != b and max(a, b) < L
        perm = torch.arange(LMAX)
        perm[a], perm[b] = b, a
        vx = vx[:, :, perm]
    elif mut == "other_sample_v":
        if L % 32 == 0:
            return None
        arena = torch.cat([to2(v4), torch.full((LMAX + 1, H * HD), float("nan"), dtype=f64)], 0)
        rows = (torch.arange(B)[:, None] * L + key[None, :]).reshape(-1)
        vx = to4(arena[rows], B, H, LMAX)
    s = q4 @ kx.transpose(-1, -2)                                       # [B, H, L, 128]
    r = Emu()
    r.n = vis_ref.sum(-1)
    sr = s.masked_fill(~vis_ref[:, None], float("-inf"))
    mr = sr.max(-1, keepdim=True).values
    pr = torch.exp2(sr - torch.where(torch.isinf(mr), torch.zeros_like(mr), mr))
    lr = pr.sum(-1, keepdim=True)
    r.o_ref = (pr[..., :L] @ v4) / lr.clamp_min(1e-300)
    se = s.masked_fill(~adm[:, None], float("-inf"))
    me = se.max(-1, keepdim=True).values
    p0 = torch.exp2(se - torch.where(torch.isinf(me), torch.zeros_like(me), me))   # a query without a key: m = 0, every P = exp2(-inf) = 0
    p0 = torch.where(p0 < 2.0 ** -126, torch.zeros_like(p0), p0)        # the kernel's P is an fp32 number
    p16 = p0 if mut == "skip_p_round" else rnd(p0, bf16)
    l = (p16 if mut == "l_rounded" else p0).sum(-1, keepdim=True)
    inv = torch.where(l > 0, 1.0 / l.clamp_min(1e-300), torch.zeros_like(l))
    o = torch.zeros((B, H, L, HD), dtype=f64)
    for t in range(nt):                                                 # one wave: 16 queries, the staged keys 0 .. 32 nk32 - 1
        rows, staged = slice(16 * t, min(16 * t + 16, L)), 32 * ((t + 2) >> 1)
        o[:, :, rows] = p16[:, :, rows, :staged] @ vx[:, :, :staged]
    r.o = rnd(o * inv, bf16)
    return r


def inputs(batch, heads, L, qamp=1.0, seed=11):
    """the Part 2 operands, token-major bf16 [batch * L, heads * 64]: N(0, 1), q times qamp and prescaled by scale * log2 e, rounded once"""
    C = heads * HD
    q2 = (_rand((batch * L, C), "cpu", seed + L).to(f64) * (qamp * PRESCALE)).to(bf16)
    return q2, _rand((batch * L, C), "cpu", seed + L + 1).to(bf16), _rand((batch * L, C), "cpu", seed + L + 2).to(bf16)


def bad_rows(o, want):
    """the (sample, head, query) rows of o [batch, heads, L, 64] float64 that are not `want` bit for bit as bf16, or not finite"""
    same = (o.to(bf16) == want.to(bf16)).all(-1) & torch.isfinite(o).all(-1)
    return int((~same).sum())


# ------------------------------------------------------------------------------------------- seer_embed_tokens
EMBED_C = (8, 768, 1016, 1024, 1032, 2056)


def embed_tables(vocab, L_max, C, seed=0):
    """tok [vocab, C], pos [L_max, C] bf16: arbitrary bit patterns without inf / NaN; every eighth column (c % 8 == 3) holds the pairs
    whose fp32 sum is a bf16 tie: tok 1 or 1 + 2^-7 by row, pos 2^-8 -- 1 + 2^-8 rounds DOWN to the even 1, 1 + 2^-7 + 2^-8 rounds UP to
    the even 1 + 2^-6 -- and, in every other pair of rows, their negatives, whose sums -(1 - 2^-8) and -(1 + 2^-8) are exact and a tie"""
    def bits(rows, s):
        g = torch.Generator().manual_seed(s)
        b = torch.randint(0, 65536, (rows, C), generator=g, dtype=torch.int32)
        b = torch.where((b & 0x7F80) == 0x7F80, b & ~0x0080, b)
        return (b - ((b & 0x8000) << 1)).to(torch.int16).view(bf16)
    tok, pos = bits(vocab, 4000 + seed + C), bits(L_max, 5000 + seed + C)
    tie = torch.arange(C) % 8 == 3
    rt = torch.arange(vocab)[:, None]
    tok_t = ((1.0 - 2.0 * ((rt // 2) % 2)) * (1.0 + 2.0 ** -7 * (rt % 2))).expand(vocab, C)
    tok = torch.where(tie, tok_t.to(bf16), tok)
    pos = torch.where(tie, torch.full((L_max, C), 2.0 ** -8).to(bf16), pos)
    return tok, pos


def embed_ref(ids, tok, pos):
    """ids int64 [batch, L] -> bf16 [batch * L, C]: (tok[clamp(ids)].float() + pos[l].float()).to(bf16)"""
    b, L = ids.shape
    return (tok[ids.clamp(0, tok.shape[0] - 1)].float() + pos[:L].float()[None]).to(bf16).reshape(b * L, -1)
