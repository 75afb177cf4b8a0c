"""The two kernels of the CLIP text tower (csrc/clip_text.hip) tested exactly, per query row and at their edges: the part of the matrix
series (test_gpu_f16_matrix.py, test_gpu_train_matrix.py, test_gpu_attn_fwd_matrix.py, ...) for seer_attn_causal64, the one MFMA attention
kernel that series had left out, and for seer_embed_tokens.  The older tests (test_gpu_clip_text.py, unchanged) compare N(0, 1) problems over
the whole tensor with rtol 2e-2 / atol 1e-2: the softmax is nearly uniform there (p about 1 / L), so two keys swapped in the V order of
the LDS stage move an element by about |v_a - v_b| / L -- 0.018 at L = 77 --, and one masked key admitted among 77 by 1/77 of a value:
both at the edge of that bound.  Five parts (constructions, reference, emulation and mutations: tests/clip_matrix_ref.py, plain torch
on the CPU; nothing in any bound comes from the kernel):

1. EXACT, zero tolerance, every query row of every case: L in {1, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 77, 96, 97, 127, 128} (every
   count of key tiles 1 .. 8, both parities of nk32, one before, at and after each tile edge) x ten masks (the six kinds of
   test_gpu_clip_text._mask; only the last key hidden; a whole 16-key tile hidden; the even tile of a 32-key pair hidden and its odd tile
   visible; every other key hidden) in (batch, heads) = (1, 1), (2, 2), (3, 3) by turns, and (1, 12) at L = 77.
   SELECTOR: K holds j, j^2 // 256, j^2 % 256 and Q holds 512 t, -65536, -256 in three columns, so the score is 256 (t^2 - (j - t)^2), an
   integer below 2^24, P is one-hot on the visible key nearest to the query's target t, and O[i] = V[that key] bit for bit for V of
   arbitrary finite bf16 bit patterns: the pos permutation of the V stage and the visibility rule key by key.  Targets: t = i (key <= q, not
   <), t = i + 1 (the diagonal key instead), any t <= i (a masked target falls back to its neighbour: the mask is read per key), and on
   small dyadic V hidden targets between two visible keys (a tie: the mean of the two).
   UNIFORM: Q = 0, every visible P = 2^0, V a function of a key's rank among the visible ones (RAMP, BALANCE and LEVEL columns
   interleaved), so that (sum of the visible V) / n_i is exact for every row of every mask: a dropped key, a masked key or a key past L in
   the denominator.  Queries with no visible key come out as zeros exactly, and their neighbours do not.
   INDEPENDENCE on N(0, 1) data, bit for bit: O[<= i] of Q, K, V rows past i; O of K, V at masked keys; the O of one (sample, head) of where
   that sample and head sit in batch x heads, in a wider fused projection and a wider output row.
   Every exact case runs twice and repeats its bits.
2. PER OWN ROW -- one (sample, head, query) vector of 64 values -- against the float64 softmax formula on N(0, 1) inputs, q prescaled, and
   with q x 3: |got - ref|_2 / max(|ref|_2, 2^-6 rms row norm).  The kernel's worst row must be within 2x the worst row of the float64
   emulation that rounds only where the kernel rounds (P to bf16 for the P V product, the denominator from the unrounded P, O to bf16); 2x
   is the project's margin for 16-bit emulations (test_gpu_attn_fwd_matrix.py, test_gpu_clip_text.py).
3. The mutation table runs on the CPU (tests/test_clip_matrix_ref_cpu.py).
4. seer_embed_tokens bit for bit: C in {8, 768, 1016, 1024, 1032, 2056} (the first, second and third pass of the `c += 1024` loop and a
   ragged last pass), ldx == C and ldx = C + 8 into a NaN arena with a guard row, L < L_max with batch 3 (row % L is not row) and
   L == L_max, ids 0, vocab - 1, outside the table on both sides up to +-2^40, vocab = 1, arbitrary bit patterns and planted rounding ties.
5. Every SEER_EINVAL / SEER_ENOSYS branch of both entry points with real buffers: the code, and NaN-filled outputs keep their bits.

Every attention case runs on the sentinel layout (_call): Q, K, V are column slices, 8 spare columns apart, of ONE NaN-filled
[batch * L + 1, 3 * heads * 64 + 16] buffer; O is columns 4 .. 4 + heads * 64 of a NaN-filled [batch * L + 1, heads * 64 + 12] buffer (8-byte
aligned, a row stride that is a multiple of 4 and not of 8).  After the call the inputs and the mask keep their bits, everything outside
the O slice keeps its NaN bits, O is finite: a read of the guard row (the clamps to L - 1 and the `key < L` guard of the V stage prevent
it) or of a spare column would show as NaN in O.

Covered here for the first time, and the assertion that covers each: the second and third iteration of `c += 1024` (test_embed_edges at
C = 1032 and 2056) . the half-empty last 32-key step of an odd number of key tiles (test_exact at L = 1, 15, 16, 33, 48, 65, 77, 97 for the
last query tile, where the odd half lies past L, and in every case for the query tiles 0, 2, 4, 6, where it holds later keys) . every key position of pos (test_exact, selector diag: query i
selects key i, in each of the four 16-column tiles of O) . O's row stride % 8 == 4 and ldx > C (_call, test_embed_edges).

FOUND BY THIS FILE: nothing.  Both kernels pass every assertion as they were; the measured figures, the mutation table and the run times
are in profiles/clip_matrix.md."""
import pytest
import torch

from tests import clip_matrix_ref as R
from tests.test_gpu_f16_matrix import _eq, _rand
from tests.test_gpu_train_matrix import _row_err

pytestmark = pytest.mark.gpu
bf16, f64 = torch.bfloat16, torch.float64
EINVAL, ENOSYS = -22, -38


def _nan(dev, rows, cols):
    return torch.full((rows, cols), float("nan"), device=dev, dtype=bf16)


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def _call(dev, q2, k2, v2, m, batch, heads, L, wide=0, what=""):
    """one launch on the sentinel layout (module docstring); `wide`: that many more columns in both buffers.  q2, k2, v2: [batch * L,
    heads * 64] bf16 (any device), m: uint8 [batch, L] or None.  Returns O, a view of its NaN buffer"""
    from seervideoldm_amd import ops
    C, T = heads * 64, batch * L
    assert wide % 8 == 0
    inb, obuf = _nan(dev, T + 1, 3 * C + 16 + wide), _nan(dev, T + 1, C + 12 + wide)
    q, k, v = inb[:T, :C], inb[:T, C + 8:2 * C + 8], inb[:T, 2 * C + 16:3 * C + 16]
    q.copy_(q2), k.copy_(k2), v.copy_(v2)
    out = obuf[:T, 4:4 + C]
    assert out.stride(0) % 8 == 4 and out.data_ptr() % 8 == 0 and all(t.data_ptr() % 16 == 0 for t in (q, k, v))
    md = None if m is None else m.to(dev)
    before = [inb.clone(), obuf.clone(), None if md is None else md.clone()]
    ops.attn_causal64(q, k, v, out, batch=batch, heads=heads, L=L, key_mask=md)
    assert _bits_equal(inb, before[0]) and (md is None or torch.equal(md, before[2])), f"{what}: the kernel wrote into its inputs"
    keep = torch.ones(obuf.shape, dtype=torch.bool, device=dev)
    keep[:T, 4:4 + C] = False
    moved = obuf.view(torch.int16)[keep] != before[1].view(torch.int16)[keep]
    assert not bool(moved.any()), f"{what}: {int(moved.sum())} stores outside the O slice (spare columns / guard row)"
    assert bool(torch.isfinite(out.float()).all()), f"{what}: O not finite (an element not written, or a read of the guard row / a spare column)"
    return out


def _twice(dev, q2, k2, v2, m, batch, heads, L, what, wide=0):
    a = _call(dev, q2, k2, v2, m, batch, heads, L, wide, what)
    b = _call(dev, q2, k2, v2, m, batch, heads, L, wide, what)
    assert _bits_equal(a.contiguous(), b.contiguous()), f"{what}: the second run gives other bits"
    return a


def test_prescale_is_the_products():
    from seervideoldm_amd import ops
    assert R.PRESCALE == ops.qk_prescale(64)


# =========================================================================================== 1. exact, zero tolerance
@pytest.mark.parametrize("L", R.LENGTHS)
def test_exact(device, L):
    """selector (diag, beyond, spread, ties) and uniform runs of every mask, in the layout of its turn; every row compared"""
    for kind in R.MASKS:
        for batch, heads in R.layouts(L, kind):
            vis = R.visible(R.mask(kind, batch, L), batch, L)
            for name, q4, k4, v4, want4, m in R.exact_runs(L, kind, batch, heads):
                what = f"L{L} {kind} b{batch} h{heads} {name}"
                q2, k2, v2 = (R.to2(t).to(bf16) for t in (q4, k4, v4))
                out = _twice(device, q2, k2, v2, m, batch, heads, L, what)
                _eq(out, R.to2(want4).to(device), bf16, what)
                if name == "uniform":
                    o = out.float().reshape(batch, L, heads, 64)
                    none = (~vis.any(-1)).to(device)
                    assert bool((o[none] == 0).all()), f"{what}: a query without a visible key is not zeros"
                    assert bool((o[~none].abs().sum(-1) > 0).all()), f"{what}: a neighbour of a query without a key was zeroed with it"


def _random_case(dev, L, kind, batch, heads, seed=11):
    q2, k2, v2 = R.inputs(batch, heads, L, seed=seed)
    return q2, k2, v2, R.mask(kind, batch, L)


@pytest.mark.parametrize("L", R.LENGTHS)
def test_independent_of_later_rows(device, L):
    """other finite Q, K, V rows at every position past i: O[<= i] keeps its bits (the cut before, at and after a tile edge, and the last)"""
    for kind in ("null", "holes"):
        batch, heads = R.layouts(L, kind)[0]
        q2, k2, v2, m = _random_case(device, L, kind, batch, heads)
        base = _twice(device, q2, k2, v2, m, batch, heads, L, f"L{L} {kind}")
        o2 = [_rand((batch * L, heads * 64), "cpu", 50 + n, 3.0).to(bf16) for n in range(3)]
        for cut in sorted({c for c in (0, 14, 15, 16, 31, 32, L // 2, L - 2) if 0 <= c < L - 1}):
            later = (torch.arange(batch * L) % L > cut)[:, None]
            qc, kc, vc = (torch.where(later, o, t) for o, t in zip(o2, (q2, k2, v2)))
            got = _call(device, qc, kc, vc, m, batch, heads, L, what=f"L{L} {kind} cut {cut}")
            keep = ~later[:, 0].to(device)
            assert _bits_equal(got[keep], base[keep]), f"L{L} {kind}: rows past {cut} reach O[<= {cut}]"
            assert L < 3 or not _bits_equal(got[~keep], base[~keep])                # the changed rows did change theirs


@pytest.mark.parametrize("L", R.LENGTHS)
def test_independent_of_masked_keys(device, L):
    """other finite K, V at the keys the mask hides: O keeps its bits"""
    for kind in ("len1", "len20", "holes", "zero", "last", "tile", "even", "comb"):
        batch, heads = R.layouts(L, kind)[0]
        q2, k2, v2, m = _random_case(device, L, kind, batch, heads)
        base = _twice(device, q2, k2, v2, m, batch, heads, L, f"L{L} {kind}")
        hidden = (m == 0).reshape(-1, 1)
        kc = torch.where(hidden, _rand(k2.shape, "cpu", 60, 3.0).to(bf16), k2)
        vc = torch.where(hidden, _rand(v2.shape, "cpu", 61, 3.0).to(bf16), v2)
        got = _call(device, q2, kc, vc, m, batch, heads, L, what=f"L{L} {kind} masked keys changed")
        assert _bits_equal(got.contiguous(), base.contiguous()), f"L{L} {kind}: K / V of a masked key reach O"


@pytest.mark.parametrize("L", R.ROW_LENGTHS)
def test_same_bits_in_every_layout(device, L):
    """the O of one (sample, head) alone in a (1, 1) launch, and as any slot of (2, 2), (3, 3), (1, 12), in a wider fused projection and a
    wider output row"""
    for n, (batch, heads) in enumerate(((2, 2), (3, 3), (1, 12))):
        kind = ("holes", "comb", "len20")[n]
        q2, k2, v2, m = _random_case(device, L, kind, batch, heads, seed=20 + n)
        full = _call(device, q2, k2, v2, m, batch, heads, L, wide=64, what=f"L{L} b{batch} h{heads} wide")
        for b in range(batch):
            for h in range(heads):
                rows, cols = slice(b * L, b * L + L), slice(64 * h, 64 * h + 64)
                one = _call(device, q2[rows, cols], k2[rows, cols], v2[rows, cols], m[b:b + 1], 1, 1, L, what=f"L{L} sample {b} head {h} alone")
                assert _bits_equal(full[rows, cols].contiguous(), one.contiguous()), f"L{L} b{batch} h{heads}: slot ({b}, {h}) differs from the same problem alone"


# =========================================================================================== 2. per own row against float64
@pytest.mark.parametrize("L", R.ROW_LENGTHS)
def test_rows(device, L):
    fails = []
    for kind in R.ROW_MASKS:
        batch, heads = R.layouts(L, kind)[0]
        m = R.mask(kind, batch, L)
        for qamp in (1.0, 3.0):
            q2, k2, v2 = R.inputs(batch, heads, L, qamp)
            r = R.emulate(*(R.to4(t.to(f64), batch, heads, L) for t in (q2, k2, v2)), m)
            tag = f"L{L} | {kind} | b{batch} h{heads} | q x {qamp:g}"
            out = _call(device, q2, k2, v2, m, batch, heads, L, what=tag)
            got4 = R.to4(out.cpu().to(f64), batch, heads, L)
            floor = R.row_floor(r.o_ref)
            e_emu, e_got = _row_err(r.o, r.o_ref, floor), _row_err(got4, r.o_ref, floor)
            print(f"clip_matrix part2 | {tag} | emulation {e_emu:.3e} | kernel {e_got:.3e} | ratio {e_got / max(e_emu, 1e-300):.3f}")
            if not e_got <= 2 * e_emu:
                fails.append(f"{tag}: worst row {e_got:.4g} > 2 x emulation = {2 * e_emu:.4g}")
    assert not fails, "\n".join(fails)


# =========================================================================================== 4. seer_embed_tokens
def _ids(batch, L, vocab, seed):
    ids = torch.randint(0, vocab, (batch, L), generator=torch.Generator().manual_seed(seed))
    wild = [0, vocab - 1, -1, vocab, -3, vocab + 10, -2 ** 40, 2 ** 40, -2 ** 31, 2 ** 31, 2 ** 32 + 1, -2 ** 63, 2 ** 63 - 1]
    flat = ids.reshape(-1)
    for n, w in enumerate(wild[:flat.numel()]):
        flat[(n * 7) % flat.numel()] = w
    return ids


@pytest.mark.parametrize("C", R.EMBED_C)
def test_embed_edges(device, C):
    from seervideoldm_amd import ops
    L_max = 77
    for vocab in (11, 1):
        tok, pos = R.embed_tables(vocab, L_max, C)
        tok_d, pos_d = tok.to(device), pos.to(device)
        for batch, L in ((3, 5), (3, 77), (1, 1)):
            ids = _ids(batch, L, vocab, seed=L)
            ref = R.embed_ref(ids, tok, pos).to(device)
            what = f"C{C} vocab {vocab} b{batch} L{L}"
            x = ops.embed_tokens(ids.to(device), tok_d, pos_d)                             # ldx == C
            assert x.shape == ref.shape and _bits_equal(x, ref), f"{what}: ldx == C"
            arena = _nan(device, batch * L + 1, C + 8)                                     # ldx == C + 8, guard row
            before = arena.clone()
            out = arena[:batch * L, :C]
            ops.embed_tokens(ids.to(device), tok_d, pos_d, out=out)
            assert _bits_equal(out.contiguous(), ref), f"{what}: ldx == C + 8"
            assert _bits_equal(arena[:, C:], before[:, C:]) and _bits_equal(arena[batch * L:], before[batch * L:]), f"{what}: a store outside the rows"
            assert _bits_equal(tok_d, tok.to(device)) and _bits_equal(pos_d, pos.to(device))


# =========================================================================================== 5. refusals on the device
def test_attn_refusals(device):
    from seervideoldm_amd import _lib
    lib = _lib.load()
    batch, heads, L = 2, 2, 77
    C, T = heads * 64, batch * L
    inb, obuf = torch.zeros((T + 1, 3 * C + 16), device=device, dtype=bf16), _nan(device, T + 1, C + 12)
    mask = torch.ones((batch, L), device=device, dtype=torch.uint8)
    before = obuf.clone()
    q, k, v, o = inb.data_ptr(), inb.data_ptr() + 2 * (C + 8), inb.data_ptr() + 2 * (2 * C + 16), obuf.data_ptr() + 8
    ok = dict(Q=q, K=k, V=v, ld=3 * C + 16, O=o, ldo=C + 12, mask=mask.data_ptr(), batch=batch, heads=heads, L=L)

    def attn(**kw):
        a = dict(ok, **kw)
        rc = lib.seer_attn_causal64(a["Q"], a["K"], a["V"], a["ld"], a["O"], a["ldo"], a["mask"], a["batch"], a["heads"], a["L"], None)
        torch.cuda.synchronize()
        assert rc == 0 or _bits_equal(obuf, before), f"a refused call wrote into O: {kw}"
        return rc

    for name in ("Q", "K", "V", "O"):
        assert attn(**{name: None}) == EINVAL
    assert attn(Q=q + 2) == EINVAL and attn(K=k + 8) == EINVAL and attn(V=v + 4) == EINVAL       # 16-byte alignment of the three slices
    assert attn(O=o + 4) == EINVAL and attn(O=o + 2) == EINVAL                                   # 8-byte alignment of O
    assert attn(batch=0) == EINVAL and attn(batch=-1) == EINVAL and attn(heads=0) == EINVAL and attn(heads=-2) == EINVAL
    assert attn(L=0) == EINVAL and attn(L=-77) == EINVAL
    assert attn(ld=C - 8) == EINVAL and attn(ld=3 * C + 12) == EINVAL                            # below heads * 64 / not a multiple of 8
    assert attn(ldo=C - 4) == EINVAL and attn(ldo=C + 2) == EINVAL                               # below heads * 64 / not a multiple of 4
    assert attn(L=129) == ENOSYS and attn(L=2 ** 31 - 1) == ENOSYS                               # the one-pass kernel ends at 128 keys
    assert attn(batch=2 ** 22, heads=1024, ld=2 ** 16, ldo=2 ** 16) == ENOSYS                    # more than 2^31 - 1 blocks
    assert attn(batch=2 ** 30, heads=1, L=2) == ENOSYS                                           # batch * L past 2^31 - 1
    assert attn() == 0                                                                           # the same arguments unchanged: a launch
    torch.cuda.synchronize()
    assert bool(torch.isfinite(obuf[:T, 4:4 + C].float()).all())


def test_embed_refusals(device):
    from seervideoldm_amd import _lib
    lib = _lib.load()
    batch, L, L_max, vocab, C = 2, 5, 7, 11, 64
    ids = torch.zeros((batch * L + 1,), device=device, dtype=torch.int64)
    tok, pos = torch.zeros((vocab, C + 8), device=device, dtype=bf16), torch.zeros((L_max, C + 8), device=device, dtype=bf16)
    x = _nan(device, batch * L + 1, C + 8)
    before = x.clone()
    ok = dict(ids=ids.data_ptr(), batch=batch, L=L, tok=tok.data_ptr(), vocab=vocab, pos=pos.data_ptr(), L_max=L_max, C=C, x=x.data_ptr(), ldx=C + 8)

    def emb(**kw):
        a = dict(ok, **kw)
        rc = lib.seer_embed_tokens(a["ids"], a["batch"], a["L"], a["tok"], a["vocab"], a["pos"], a["L_max"], a["C"], a["x"], a["ldx"], None)
        torch.cuda.synchronize()
        assert rc == 0 or _bits_equal(x, before), f"a refused call wrote into x: {kw}"
        return rc

    for name in ("ids", "tok", "pos", "x"):
        assert emb(**{name: None}) == EINVAL
    assert emb(ids=ok["ids"] + 4) == EINVAL and emb(tok=ok["tok"] + 8) == EINVAL and emb(pos=ok["pos"] + 8) == EINVAL and emb(x=ok["x"] + 8) == EINVAL
    assert emb(batch=0) == EINVAL and emb(batch=-1) == EINVAL and emb(L=0) == EINVAL and emb(L=-1) == EINVAL
    assert emb(L=L_max + 1) == EINVAL and emb(vocab=0) == EINVAL and emb(vocab=-1) == EINVAL
    assert emb(C=0) == EINVAL and emb(C=-8) == EINVAL and emb(C=60) == EINVAL                    # not a multiple of 8
    assert emb(ldx=C - 8) == EINVAL and emb(ldx=C + 4) == EINVAL                                 # below C / not a multiple of 8
    assert emb(batch=2 ** 30, L=2) == ENOSYS                                                     # batch * L past 2^31 - 1
    assert emb() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x[:batch * L, :C].float()).all()) and _bits_equal(x[:, C:], before[:, C:]) and _bits_equal(x[batch * L:], before[batch * L:])
