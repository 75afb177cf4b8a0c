"""The IEEE-half (SEER_EPI_F16 / SEER_ATTN_F16) instantiations tested as hard as the bf16 ones -- every shipped yaml says
mixed_precision: "fp16", so this is the engine a user of the unchanged scripts runs.  Three parts:

1. EXACT arithmetic, both storage types: integer inputs make every product and partial sum an integer below 2^24, the fp32
   accumulator is exact whatever the order, and the one rounding to 16 bits is fully determined (round to nearest even).  Zero
   tolerance: a dropped K element, a tail element read twice or a truncating store cannot hide.  Plus what only fp16 has: the range
   that ends at 65504 and subnormals below 6.1e-5.
2. fp16 tolerance matrix with a DERIVED per-element bound (one rounding to 11 bits + worst-case fp32 accumulation).
3. fp16 attention: the routing boundary at 256 keys, the refusals, sharp softmax against an emulation that rounds where the kernel
   rounds, and a re-base staircase that makes a skipped / doubled rescale of the d = 40 tracked form an O(1) error.

All references are plain torch in float64 on inputs already rounded to the storage type.  Measured values: profiles/f16_matrix.md."""
import math

import pytest
import torch
import torch.nn.functional as Fn

from tests.test_gpu_f16 import _close as _close_f16

pytestmark = pytest.mark.gpu

f16, bf16, f64 = torch.float16, torch.bfloat16, torch.float64
DTS = [pytest.param(f16, id="f16"), pytest.param(bf16, id="bf16")]
T320 = 22


def _ints(shape, dev, seed, lo=-3, hi=3):
    """integers in [lo, hi] as float64 on the device"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(dev).to(f64)


def _store(x64, dt):
    """to the storage type, asserting that nothing was rounded"""
    x = x64.to(dt)
    assert torch.equal(x.to(f64), x64), "test input is not exact in the storage type"
    return x


def _rand(shape, dev, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev)


def _exact_pre(K, amax, wmax, *terms):
    """every partial sum of the accumulator is an integer (or a multiple of 2^-k the caller scaled by) below 2^24"""
    assert K * amax * wmax + sum(terms) < 2 ** 24


def _eq(got, ref64, dt, what):
    """bit equality with the float64 reference rounded ONCE (torch's cast is round-to-nearest-even)"""
    want = ref64.to(torch.float32) if got.dtype == torch.float32 else ref64.to(dt)
    if got.dtype == torch.float32:
        assert torch.equal(want.to(f64), ref64), "reference not exact in fp32"
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    same = (got == want) | (got.isnan() & want.isnan())
    if not bool(same.all()):
        idx = (~same).nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int((~same).sum())}/{same.numel()} elements differ; first at {idx}: got "
                             f"{got[tuple(idx)].item()!r} want {want[tuple(idx)].item()!r} (exact {ref64[tuple(idx)].item()!r})")


def _gemm_case(dev, dt, M, N, K, seed=0, a2k=0, hi=3, nonneg=False):
    lo = 0 if nonneg else -hi
    a64, w64 = _ints((M, K), dev, seed + 1, lo, hi), _ints((N, K), dev, seed + 2, lo, hi)
    return a64, w64, _store(a64, dt), _store(w64, dt)


# =========================================================================================== 1. exact arithmetic
_TILE_SHAPES = [
    (1, 256, 128, 64), (1, 300, 132, 192), (2, 256, 128, 64), (2, 100, 64, 128), (3, 256, 128, 64), (3, 130, 68, 192),
    (5, 512, 256, 1280), (5, 300, 132, 192), (6, 512, 256, 1280), (6, 130, 68, 192), (7, 1536, 1280, 1280), (7, 130, 68, 192),
    (8, 384, 320, 2560), (8, 100, 64, 128), (9, 6144, 640, 128), (9, 1848, 640, 768), (10, 384, 320, 2560), (10, 100, 64, 128),
    (11, 1536, 1280, 1280), (11, 300, 132, 192), (12, 384, 320, 320), (12, 130, 68, 192), (13, 384, 320, 2560), (13, 1000, 640, 128),
    (14, 512, 256, 1280), (14, 300, 132, 192), (15, 24576, 320, 320), (15, 1000, 64, 320), (16, 1536, 320, 1280), (16, 1000, 320, 320),
    (17, 384, 320, 320), (17, 130, 68, 192), (18, 1536, 640, 640), (18, 100, 64, 128), (21, 512, 512, 64), (21, 512, 256, 1280),
    (21, 300, 132, 192),
]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("tile,M,N,K", _TILE_SHAPES)
def test_exact_gemm_every_tile(device, dt, tile, M, N, K):
    """every explicit tile code, one aligned and one ragged shape: bias + column scale 0.5 + residual on signed integers (fp32 and
    16-bit output), then non-negative integers drawn from a range that shrinks with K so that the sums sit near 12 000 at every
    shape, where the 16-bit store rounds most elements (asserted on the reference; half ulp 8, bf16 ulp 64): pins
    round-to-nearest-even in every tile's epilogue"""
    from seervideoldm_amd import ops
    a64, w64, a, w = _gemm_case(device, dt, M, N, K)
    bias64, res64 = _ints((N,), device, 3, -8, 8), _ints((M, N), device, 4, -8, 8)
    res = _store(res64, dt)
    cols = min(64, N)
    _exact_pre(K, 3, 3, 8, 8)
    ref = a64 @ w64.t() + bias64
    ref[:, :cols] *= 0.5
    ref = ref + res64
    assert ref.abs().max() < 60000
    kw = dict(bias=bias64.float(), residual=res, col_scale=(0.5, cols), tile=tile, splits=1)
    _eq(ops.gemm(a, w, out_f32=True, **kw), ref, dt, f"tile {tile} {M}x{N}x{K} fp32 out")
    _eq(ops.gemm(a, w, **kw), ref, dt, f"tile {tile} {M}x{N}x{K} 16-bit out")
    hi = int(round((48000.0 / K) ** 0.5))          # sums of about 12 000 at every K: half ulp 8, bf16 ulp 64
    a64, w64, a, w = _gemm_case(device, dt, M, N, K, seed=10, hi=hi, nonneg=True)
    _exact_pre(K, hi, hi)
    ref = a64 @ w64.t()
    assert ref.abs().max() < 60000 and (ref.to(dt).to(f64) != ref).double().mean() > 0.5, "the store must round most elements"
    _eq(ops.gemm(a, w, tile=tile, splits=1), ref, dt, f"tile {tile} {M}x{N}x{K} rounding of large sums")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K,a2k", [(1000, 320, 320, 0), (1283, 192, 640, 0), (4096, 136, 320, 0), (1536, 200, 640, 0),
                                       (1100, 1000, 320, 0), (6144, 640, 640, 320), (24576, 320, 640, 320)])
def test_exact_gemm_weight_stationary(device, dt, M, N, K, a2k):
    """tile 19 (the weight-stationary persistent kernel) and tile 20 (AUTO restricted to the tile kernel) on row tails, column tails
    and two K sources: both exact, hence equal"""
    from seervideoldm_amd import ops
    a64, w64 = _ints((M, K), device, 1), _ints((N, K), device, 2)
    a = _store(a64[:, :K - a2k].contiguous(), dt)
    a2 = _store(a64[:, K - a2k:].contiguous(), dt) if a2k else None
    w = _store(w64, dt)
    bias64 = _ints((N,), device, 3, -8, 8)
    cols = min(64, N)
    _exact_pre(K, 3, 3, 8)
    ref = a64 @ w64.t() + bias64
    ref[:, :cols] *= 0.5
    assert ref.abs().max() < 60000
    for tile in (19, 20, 0):
        _eq(ops.gemm(a, w, a2=a2, bias=bias64.float(), col_scale=(0.5, cols), tile=tile), ref, dt, f"tile {tile} {M}x{N}x{K}")


@pytest.mark.parametrize("tile", [0, T320])
@pytest.mark.parametrize("M,N,K,splits", [(512, 640, 320, 1), (1536, 1280, 1280, 1), (6144, 640, 640, 1), (384, 320, 320, 1),
                                          (300, 960, 192, 1), (1536, 1280, 5120, 0), (6144, 640, 2560, 3)])
def test_exact_gemm_f16_where_bf16_takes_the_256x320_tile(device, tile, M, N, K, splits):
    """the projection shapes bf16 hands to the 256 x 320 kernel: that kernel refuses IEEE half, so AUTO lands on another tile and an
    explicit SEER_TILE_T256x320 must fall through to one -- and still be exact"""
    from seervideoldm_amd import ops
    a64, w64, a, w = _gemm_case(device, f16, M, N, K)
    bias64, res64 = _ints((N,), device, 3, -8, 8), _ints((M, N), device, 4, -8, 8)
    _exact_pre(K, 3, 3, 8, 8)
    ref = a64 @ w64.t() + bias64 + res64
    assert ref.abs().max() < 60000
    _eq(ops.gemm(a, w, bias=bias64.float(), residual=_store(res64, f16), tile=tile, splits=splits), ref, f16, f"tile {tile} {M}x{N}x{K}")


@pytest.mark.parametrize("tile", [0, T320])
@pytest.mark.parametrize("n_img,H,W,Ci,Co,stride,splits", [(4, 16, 16, 320, 320, 1, 1), (24, 8, 8, 640, 640, 1, 0), (24, 4, 4, 1280, 1280, 1, 0),
                                                           (2, 32, 32, 320, 320, 2, 1), (2, 6, 10, 64, 320, 1, 1)])
def test_exact_conv_f16_where_bf16_takes_the_256x320_tile(device, tile, n_img, H, W, Ci, Co, stride, splits):
    from seervideoldm_amd import ops
    from seervideoldm_amd.weights import pack_conv3x3
    x64, w64 = _ints((n_img, Ci, H, W), device, 1), _ints((Co, Ci, 3, 3), device, 2)
    bias64 = _ints((Co,), device, 3, -8, 8)
    _exact_pre(9 * Ci, 3, 3, 8)
    ref = Fn.conv2d(x64, w64, bias64, stride=stride, padding=1).permute(0, 2, 3, 1).reshape(-1, Co)
    assert ref.abs().max() < 60000
    x_cl = _store(x64.permute(0, 2, 3, 1).reshape(-1, Ci).contiguous(), f16)
    out = ops.conv3x3(x_cl, pack_conv3x3(_store(w64, f16)), n_img, H, W, stride=stride, bias=bias64.float(), tile=tile, splits=splits)
    _eq(out, ref, f16, f"conv tile {tile} {Ci}->{Co}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K,splits", [(384, 1280, 1280, 0), (384, 1280, 5120, 4), (200, 68, 1024, 3), (300, 132, 1280, 5), (1536, 1280, 5120, 0)])
def test_exact_gemm_split_k(device, dt, M, N, K, splits):
    """split-K (fp32 slices, ordered reduce pass with the epilogue): bias, per-batch row vector, residual; explicit slice counts and AUTO"""
    from seervideoldm_amd import ops
    a64, w64, a, w = _gemm_case(device, dt, M, N, K)
    bias64, res64, rv64 = _ints((N,), device, 3, -8, 8), _ints((M, N), device, 4, -8, 8), _ints((2, N), device, 5, -8, 8)
    _exact_pre(K, 3, 3, 8, 8, 8)
    ref = a64 @ w64.t() + bias64 + rv64.repeat_interleave(M // 2, 0) + res64
    assert ref.abs().max() < 60000
    kw = dict(bias=bias64.float(), residual=_store(res64, dt), rowvec=rv64.float(), rows_per_batch=M // 2, splits=splits)
    _eq(ops.gemm(a, w, **kw), ref, dt, f"split-K {M}x{N}x{K} s{splits}")
    kw.pop("residual")
    _eq(ops.gemm(a, w, out_f32=True, **kw), ref - res64, dt, f"split-K {M}x{N}x{K} s{splits} fp32 out")
    ref2 = a64 @ w64.t()
    ref2[:, :N // 2 // 4 * 4] *= 0.5
    _eq(ops.gemm(a, w, col_scale=(0.5, N // 2 // 4 * 4), splits=splits), ref2, dt, "split-K column scale")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n_img,H,W,Ci,Co,stride,up,pad_after,splits", [
    (2, 8, 8, 64, 64, 1, False, False, 1), (2, 16, 16, 64, 128, 2, False, False, 1), (2, 8, 8, 64, 64, 1, True, False, 1),
    (3, 16, 24, 128, 64, 2, False, True, 1), (3, 6, 10, 64, 68, 1, False, False, 1), (3, 6, 10, 64, 68, 2, False, False, 1),
    (6, 4, 4, 640, 320, 1, False, False, 0), (6, 4, 4, 640, 320, 1, False, False, 5), (6, 4, 4, 640, 320, 1, False, False, 3),
    (4, 8, 8, 1280, 1280, 1, False, False, 0),
])
def test_exact_conv3x3(device, dt, n_img, H, W, Ci, Co, stride, up, pad_after, splits):
    """implicit-GEMM conv: stride 1 / 2, behind the nearest-2x upsample, padded after only, odd sizes, split-K explicit and AUTO; the
    bias, a per-batch row vector and a residual in the epilogue"""
    from seervideoldm_amd import ops
    from seervideoldm_amd.weights import pack_conv3x3
    x64, w64 = _ints((n_img, Ci, H, W), device, 1), _ints((Co, Ci, 3, 3), device, 2)
    bias64 = _ints((Co,), device, 3, -8, 8)
    _exact_pre(9 * Ci, 3, 3, 8, 8, 8)
    xin = Fn.interpolate(x64, scale_factor=2.0, mode="nearest") if up else x64
    if pad_after:
        ref = Fn.conv2d(Fn.pad(xin, (0, 1, 0, 1)), w64, bias64, stride=stride)
    else:
        ref = Fn.conv2d(xin, w64, bias64, stride=stride, padding=1)
    Ho, Wo = ref.shape[2:]
    ref = ref.permute(0, 2, 3, 1).reshape(-1, Co)
    rv64, res64 = _ints((n_img, Co), device, 4, -8, 8), _ints((ref.shape[0], Co), device, 5, -8, 8)
    ref = ref + rv64.repeat_interleave(Ho * Wo, 0) + res64
    assert ref.abs().max() < 60000
    x_cl = _store(x64.permute(0, 2, 3, 1).reshape(-1, Ci).contiguous(), dt)
    out = ops.conv3x3(x_cl, pack_conv3x3(_store(w64, dt)), n_img, H, W, stride=stride, upsample=up, pad_after_only=pad_after,
                      bias=bias64.float(), rowvec=rv64.float(), rows_per_batch=Ho * Wo, residual=_store(res64, dt), splits=splits)
    _eq(out, ref, dt, f"conv {Ci}->{Co} s{stride} up{up} pad_after{pad_after} splits{splits}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("tile", [0, 5, 8, 12, 21])
@pytest.mark.parametrize("n_img,H,W,Ci,Co", [(2, 8, 8, 64, 64), (2, 6, 10, 64, 68), (3, 4, 4, 128, 192)])
def test_exact_conv_up2x_phases(device, dt, tile, n_img, H, W, Ci, Co):
    """the four phase convs of nearest-2x + conv3x3: integer taps keep the summed phase weights integer (at most 4 taps: |w| <= 12)"""
    from seervideoldm_amd import ops
    from seervideoldm_amd.weights import pack_conv3x3_up_phases
    x64, w64 = _ints((n_img, Ci, H, W), device, 1), _ints((Co, Ci, 3, 3), device, 2)
    bias64 = _ints((Co,), device, 3, -8, 8)
    _exact_pre(4 * Ci, 3, 12, 8)
    ref = Fn.conv2d(Fn.interpolate(x64, scale_factor=2.0, mode="nearest"), w64, bias64, padding=1).permute(0, 2, 3, 1).reshape(-1, Co)
    w4 = pack_conv3x3_up_phases(w64.float())
    assert torch.equal(w4, w4.round()) and w4.abs().max() <= 12 and ref.abs().max() < 60000
    x_cl = _store(x64.permute(0, 2, 3, 1).reshape(-1, Ci).contiguous(), dt)
    out = ops.conv_up2x(x_cl, _store(w4.to(f64), dt), n_img, H, W, bias=bias64.float(), tile=tile)
    _eq(out, ref, dt, f"conv_up2x {Ci}->{Co} tile {tile}")


@pytest.mark.parametrize("dt", DTS)
def test_exact_gemm_batched_and_strided_views(device, dt):
    from seervideoldm_amd import ops
    Bt, M, N, K = 3, 256, 192, 128
    a64, w64 = _ints((Bt, M, K), device, 1), _ints((Bt, N, K), device, 2)
    _exact_pre(K, 3, 3)
    ref = torch.einsum("bmk,bnk->bmn", a64, w64)
    assert ref.abs().max() < 60000
    a, w = _store(a64, dt), _store(w64, dt)
    _eq(ops.gemm_batched(a, w), ref, dt, "batched")
    _eq(ops.gemm_batched(a, w, trans_out=True), ref.transpose(1, 2).contiguous(), dt, "batched, transposed store")
    _eq(ops.gemm_batched(a, w, out_f32=True), ref, dt, "batched, fp32 out")
    # A and C as column slices of wider buffers; the other half of the output buffer stays untouched
    M, K, N = 500, 320, 328
    big64, w64 = _ints((M, 3 * K), device, 3), _ints((N, K), device, 4)
    _exact_pre(K, 3, 3)
    big = _store(big64, dt)
    outbig = torch.zeros((M, 2 * N), device=device, dtype=dt)
    ops.gemm(big[:, K:2 * K], _store(w64, dt), out=outbig[:, N:])
    assert (big64[:, K:2 * K] @ w64.t()).abs().max() < 60000
    _eq(outbig[:, N:], big64[:, K:2 * K] @ w64.t(), dt, "strided gemm")
    assert (outbig[:, :N] == 0).all()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind,shape,tile,splits", [
    ("gemm", (1536, 640, 640), 0, 0), ("gemm", (3072, 320, 320), 16, 1), ("gemm", (768, 1280, 2560), 0, 0), ("gemm", (1024, 1280, 5120), 5, 4),
    ("conv", (8, 16, 16, 640, 640), 0, 0), ("conv", (24, 4, 4, 1280, 1280), 0, 0), ("conv", (8, 16, 16, 640, 640), 8, 1),
    ("up", (4, 8, 8, 640, 640), 0, 0),
])
def test_exact_column_sums(device, dt, kind, shape, tile, splits):
    """colsum_batch: the fixed-point (sum, sum of squares) a launch accumulates next to its output equal the float64 sums of the stored
    integers EXACTLY.  |result| <= 256 (bf16) / 2048 (fp16), so the stored value is the fp32 value and it does not matter which of
    the two a producer sums; inputs from {-1, 0, 1} with one operand sparse keep the results that small."""
    from seervideoldm_amd import ops
    B = 2
    arena = ops.FxArena(device, 1 << 18)
    lim = 2048 if dt == f16 else 256

    def sparse(shp, seed, keep):
        m = (torch.rand(shp, generator=torch.Generator().manual_seed(seed + 100)) < keep).to(device)
        return _ints(shp, device, seed, -1, 1) * m
    if kind == "gemm":
        M, N, K = shape
        a64, w64 = sparse((M, K), 1, 0.25), _ints((N, K), device, 2, -1, 1)
        bias64, res64 = _ints((N,), device, 3, -4, 4), _ints((M, N), device, 4, -4, 4)
        ref = a64 @ w64.t() + bias64 + res64
        y = ops.gemm(_store(a64, dt), _store(w64, dt), bias=bias64.float(), residual=_store(res64, dt), tile=tile, splits=splits,
                     colsum_batch=(B, arena))
    else:
        n_img, H, W, Ci, Co = shape
        x64, w64 = sparse((n_img, Ci, H, W), 1, 0.25 if kind == "conv" else 0.5), _ints((Co, Ci, 3, 3), device, 2, -1, 1)
        bias64 = _ints((Co,), device, 3, -4, 4)
        x_cl = _store(x64.permute(0, 2, 3, 1).reshape(-1, Ci).contiguous(), dt)
        if kind == "up":
            from seervideoldm_amd.weights import pack_conv3x3_up_phases
            ref = Fn.conv2d(Fn.interpolate(x64, scale_factor=2.0, mode="nearest"), w64, bias64, padding=1)
            y = ops.conv_up2x(x_cl, _store(pack_conv3x3_up_phases(w64.float()).to(f64), dt), n_img, H, W, bias=bias64.float(), tile=tile,
                              colsum_batch=(B, arena))
        else:
            from seervideoldm_amd.weights import pack_conv3x3
            ref = Fn.conv2d(x64, w64, bias64, padding=1)
            y = ops.conv3x3(x_cl, pack_conv3x3(_store(w64, dt)), n_img, H, W, bias=bias64.float(), tile=tile, splits=splits,
                            colsum_batch=(B, arena))
        ref = ref.permute(0, 2, 3, 1).reshape(-1, Co)
    assert ref.abs().max() <= lim, float(ref.abs().max())
    _eq(y, ref, dt, f"{kind} {shape}")
    assert isinstance(y.colsums, ops.ColSumsFx), "this launch was expected to accumulate its column sums"
    v = ref.reshape(B, -1, ref.shape[1])
    want = torch.stack([v.sum(1), (v * v).sum(1)], -1)
    assert want.abs().max() < 2 ** 43
    tot = y.colsums.totals()
    assert torch.equal(tot, want), f"column sums off by up to {(tot - want).abs().max().item()}"


# ------------------------------------------------------------------------- the edges only fp16 has
def test_f16_overflow_is_ieee(device):
    """POLICY PINNED HERE: a result beyond the half range leaves as +-inf, exactly where torch's own float32 -> float16 cast gives it
    (65520 and above; 65504..65519 round to 65504) -- IEEE overflow, the same as the reference under fp16 autocast.  No saturation,
    no NaN, and the neighbour in the same packed 32-bit word (pack2h writes two) is untouched."""
    from seervideoldm_amd import ops
    from seervideoldm_amd.weights import pack_conv3x3
    M, N, K = 256, 128, 128
    a64, w64, _, _ = _gemm_case(device, f16, M, N, K)
    bias64, res64 = _ints((N,), device, 3, -8, 8), _ints((M, N), device, 4, -8, 8)
    # rows (a tile corner, a ragged interior, the last row) that read only the first two K elements, against columns (odd and even
    # ones, neighbours in one packed word) whose first two weights put 255 w0 + w1 + bias + residual exactly at the edge
    rows = [0, 5, 17, 100, 255]
    targets = {0: 65504.0, 3: 65519.0, 4: 65520.0, 7: 70000.0, 33: 65536.0, 64: -65519.0, 65: -65520.0, 126: 1e5, 127: -1e5}
    a64[rows] = 0.0
    a64[rows, 0], a64[rows, 1] = 255.0, 1.0
    res64[rows] = 0.0
    for n, t in targets.items():
        w0 = float(int(t / 255.0))
        w64[n, 0], w64[n, 1] = w0, t - 255.0 * w0 - bias64[n].item()
    ref = a64 @ w64.t() + bias64 + res64
    _exact_pre(K, 255, 400, 8, 8)
    for n, t in targets.items():
        assert (ref[rows, n] == t).all()
    want = ref.to(f16)
    assert int(want.isinf().sum()) == 6 * len(rows) and not want.isnan().any() and (want[rows][:, [0, 3]] == 65504.0).all()
    assert ref[~want.isinf()].abs().max() < 65520 and (want[:, [1, 2, 5, 6, 32, 34, 66, 125]].abs() < 4000).all(), "the neighbours are ordinary values"
    out = ops.gemm(_store(a64, f16), _store(w64, f16), bias=bias64.float(), residual=_store(res64, f16))
    assert not out.isnan().any()
    _eq(out, ref, f16, "gemm at the end of the half range")
    _eq(ops.gemm(_store(a64, f16), _store(w64, f16), bias=bias64.float(), residual=_store(res64, f16), splits=2), ref, f16, "split-K at the end of the half range")
    # conv: all-ones 3x3 over a plateau
    n_img, H, W, Ci, Co = 1, 8, 8, 64, 64
    x64 = torch.zeros((n_img, Ci, H, W), device=device, dtype=f64)
    x64[0, :, 2:5, 2:5] = 16.0
    x64[0, :, 6, 6] = -16.0
    w64 = torch.zeros((Co, Ci, 3, 3), device=device, dtype=f64)
    w64[::2] = 8.0                 # even output channels: 9 * 64 * 16 * 8 = 73728 at the centre of the plateau -> inf; odd ones: 0
    w64[1::2, 0] = 1.0
    ref = Fn.conv2d(x64, w64, None, padding=1).permute(0, 2, 3, 1).reshape(-1, Co)
    _exact_pre(9 * Ci, 16, 8)
    want = ref.to(f16)
    assert want.isinf().any() and (want.isinf().sum() < want.numel() // 8) and not want.isnan().any()
    out = ops.conv3x3(_store(x64.permute(0, 2, 3, 1).reshape(-1, Ci).contiguous(), f16), pack_conv3x3(_store(w64, f16)), n_img, H, W)
    _eq(out, ref, f16, "conv at the end of the half range")


def test_f16_subnormals_are_kept(device):
    """operands below 6.1e-5 (subnormal in IEEE half): A = n * 2^-20 against integer W is exact in the fp32 accumulator, a subnormal
    residual adds exactly, and a result that lands subnormal is rounded to the 2^-24 grid -- nothing is flushed to zero."""
    from seervideoldm_amd import ops
    M, N, K = 300, 132, 192
    n64, w64 = _ints((M, K), device, 1, -15, 15), _ints((N, K), device, 2)
    a64 = n64 * 2.0 ** -20
    a, w = _store(a64, f16), _store(w64, f16)
    assert (a64.abs() < 6.1e-5).all()
    _exact_pre(K, 15, 3, 16)
    ref = a64 @ w64.t()
    for tile in (0, 2, 5, 12, 21):
        _eq(ops.gemm(a, w, out_f32=True, tile=tile), ref, f16, f"subnormal A, fp32 out, tile {tile}")
    res64 = _ints((M, N), device, 4, -15, 15) * 2.0 ** -24
    res = _store(res64, f16)
    _eq(ops.gemm(a, w, residual=res, out_f32=True), ref + res64, f16, "subnormal residual")
    out = ops.gemm(a, w, residual=res)
    want = (ref + res64).to(f16)
    sub = (want != 0) & (want.abs().to(f64) < 2.0 ** -14)
    assert int(sub.sum()) > want.numel() // 100, "the case must store subnormal results"
    _eq(out, ref + res64, f16, "subnormal results on the 16-bit store")


# =========================================================================================== 2. fp16 tolerance matrix, derived bound
def _bound(ref, absacc, K, out16=True, extra=None):
    """|out - ref| <= 2^-11 |ref|  +  (K + 4) 2^-23 (|A| |W|^T + |bias| + |res|)  +  2^-25
    one rounding to 11 significand bits (16-bit output only); worst-case fp32 accumulation of K products and the epilogue terms
    (2^-23, not 2^-24: a truncating accumulator inside the MFMA is not called a bug); subnormal outputs"""
    tol = (K + 4) * 2.0 ** -23 * absacc + 2.0 ** -25
    if out16:
        tol = tol + 2.0 ** -11 * ref.abs()
    if extra is not None:
        tol = tol + extra
    return tol


def _within(got, ref, tol, what, also_close=True):
    g = got.to(f64)
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    err = (g - ref).abs()
    bad = err > tol
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} outside the derived bound; worst ratio {(err / tol).max().item():.3g}; "
                             f"first {i}: got {g[i].item():.8g} ref {ref[i].item():.8g} tol {tol[i].item():.3g}")
    if also_close:
        _close_f16(got, ref, what=what)
    return (err / tol).max().item()


def test_f16_random_shapes_auto_heuristics(device):
    """the 36 + 14 seeded shapes of test_gemm_and_conv_random_shapes_auto_heuristics through the AUTO tile / split-K choice with IEEE-half
    operands: derived bound, and the same bits from launch to launch"""
    from seervideoldm_amd import ops
    from seervideoldm_amd.weights import pack_conv3x3
    rng = torch.Generator().manual_seed(1234)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=rng))
    for it in range(36):
        M = [ri(1, 300), ri(300, 2000), ri(2000, 9000)][it % 3]
        N = 4 * ri(1, 40) if it % 4 else 128 * ri(5, 12)
        K = 64 * [ri(1, 6), ri(6, 40), ri(40, 100)][(it // 3) % 3]
        a = _rand((M, K), device, 10 + it).to(f16)
        w = _rand((N, K), device, 50 + it, K ** -0.5).to(f16)
        bias = _rand((N,), device, 90 + it) if it % 2 else None
        res = _rand((M, N), device, 130 + it).to(f16) if it % 3 == 0 else None
        out = ops.gemm(a, w, bias=bias, residual=res)
        ref = a.to(f64) @ w.to(f64).t() + (bias.to(f64) if bias is not None else 0) + (res.to(f64) if res is not None else 0)
        absacc = a.to(f64).abs() @ w.to(f64).abs().t() + (bias.to(f64).abs() if bias is not None else 0) + (res.to(f64).abs() if res is not None else 0)
        _within(out, ref, _bound(ref, absacc, K), f"auto gemm {M}x{N}x{K}")
        assert torch.equal(out, ops.gemm(a, w, bias=bias, residual=res)), f"gemm {M}x{N}x{K} not deterministic"
    for it in range(14):
        n_img, H, W = ri(1, 12), 2 * ri(1, 12), 2 * ri(1, 12)
        Ci, Co = 64 * ri(1, 10), [4 * ri(2, 40), 128 * ri(5, 10)][it % 2]
        stride, up = (2, False) if it % 5 == 0 else ((1, True) if it % 5 == 1 else (1, False))
        x = _rand((n_img, Ci, H, W), device, 200 + it).to(f16)
        w = _rand((Co, Ci, 3, 3), device, 240 + it, (9 * Ci) ** -0.5).to(f16)
        bias = _rand((Co,), device, 280 + it)
        x_cl = x.permute(0, 2, 3, 1).reshape(-1, Ci).contiguous()
        out = ops.conv3x3(x_cl, pack_conv3x3(w), n_img, H, W, stride=stride, upsample=up, bias=bias)
        xin = Fn.interpolate(x.to(f64), scale_factor=2.0, mode="nearest") if up else x.to(f64)
        ref = Fn.conv2d(xin, w.to(f64), bias.to(f64), stride=stride, padding=1).permute(0, 2, 3, 1).reshape(-1, Co)
        absacc = Fn.conv2d(xin.abs(), w.to(f64).abs(), bias.to(f64).abs(), stride=stride, padding=1).permute(0, 2, 3, 1).reshape(-1, Co)
        _within(out, ref, _bound(ref, absacc, 9 * Ci), f"auto conv n{n_img} {H}x{W} {Ci}->{Co} s{stride} up{up}")
        assert torch.equal(out, ops.conv3x3(x_cl, pack_conv3x3(w), n_img, H, W, stride=stride, upsample=up, bias=bias))


@pytest.mark.parametrize("tile", [0, 21, 19])
@pytest.mark.parametrize("M,C", [(384, 1280), (1536, 320), (2049, 640)])
def test_f16_geglu(device, M, C, tile):
    """value * gelu(gate) in the epilogue (tile kernel, 256 x 256 tile, weight-stationary kernel).  The bound carries the error of
    both accumulators through the product (|gelu'| <= 1.13) and the GELU's own stated error (3.1e-7 absolute, seer_common.h)."""
    from seervideoldm_amd import ops
    from seervideoldm_amd.weights import interleave_geglu
    N = 8 * C
    a = _rand((M, C), device, 1).to(f16)
    w = _rand((N, C), device, 2, C ** -0.5).to(f16)
    bias = _rand((N,), device, 3, 0.5)
    wi, bi = interleave_geglu(w, bias)
    out = ops.gemm(a, wi, bias=bi, geglu=True, tile=tile)
    assert out.dtype == f16
    h = a.to(f64) @ w.to(f64).t() + bias.to(f64)
    dh = (C + 4) * 2.0 ** -23 * (a.to(f64).abs() @ w.to(f64).abs().t() + bias.to(f64).abs())
    val, gate = h.chunk(2, dim=-1)
    dv, dg = dh.chunk(2, dim=-1)
    gl = 0.5 * gate * (1 + torch.erf(gate / math.sqrt(2)))
    ref = val * gl
    tol = 2.0 ** -11 * ref.abs() + dv * gl.abs() + (val.abs() + dv) * (1.13 * dg + 3.1e-7) + 2.0 ** -23 * ref.abs() + 2.0 ** -25
    _within(out, ref, tol, f"f16 GEGLU {M}x{C} tile {tile}")


@pytest.mark.parametrize("d,T,off", [(40, 640, 128), (80, 192, 64), (160, 48, 16)])
def test_f16_rotary_epilogue_and_col_scale(device, d, T, off):
    """q|k|v projection with the rotary fused into the epilogue at a position offset, the q columns scaled; reference: the float64
    rotation by the table the kernel reads.  Two accumulators meet in every rotated column: their bounds add, and the rotation and
    the scale are three more fp32 roundings."""
    from seervideoldm_amd import ops
    B, Hh, rd = 2, 8, 32
    C = Hh * d
    x = _rand((B * T, C), device, 1).to(f16)
    w = _rand((3 * C, C), device, 2, C ** -0.5).to(f16)
    freqs = (1.0 / (10000 ** (torch.arange(0, rd, 2).float() / rd))).to(device)
    cs = ops.rotary_table(freqs, T + off)
    sc = ops.qk_prescale(d)
    out = ops.gemm(x, w, rotary=(cs, T, off, d, rd, 2 * C), col_scale=(sc, C))
    acc = x.to(f64) @ w.to(f64).t()
    ab = x.to(f64).abs() @ w.to(f64).abs().t()
    pos = (torch.arange(B * T, device=device) % T) + off
    c, s = cs[pos, :, 0].to(f64)[:, None], cs[pos, :, 1].to(f64)[:, None]
    t, tb = acc[:, :2 * C].reshape(B * T, 2 * Hh, d).clone(), ab[:, :2 * C].reshape(B * T, 2 * Hh, d).clone()
    x0, x1, b0, b1 = t[..., 0:rd:2].clone(), t[..., 1:rd:2].clone(), tb[..., 0:rd:2].clone(), tb[..., 1:rd:2].clone()
    t[..., 0:rd:2], t[..., 1:rd:2] = x0 * c - x1 * s, x1 * c + x0 * s
    tb[..., 0:rd:2], tb[..., 1:rd:2] = b0 * c.abs() + b1 * s.abs(), b1 * c.abs() + b0 * s.abs()
    ref = torch.cat([t.reshape(B * T, 2 * C), acc[:, 2 * C:]], 1)
    absacc = torch.cat([tb.reshape(B * T, 2 * C), ab[:, 2 * C:]], 1)
    scv = torch.ones(3 * C, device=device, dtype=f64)
    scv[:C] = float(torch.tensor(sc, dtype=torch.float32))
    ref, absacc = ref * scv, absacc * scv
    _within(out, ref, _bound(ref, absacc, C + 3), f"f16 rotary d{d}")


def test_f16_col_scale_split_k_dual_source_rowvec(device):
    from seervideoldm_amd import ops
    for M, N, K, cols, splits in ((512, 960, 320, 320, 1), (384, 1280, 2560, 1280, 4), (200, 384, 128, 128, 1)):
        a = _rand((M, K), device, 61).to(f16)
        w = (_rand((N, K), device, 62) * K ** -0.5).to(f16)
        out = ops.gemm(a, w, col_scale=(0.228, cols), splits=splits)
        scv = torch.ones(N, device=device, dtype=f64)
        scv[:cols] = float(torch.tensor(0.228, dtype=torch.float32))
        ref = a.to(f64) @ w.to(f64).t() * scv
        absacc = a.to(f64).abs() @ w.to(f64).abs().t() * scv
        _within(out, ref, _bound(ref, absacc, K + 1), f"f16 col_scale {M}x{N}x{K} s{splits}")
    M, K1, K2, N = 768, 640, 320, 320
    a1, a2 = _rand((M, K1), device, 1).to(f16), _rand((M, K2), device, 2).to(f16)
    w = _rand((N, K1 + K2), device, 3, 0.03).to(f16)
    bias, rv = _rand((N,), device, 4), _rand((2, N), device, 5)
    for tile in (0, 19, 20):
        out = ops.gemm(a1, w, a2=a2, bias=bias, rowvec=rv, rows_per_batch=M // 2, tile=tile)
        A = torch.cat([a1, a2], 1).to(f64)
        ref = A @ w.to(f64).t() + bias.to(f64) + rv.to(f64).repeat_interleave(M // 2, 0)
        absacc = A.abs() @ w.to(f64).abs().t() + bias.to(f64).abs() + rv.to(f64).abs().repeat_interleave(M // 2, 0)
        _within(out, ref, _bound(ref, absacc, K1 + K2), f"f16 dual source + row vector, tile {tile}")


def test_f16_conv3x3_epilogue(device):
    from seervideoldm_amd import ops
    from seervideoldm_amd.weights import pack_conv3x3
    B, Fr, H, W, Ci, Co = 2, 3, 8, 8, 64, 128
    n_img = B * Fr
    x = _rand((n_img, Ci, H, W), device, 1).to(f16)
    w = _rand((Co, Ci, 3, 3), device, 2, 0.04).to(f16)
    bias, temb = _rand((Co,), device, 3), _rand((B, Co), device, 4)
    res = _rand((n_img * H * W, Co), device, 5).to(f16)
    x_cl = x.permute(0, 2, 3, 1).reshape(-1, Ci).contiguous()
    out = ops.conv3x3(x_cl, pack_conv3x3(w), n_img, H, W, bias=bias, rowvec=temb, rows_per_batch=Fr * H * W, residual=res)
    rvt = temb.to(f64).repeat_interleave(Fr, 0)[:, :, None, None]
    ref = (Fn.conv2d(x.to(f64), w.to(f64), bias.to(f64), padding=1) + rvt).permute(0, 2, 3, 1).reshape(-1, Co) + res.to(f64)
    absacc = (Fn.conv2d(x.to(f64).abs(), w.to(f64).abs(), bias.to(f64).abs(), padding=1) + rvt.abs()).permute(0, 2, 3, 1).reshape(-1, Co) \
        + res.to(f64).abs()
    _within(out, ref, _bound(ref, absacc, 9 * Ci), "f16 conv epilogue")


@pytest.mark.parametrize("M,B,strided", [(960, 2, False), (6144, 2, False), (12288, 1, True),
                                         (1000, 1, False),      # a ragged last tile (40 rows): no column sums at all
                                         (2048, 2, False)])     # 1024 rows per batch element: tile 10 straddles the two, no per-tile sums
def test_f16_ff_fused_c320_without_the_prologue(device, M, B, strided):
    """seer_ff_fused_c320 on IEEE-half storage WITHOUT the to_out prologue (the form the engine runs wherever the attention output is
    already projected): the structure of test_ff_fused_c320 with every rounding of its formula (a) to float16 and its column-sum
    assertions unchanged (fixed-point sums, the per-tile form and the GroupNorm statistics from it, the cases that leave none).
    Measured rel-L2 values: profiles/f16_matrix.md."""
    from seervideoldm_amd import ops
    from seervideoldm_amd.weights import geglu_row_order
    C, inner = 320, 1280
    ld = C + 64 if strided else C
    hbuf, xbuf = _rand((M, ld), device, 1).to(f16), _rand((M, ld), device, 2).to(f16)
    h, x = hbuf[:, :C], xbuf[:, :C]
    gamma, beta = 1.0 + 0.2 * _rand((C,), device, 3), 0.1 * _rand((C,), device, 4)
    w1 = _rand((2 * inner, C), device, 5, C ** -0.5).to(f16)
    b1 = 0.2 * _rand((2 * inner,), device, 6)
    wcat = _rand((C, C + inner), device, 7, (C + inner) ** -0.5).to(f16)
    bcat = 0.2 * _rand((C,), device, 8)
    order = geglu_row_order(inner, device)
    w1p, b1p = w1[order].contiguous(), b1[order].contiguous()
    w1f, wcf = ops.ff_fused_pack(w1p, wcat)
    arena = ops.FxArena(device, 1 << 16)
    arena.reset()
    y = ops.ff_fused(h, x, gamma, beta, w1f, b1p, wcf, bcat, colsum_batch=(B, arena))
    assert y is not None and y.shape == (M, C) and y.dtype == f16
    hn = Fn.layer_norm(h.to(f64), (C,), gamma.to(f64), beta.to(f64), 1e-5).to(f16).to(f64)
    pre = hn @ w1.to(f64).t() + b1.to(f64)
    gt = pre[:, inner:]
    g = (pre[:, :inner] * (0.5 * gt * (1 + torch.erf(gt / math.sqrt(2))))).to(f16).to(f64)
    ref = x.to(f64) + torch.cat([h.to(f64), g], 1) @ wcat.to(f64).t() + bcat.to(f64)
    _close_f16(y, ref, what="f16 ff_fused vs formula")
    rel = ((y.to(f64) - ref).norm() / ref.norm()).item()
    n = ops.layernorm(h.contiguous(), gamma, beta)
    gg = ops.gemm(n, w1p, bias=b1p, geglu=True)
    y3 = ops.gemm(h.contiguous(), wcat, a2=gg, bias=bcat, residual=x.contiguous())
    rel3 = ((y.to(f64) - y3.to(f64)).norm() / y3.to(f64).norm()).item()
    print(f"ff_fused f16 M={M} strided={strided}: rel-L2 vs formula {rel:.3e}, vs three launches {rel3:.3e}")
    assert rel < 4e-3 and rel3 < 4e-3, (rel, rel3)
    cs = y.colsums
    if (M // B) % 16:
        assert cs is None
        return
    assert cs is not None
    tot = cs.totals()
    yb = y.to(f64).reshape(B, M // B, C)
    assert torch.allclose(tot[:, :, 0], yb.sum(1), rtol=0, atol=2e-2)
    assert torch.allclose(tot[:, :, 1], (yb * yb).sum(1), rtol=1e-5, atol=2e-2)
    # the per-tile form of the same sums (where no tile straddles two batch elements; else the launch leaves none)
    yt = ops.ff_fused(h, x, gamma, beta, w1f, b1p, wcf, bcat, colsum_batch=B)
    assert torch.equal(yt, y)
    if (M // B) % 96 == 0:
        assert isinstance(yt.colsums, ops.ColSums) and yt.colsums.tiles == M // 96
        tt = yt.colsums.buf.double().reshape(B, M // B // 96, C, 2).sum(1)
        assert torch.allclose(tt[:, :, 0], yb.sum(1), rtol=0, atol=2e-2) and torch.allclose(tt[:, :, 1], (yb * yb).sum(1), rtol=1e-5, atol=2e-2)
        stats = torch.empty((B, 32, 2), device=device)
        ops.groupnorm_stats_from_colsums(yt.colsums, None, B, 32, stats)
        want = torch.stack([yb.reshape(B, M // B, 32, 10).sum((1, 3)), (yb * yb).reshape(B, M // B, 32, 10).sum((1, 3))], -1)
        assert torch.allclose(stats.double(), want, rtol=1e-4, atol=1e-1)
    else:
        assert yt.colsums is None
    # in place on the residual stream
    x2 = x.contiguous().clone()
    assert torch.equal(ops.ff_fused(h, x2, gamma, beta, w1f, b1p, wcf, bcat, out=x2), y)


@pytest.mark.parametrize("B,rows,C1,C2,silu", [(2, 200, 1280, 640, True), (2, 192, 640, 320, False), (2, 768, 320, 320, True)])
def test_f16_groupnorm_two_sources(device, B, rows, C1, C2, silu):
    from seervideoldm_amd import ops
    x1 = (_rand((B * rows, C1), device, 1) * 2 + 0.5).to(f16)
    x2 = (_rand((B * rows, C2), device, 2) - 1.0).to(f16)
    Ct = C1 + C2
    gamma, beta = _rand((Ct,), device, 3) + 1.0, _rand((Ct,), device, 4)
    stats = torch.zeros((B, 32, 2), device=device, dtype=torch.float32)
    ops.groupnorm_stats(x1, x2, B, 32, stats)
    y = ops.groupnorm_apply(x1, x2, B, 32, stats, rows * (Ct // 32), 1e-5, gamma, beta, silu)
    xr = torch.cat([x1, x2], 1).to(f64).reshape(B, rows, Ct).permute(0, 2, 1)
    ref = Fn.group_norm(xr, 32, gamma.to(f64), beta.to(f64), eps=1e-5)
    if silu:
        ref = Fn.silu(ref)
    _close_f16(y, ref.permute(0, 2, 1).reshape(B * rows, Ct), what="f16 groupnorm, two sources")


@pytest.mark.parametrize("C1,C2,rows", [(320, 0, 1536), (640, 320, 768), (1280, 1280, 256), (512, 512, 512)])
def test_f16_groupnorm_apply_from_colsums(device, C1, C2, rows):
    from seervideoldm_amd import ops
    B, G = 2, 32
    M = B * rows

    def produce(C, seed):
        a = _rand((M, 320), device, seed).to(f16)
        w = _rand((C, 320), device, seed + 1, 320 ** -0.5).to(f16)
        y = ops.gemm(a, w, bias=_rand((C,), device, seed + 2), colsum_batch=B)
        assert y.colsums is not None
        return y
    x1 = produce(C1, 1)
    x2 = produce(C2, 11) if C2 else None
    C = C1 + C2
    gamma, beta = _rand((C,), device, 21) + 1.0, _rand((C,), device, 22)
    count = rows * (C // G)
    got = ops.groupnorm_apply_from_colsums(x1, x2, x1.colsums, x2.colsums if C2 else None, B, G, count, 1e-5, gamma, beta, True)
    assert got is not None and got.dtype == f16
    xc = x1.to(f64) if x2 is None else torch.cat([x1.to(f64), x2.to(f64)], 1)
    ref = Fn.silu(Fn.group_norm(xc.reshape(B, rows, C).permute(0, 2, 1), G, gamma.to(f64), beta.to(f64), 1e-5)).permute(0, 2, 1).reshape(M, C)
    _close_f16(got, ref, what=f"f16 fused groupnorm C {C1}+{C2}")
    again = ops.groupnorm_apply_from_colsums(x1, x2, x1.colsums, x2.colsums if C2 else None, B, G, count, 1e-5, gamma, beta, True)
    assert torch.equal(got, again)


@pytest.mark.parametrize("C,rows,B", [(320, 3072, 2), (640, 768, 1), (1280, 192, 2), (72, 100, 3)])
def test_f16_groupnorm_stats_fx_is_exact_and_shard_invariant(device, C, rows, B):
    from seervideoldm_amd import ops
    x = (_rand((B * rows, C), device, 5) * 3 + 0.7).to(f16)
    fx = ops.groupnorm_stats_fx(x, B)
    v = x.float().reshape(B, rows, C)
    ref = torch.stack([torch.round(v * 2.0 ** 20).to(torch.int64).sum(1), torch.round(v * v * 2.0 ** 20).to(torch.int64).sum(1)], 1)
    assert torch.equal(fx.buf[0], ref)
    assert torch.equal(ops.groupnorm_stats_fx(x, B).buf, fx.buf)
    cut = (rows * 2 // 3) // 4 * 4 or rows // 2
    xs = x.reshape(B, rows, C)
    a, b = xs[:, :cut].reshape(-1, C).contiguous(), xs[:, cut:].reshape(-1, C).contiguous()
    fa, fb = ops.groupnorm_stats_fx(a, B), ops.groupnorm_stats_fx(b, B)
    assert torch.equal(fa.buf + fb.buf, fx.buf)
    if C % 32 == 0 and C >= 320:
        G = 32
        gamma, beta = _rand((C,), device, 21) + 1.0, _rand((C,), device, 22)
        count = rows * (C // G)
        y_full = ops.groupnorm_apply_fx(x, None, fx, None, B, G, count, 1e-5, gamma, beta, True)
        assert y_full is not None
        tot = ops.ColSumsFx(fa.buf + fb.buf, C)
        y_a = ops.groupnorm_apply_fx(a, None, tot, None, B, G, count, 1e-5, gamma, beta, True)
        y_b = ops.groupnorm_apply_fx(b, None, tot, None, B, G, count, 1e-5, gamma, beta, True)
        got = torch.cat([y_a.reshape(B, cut, C), y_b.reshape(B, rows - cut, C)], 1).reshape(-1, C)
        assert torch.equal(got, y_full)
        refy = Fn.silu(Fn.group_norm(v.to(f64).permute(0, 2, 1), G, gamma.to(f64), beta.to(f64), 1e-5)).permute(0, 2, 1).reshape(-1, C)
        _close_f16(y_full, refy, what=f"f16 groupnorm from exact sums C {C}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("log2s", [-8, 0, 8])
def test_statistics_paths_over_magnitudes(device, dt, log2s):
    """the statistics that quantise (column sums at 2^-20, row sums at 2^-24) with activations scaled by 2^-8, 1 and 2^8:
    GEMM -> colsum_fx -> groupnorm_apply_fx and GEMM -> rowstat -> LayerNorm folded into the consumer, against float64 group_norm /
    layer_norm of the STORED producer output, with the bound of the unscaled twin (test_groupnorm_apply_fx: 1e-2 bf16;
    test_gemm_f16_splitk_and_statistics: 3e-3 fp16; test_layernorm_folded_into_gemm: 2e-2 bf16; test_layernorm_f16_and_fold: 6e-3)."""
    from seervideoldm_amd import ops
    s = 2.0 ** log2s
    B, rows, C, G = 2, 768, 640, 32
    M = B * rows
    arena = ops.FxArena(device, 1 << 18)
    a = _rand((M, 320), device, 1).to(dt)
    w = (_rand((C, 320), device, 2, 320 ** -0.5) * s).to(dt)
    y = ops.gemm(a, w, bias=_rand((C,), device, 3) * 3 * s, colsum_batch=(B, arena))
    assert isinstance(y.colsums, ops.ColSumsFx)
    gamma, beta = _rand((C,), device, 21) + 1.0, _rand((C,), device, 22)
    eps = 1e-5 * s * s                  # the same normalised problem at every scale
    got = ops.groupnorm_apply_fx(y, None, y.colsums, None, B, G, rows * (C // G), eps, gamma, beta, True)
    assert got is not None
    ref = Fn.silu(Fn.group_norm(y.to(f64).reshape(B, rows, C).permute(0, 2, 1), G, gamma.to(f64), beta.to(f64), eps)).permute(0, 2, 1).reshape(M, C)
    tol = 3e-3 if dt == f16 else 1e-2
    err = (got.to(f64) - ref).abs()
    print(f"groupnorm_apply_fx {dt} scale 2^{log2s}: max err {err.max().item():.3e}, worst err / tol {(err / (tol + tol * ref.abs())).max().item():.3f}")
    assert torch.isfinite(got.float()).all() and bool((err <= tol + tol * ref.abs()).all()), err.max().item()
    # rows -> folded LayerNorm
    Cl, N = 640, 1920
    wp = (_rand((Cl, Cl), device, 5, Cl ** -0.5) * s).to(dt)
    h = ops.gemm(_rand((M, Cl), device, 4).to(dt), wp, bias=_rand((Cl,), device, 6) * s, rowstat=True)
    assert h.rowstats is not None
    wl, bl = _rand((N, Cl), device, 7, Cl ** -0.5), _rand((N,), device, 8)
    g2, b2 = _rand((Cl,), device, 9) * 0.3 + 1.0, _rand((Cl,), device, 10) * 0.2
    wf, wsum, bf = ops.fold_layernorm(wl, g2, b2, bl, dtype=dt)
    got = ops.gemm(h, wf, bias=bf, ln=(h.rowstats, wsum, eps))
    assert got is not None
    ref = Fn.layer_norm(h.to(f64), (Cl,), g2.to(f64), b2.to(f64), eps) @ wl.to(f64).t() + bl.to(f64)
    tol = 6e-3 if dt == f16 else 2e-2
    err = (got.to(f64) - ref).abs()
    print(f"folded LayerNorm {dt} scale 2^{log2s}: max err {err.max().item():.3e}, worst err / tol {(err / (tol + tol * ref.abs())).max().item():.3f}")
    assert torch.isfinite(got.float()).all() and bool((err <= tol + tol * ref.abs()).all()), err.max().item()


# =========================================================================================== 3. fp16 attention
def _attn_ref64(q, k, v, B, Sq, Sk, Hh, d, causal=False, off=0, prescaled=False, scale=None):
    """float64 softmax attention on the stored q, k, v ([B*S, Hh*d] token-major) -> [B*Sq, Hh*d]"""
    qq = q.to(f64).reshape(B, Sq, Hh, d).permute(0, 2, 1, 3)
    kk = k.to(f64).reshape(B, Sk, Hh, d).permute(0, 2, 1, 3)
    vv = v.to(f64).reshape(B, Sk, Hh, d).permute(0, 2, 1, 3)
    s = qq @ kk.transpose(-1, -2) * (math.log(2.0) if prescaled else (scale if scale is not None else d ** -0.5))
    if causal:
        i = torch.arange(Sq, device=q.device)[:, None] + off
        s = s.masked_fill(~(torch.arange(Sk, device=q.device)[None, :] <= i), float("-inf"))
    return (s.softmax(-1) @ vv).permute(0, 2, 1, 3).reshape(B * Sq, Hh * d)


def _attn_close(out, ref, what, dt=f16):
    if dt == f16:
        _close_f16(out, ref, rtol=3e-3, atol=2e-3, what=what)          # test_attention_f16's
    else:
        from tests.test_gpu_kernels import _close
        _close(out, ref, rtol=2e-2, atol=1e-2, what=what)               # test_attention's


def test_f16_attention_random_shapes(device):
    """test_attention_random_shapes with IEEE-half operands: ragged Sq / Sk, causal with a query offset, d in 40 / 80 / 96 / 160"""
    from seervideoldm_amd import ops
    rng = torch.Generator().manual_seed(77)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=rng))
    for it in range(16):
        d = (40, 80, 96, 160)[it % 4]
        B, Hh = ri(1, 3), ri(1, 8)
        Sq, Sk = ri(1, 500), ri(1, 500)
        causal = it % 3 == 0
        off = 0
        if causal:
            Sk = max(Sk, Sq)
            off = ri(0, Sk - Sq)
        C = Hh * d
        q, k, v = (_rand((B * S, C), device, sd + it).to(f16) for S, sd in ((Sq, 300), (Sk, 340), (Sk, 380)))
        out = torch.zeros((B * Sq, C), device=device, dtype=f16)
        ops.attention(q, k, v, out, batch=B, heads=Hh, head_dim=d, Sq=Sq, Sk=Sk, causal=causal, causal_offset=off)
        _attn_close(out, _attn_ref64(q, k, v, B, Sq, Sk, Hh, d, causal, off), f"f16 attn d{d} B{B} H{Hh} {Sq}x{Sk} causal={causal}+{off}")


@pytest.mark.parametrize("variant", [0, 1, 5])
@pytest.mark.parametrize("Sk", [255, 256, 257, 383, 384])
def test_f16_attention_d40_routing_boundary(device, variant, Sk):
    """d = 40 with IEEE-half operands switches kernels at 256 keys (the generic kernel below, the d = 40 kernel's tracked form from
    there up); variant 1 / 5 force either on both sides; ragged Sq, last key tile partly filled"""
    from seervideoldm_amd import ops
    B, Hh, d, Sq = 2, 8, 40, 203
    C = Hh * d
    q, k, v = _rand((B * Sq, C), device, 1).to(f16), _rand((B * Sk, C), device, 2).to(f16), _rand((B * Sk, C), device, 3).to(f16)
    out = torch.zeros((B * Sq, C), device=device, dtype=f16)
    ops.attention(q, k, v, out, batch=B, heads=Hh, head_dim=d, Sq=Sq, Sk=Sk, variant=variant)
    _attn_close(out, _attn_ref64(q, k, v, B, Sq, Sk, Hh, d), f"f16 d40 variant {variant} Sk {Sk}")
    oc = torch.zeros_like(out)
    ops.attention(q, k, v, oc, batch=B, heads=Hh, head_dim=d, Sq=Sq, Sk=Sk, causal=True, causal_offset=Sk - Sq, variant=variant)
    _attn_close(oc, _attn_ref64(q, k, v, B, Sq, Sk, Hh, d, True, Sk - Sq), f"f16 d40 variant {variant} Sk {Sk} causal")


def test_f16_attention_refusals(device):
    """what the half form does not have is refused with SeerHipError, and nothing is written: variants 2 / 3 / 7, and lse (training)
    with every variant it otherwise takes -- the generic kernel, which has an lse store, at d = 40 (variant 1), 80 and 160 included"""
    from seervideoldm_amd import ops
    from seervideoldm_amd._lib import SeerHipError
    B, Hh, d, S = 2, 8, 40, 256
    C = Hh * d
    q, k, v = (_rand((B * S, C), device, sd).to(f16) for sd in (1, 2, 3))
    out = torch.full((B * S, C), 7.0, device=device, dtype=f16)
    for variant in (2, 3, 7):
        with pytest.raises(SeerHipError):
            ops.attention(q, k, v, out, batch=B, heads=Hh, head_dim=d, Sq=S, Sk=S, variant=variant)
    lse = torch.full((B * Hh, S), 7.0, device=device, dtype=torch.float32)
    for variant in (0, 1, 5):
        with pytest.raises(SeerHipError):
            ops.attention(q, k, v, out, batch=B, heads=Hh, head_dim=d, Sq=S, Sk=S, lse=lse, variant=variant)
    with pytest.raises(SeerHipError):          # below 256 keys AUTO is the generic kernel
        ops.attention(q, k[:B * 77], v[:B * 77], out, batch=B, heads=Hh, head_dim=d, Sq=S, Sk=77, lse=lse)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (lse == 7.0).all(), "a refused call must not write"
    for d2 in (80, 160):
        C2 = Hh * d2
        q2, k2, v2 = (_rand((B * S, C2), device, sd).to(f16) for sd in (4, 5, 6))
        out2 = torch.full((B * S, C2), 7.0, device=device, dtype=f16)
        with pytest.raises(SeerHipError):
            ops.attention(q2, k2, v2, out2, batch=B, heads=Hh, head_dim=d2, Sq=S, Sk=S, lse=lse)
        torch.cuda.synchronize()
        assert (out2 == 7.0).all() and (lse == 7.0).all(), f"a refused call must not write (d = {d2})"


@pytest.mark.parametrize("d,S,window", [(40, 1024, None), (40, 300, None), (40, 200, None), (80, 256, None), (40, 3 * 64, (8, 3, 16, 16)),
                                        (40, 5 * 64, (8, 5, 16, 16))])
def test_f16_attention_head_major_operands(device, d, S, window):
    from seervideoldm_amd import ops
    B, Hh = 2, 8
    C = Hh * d
    tok = S if window is None else window[1] * window[2] * window[3]
    qkv = _rand((B * tok, 3 * C), device, 17).to(f16)
    kw = dict(batch=B, heads=Hh, head_dim=d, Sq=S, Sk=S, causal=window is not None, window=window)
    want = torch.empty((B * tok, C), device=device, dtype=f16)
    ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], want, **kw)
    hm = [t.reshape(B, tok, Hh, d).permute(0, 2, 1, 3).contiguous().reshape(B * Hh * tok, d) for t in qkv.split(C, dim=1)]
    got = torch.empty_like(want)
    ops.attention(qkv[:, :C], hm[1], hm[2], got, kv_head_major=True, **kw)
    assert torch.equal(got, want)
    got2 = torch.empty_like(want)
    ops.attention(hm[0], hm[1], hm[2], got2, q_head_major=True, kv_head_major=True, **kw)
    assert torch.equal(got2, want)
    if window is None:
        _attn_close(want, _attn_ref64(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], B, S, S, Hh, d), f"f16 fused-qkv layout d{d} S{S}")


@pytest.mark.parametrize("d,Fr,H,W,ws,f0,f1", [(40, 6, 16, 16, 4, 2, 4), (80, 5, 8, 8, 4, 3, 5), (160, 4, 4, 4, 0, 1, 3), (40, 4, 32, 32, 8, 0, 2),
                                               (40, 6, 8, 8, 0, 2, 5)])
def test_f16_frame_shard_attention(device, d, Fr, H, W, ws, f0, f1):
    """a frame shard (queries of frames [f0, f1), K|V of all frames, causal_offset = position of frame f0) reproduces the unsharded
    rows bit for bit with IEEE-half operands too"""
    from seervideoldm_amd import ops
    B, Hh = 2, 8
    C = Hh * d
    T = Fr * H * W
    qkv = _rand((B * T, 3 * C), device, 21).to(f16)
    full = torch.zeros((B * T, C), device=device, dtype=f16)
    kw = dict(batch=B, heads=Hh, head_dim=d, causal=True)
    Fl = f1 - f0
    ql = qkv.reshape(B, Fr, H * W, 3 * C)[:, f0:f1, :, :C].reshape(B * Fl * H * W, C).contiguous()
    out = torch.zeros((B * Fl * H * W, C), device=device, dtype=f16)
    if ws:
        ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], full, Sq=Fr * ws * ws, Sk=Fr * ws * ws, window=(ws, Fr, H, W), **kw)
        ops.attention(ql, qkv[:, C:2 * C], qkv[:, 2 * C:], out, Sq=Fl * ws * ws, Sk=Fr * ws * ws, window=(ws, Fr, H, W), Fq=Fl,
                      causal_offset=f0 * ws * ws, **kw)
    else:
        ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], full, Sq=T, Sk=T, **kw)
        ops.attention(ql, qkv[:, C:2 * C], qkv[:, 2 * C:], out, Sq=Fl * H * W, Sk=T, causal_offset=f0 * H * W, **kw)
        _attn_close(full, _attn_ref64(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], B, T, T, Hh, d, True), f"f16 causal d{d} T{T}")
    assert torch.equal(out, full.reshape(B, Fr, H * W, C)[:, f0:f1].reshape(B * Fl * H * W, C))


def test_f16_attention_strided_sequences(device):
    from seervideoldm_amd import ops
    Fr, L, Hh, d = 12, 77, 8, 96
    C = Hh * d
    qkv = _rand((Fr * L, 3 * C), device, 5).to(f16)
    out = torch.zeros((Fr * L, C), device=device, dtype=f16)
    ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], out, batch=L, heads=Hh, head_dim=d, Sq=Fr, Sk=Fr,
                  causal=True, seq_stride_rows=L, batch_stride_rows=1)
    q, k, v = [t.reshape(Fr, L, C).permute(1, 0, 2).reshape(L * Fr, C) for t in qkv.split(C, dim=1)]     # sequence-major copies
    ref = _attn_ref64(q, k, v, L, Fr, Fr, Hh, d, True).reshape(L, Fr, C).permute(1, 0, 2).reshape(Fr * L, C)
    _attn_close(out, ref, "f16 strided-sequence attention")


@pytest.mark.parametrize("d,S", [(40, 1024), (40, 77), (40, 300), (80, 256), (160, 64)])
def test_f16_attention_q_prescaled(device, d, S):
    from seervideoldm_amd import ops
    B, Hh = 3, 8
    C = Hh * d
    q = (_rand((B * S, C), device, 41) * ops.qk_prescale(d)).to(f16)
    k, v = _rand((B * S, C), device, 42).to(f16), _rand((B * S, C), device, 43).to(f16)
    out = torch.zeros((B * S, C), device=device, dtype=f16)
    ops.attention(q, k, v, out, batch=B, heads=Hh, head_dim=d, Sq=S, Sk=S, q_prescaled=True)
    _attn_close(out, _attn_ref64(q, k, v, B, S, S, Hh, d, prescaled=True), f"f16 prescaled q d{d}")


@pytest.mark.parametrize("d,Fr,H,W,ws", [(80, 12, 16, 16, 4), (160, 3, 8, 8, 4)])
def test_f16_window_attention(device, d, Fr, H, W, ws):
    from seervideoldm_amd import ops
    B, Hh = 2, 8
    C = Hh * d
    T = Fr * H * W
    S = Fr * ws * ws
    qkv = _rand((B * T, 3 * C), device, 11).to(f16)
    out = torch.zeros((B * T, C), device=device, dtype=f16)
    ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], out, batch=B, heads=Hh, head_dim=d, Sq=S, Sk=S, causal=True, window=(ws, Fr, H, W))

    def part(t):   # [B*T, C] -> [nW*B * S, C]: window_partition, sequences one after the other
        t = t.reshape(B, Fr, H // ws, ws, W // ws, ws, C).permute(2, 4, 0, 1, 3, 5, 6)
        return t.reshape(-1, C)
    nW = (H // ws) * (W // ws)
    o = _attn_ref64(part(qkv[:, :C]), part(qkv[:, C:2 * C]), part(qkv[:, 2 * C:]), nW * B, S, S, Hh, d, True)
    o = o.reshape(H // ws, W // ws, B, Fr, ws, ws, C).permute(2, 3, 0, 4, 1, 5, 6).reshape(B * T, C)
    _attn_close(out, o, f"f16 window attention d{d}")


def _rel_l2(got, ref):
    return ((got.to(f64) - ref).norm() / ref.norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize("d,variant", [(40, 0), (40, 1), (40, 5), (80, 0), (96, 0), (160, 0)])
@pytest.mark.parametrize("amp", [3.0, 6.0])
def test_f16_attention_sharp_softmax(device, d, variant, amp):
    """scores hundreds of log2 units apart: the softmax reference of the d = 40 tracked form re-bases again and again (the branch no
    N(0, 1) input reaches), the generic kernel rescales its accumulators.  Finite, and at most 2x the rel-L2 of an emulation that is
    float64 except where the kernel rounds: q * scale * log2(e) to fp16 in the d = 40 kernel, P = exp2(s - max) to fp16, the output
    to fp16.  (2x: the kernel's P is relative to a reference up to 2^14 above or a half ulp off the true maximum, which moves which
    terms go subnormal.)  Measured values per case: profiles/f16_matrix.md."""
    from seervideoldm_amd import ops
    B, S, Hh = 2, 1024, 8
    C = Hh * d
    q, k, v = (_rand((B * S, C), device, sd, amp).to(f16) for sd in (31, 32, 33))
    out = torch.zeros((B * S, C), device=device, dtype=f16)
    ops.attention(q, k, v, out, batch=B, heads=Hh, head_dim=d, Sq=S, Sk=S, variant=variant)
    assert torch.isfinite(out.float()).all(), "non-finite attention output"
    ref = _attn_ref64(q, k, v, B, S, S, Hh, d)
    split = lambda t: t.to(f64).reshape(B, S, Hh, d).permute(0, 2, 1, 3)
    qq, kk, vv = split(q), split(k), split(v)
    if d == 40 and variant != 1:
        qs = (q.float() * float(torch.tensor(d ** -0.5 * ops.LOG2E, dtype=torch.float32))).to(f16)
        s2 = split(qs) @ kk.transpose(-1, -2)
    else:
        s2 = qq @ kk.transpose(-1, -2) * (d ** -0.5 * ops.LOG2E)
    p = torch.exp2(s2 - s2.amax(-1, keepdim=True)).to(f16).to(f64)
    emu = ((p @ vv) / p.sum(-1, keepdim=True)).to(f16).permute(0, 2, 1, 3).reshape(B * S, C)
    e_emu, e_ker = _rel_l2(emu, ref), _rel_l2(out, ref)
    print(f"sharp softmax f16 d{d} variant {variant} amp {amp}: emulation rel-L2 {e_emu:.3e}, kernel {e_ker:.3e}")
    assert e_ker <= 2 * e_emu, (e_ker, e_emu)


def _staircase(device, dt, d, Sq, Sk, edges, step, seed=0, descending=False):
    """q (prescaled: the kernels exponentiate the raw dot products, so every level is EXACT in the storage type), k, v whose scores
    step by `step` log2 units at the key positions `edges`; v shrinks by the same factor per level (and by the level's key count),
    so every level carries a comparable share of the output.  Returns q, k, v [S, Hh*d] for B = 1 and the level of every key."""
    Hh = 2
    g = torch.Generator().manual_seed(1000 + seed)
    level = torch.zeros(Sk, dtype=torch.int64)
    for e in edges:
        level[e:] += 1
    nl = len(edges) + 1
    q = torch.randint(0, 2, (Sq, Hh, d), generator=g).double() * 2.0 ** -5 - 2.0 ** -6          # +-2^-6: score noise of ~0.05 log2 units
    q[:, :, 0] = 2.0
    k = torch.randn((Sk, Hh, d), generator=g).double() * 0.5 * (40.0 / d) ** 0.5
    lv = level.double() if not descending else -level.double()
    k[:, :, 0] = (lv * (step / 2.0))[:, None]
    u = (torch.rand((Sk, Hh, d), generator=g).double() * 0.25 + 0.75)
    if descending:
        v = u * torch.where(torch.rand((Sk, Hh, d), generator=g) < 0.5, -1.0, 1.0).double()
    else:
        counts = torch.bincount(level, minlength=nl).double()
        if dt == f16:
            # the half range holds 2^-14 .. 65504: the top level sits just above the bottom of the normal range, the levels below
            # rise by 2^step per level (capped at the top of the range) and by the ratio of the key counts
            vtop = 2.0 ** -13
            mag = torch.stack([torch.clamp(vtop * 2.0 ** (step * (nl - 1 - l)) * counts[nl - 1] / counts[l], max=60000.0) for l in range(nl)])
        else:
            mag = torch.stack([2.0 ** (step * (nl - 1 - l)) * counts[nl - 1] / counts[l] * 2.0 ** -30 for l in range(nl)])
        v = u * mag[level][:, None, None]
    to = lambda t: t.reshape(t.shape[0], Hh * d).to(device).to(dt)
    return to(q), to(k), to(v), level.to(device), Hh


_STAIR_F16 = [((45, 96), 140), ((64, 128), 200), ((128, 283), 420), ((33, 250), 290), ((150, 320), 470)]
_STAIR_BF16 = [((45, 96, 200), 300), ((64, 128, 256), 384), ((128, 283, 384), 520)]


def _run_staircase(device, dt, d, variant, edges, Sk, step):
    from seervideoldm_amd import ops
    Sq = 170
    q, k, v, level, Hh = _staircase(device, dt, d, Sq, Sk, edges, step)
    C = Hh * d
    # preconditions on the reference alone: everything representable (normal, finite), every level >= 10 % of the output norm
    vmin = 2.0 ** -14 if dt == f16 else 2.0 ** -126
    assert torch.isfinite(v.float()).all() and (v.float().abs() >= vmin).all() and torch.isfinite(k.float()).all()
    s = (q.to(f64).reshape(Sq, Hh, d).permute(1, 0, 2) @ k.to(f64).reshape(Sk, Hh, d).permute(1, 2, 0))      # [Hh, Sq, Sk], log2 units
    for i, e in enumerate(edges):
        jump = s[:, :, level == i + 1].amin(-1) - s[:, :, level <= i].amax(-1)
        assert (jump > (14.0 if dt == f16 else 16.0)).all(), "every step must exceed the re-base threshold for every query"
    p = torch.softmax(s * math.log(2.0), -1)
    vv = v.to(f64).reshape(Sk, Hh, d).permute(1, 0, 2)
    ref = (p @ vv).permute(1, 0, 2).reshape(Sq, C)
    for l in range(len(edges) + 1):
        part = ((p * (level == l)) @ vv).permute(1, 0, 2).reshape(Sq, C)
        assert part.norm() >= 0.1 * ref.norm(), f"level {l} carries {float(part.norm() / ref.norm()):.3f} of the output"
    out = torch.zeros((Sq, C), device=device, dtype=dt)
    ops.attention(q, k, v, out, batch=1, heads=Hh, head_dim=d, Sq=Sq, Sk=Sk, q_prescaled=True, variant=variant)
    # the test_attention_f16 / test_attention tolerances, relative to the output scale
    scale = ref.abs().max()
    rtol, atol = (3e-3, 2e-3) if dt == f16 else (2e-2, 1e-2)
    g = out.to(f64)
    assert torch.isfinite(g).all()
    err = (g - ref).abs()
    bad = err > rtol * ref.abs() + atol * scale
    assert not bool(bad.any()), (f"staircase {dt} d{d} variant {variant} edges {edges}: {int(bad.sum())}/{bad.numel()} outside tolerance, "
                                 f"max err {float(err.max() / scale):.3g} of the output scale")


@pytest.mark.parametrize("d,variant", [(40, 0), (40, 5), (40, 1), (80, 1), (160, 1)])
@pytest.mark.parametrize("edges,Sk", _STAIR_F16)
def test_f16_attention_rebase_staircase(device, d, variant, edges, Sk):
    """scores that step up by 15 log2 units (just over A40_THR_F16 = 14) inside a 32-key block, at a block edge and at a 128-key tile
    edge, with V scaled down from level to level (by the step's factor between the two upper levels; the bottom level is clamped at
    6e4, the top of the half range, where the construction wants 2^17, and the >= 10 % share of every level is asserted on the
    reference instead): every level carries a comparable share of the output, so a rescale of the
    accumulators that is skipped, doubled or applied to the wrong query block changes the result by O(1 / levels), not by 2^-15.
    The half range holds two such steps with V normal (2^-14 .. 6e4).  d = 40: the tracked form (variants 0 and 5) and the generic
    kernel (1); the generic kernel at d = 80 / 160 (variant 1 = 0 there)."""
    _run_staircase(device, f16, d, variant if d == 40 else 0, edges, Sk, 15.0)


@pytest.mark.parametrize("variant", [1, 2, 3, 5])
@pytest.mark.parametrize("edges,Sk", _STAIR_BF16)
def test_bf16_attention_rebase_staircase(device, variant, edges, Sk):
    """the bf16 twin: steps of 17 log2 units (A40_THR = 16), three of them; the generic kernel, both fast-path shapes (whose fixed
    reference overflows here and falls back to the tracked form) and the tracked form"""
    _run_staircase(device, bf16, 40, variant, edges, Sk, 17.0)


@pytest.mark.parametrize("dt,d,variant", [(f16, 40, 0), (f16, 40, 5), (f16, 40, 1), (f16, 80, 0), (f16, 160, 0), (bf16, 40, 1), (bf16, 40, 2),
                                          (bf16, 40, 3), (bf16, 40, 5)])
def test_attention_descending_staircase(device, dt, d, variant):
    """the descending twin: the first block holds the highest scores, later keys fall by 20 log2 units per step -- 2^-20 is a
    subnormal P in half, 2^-40 and 2^-60 are below 2^-24 and must vanish without a NaN"""
    from seervideoldm_amd import ops
    Sq, Sk = 170, 420
    q, k, v, level, Hh = _staircase(device, dt, d, Sq, Sk, (45, 128, 283), 20.0, seed=1, descending=True)
    C = Hh * d
    s = (q.to(f64).reshape(Sq, Hh, d).permute(1, 0, 2) @ k.to(f64).reshape(Sk, Hh, d).permute(1, 2, 0))
    ref = (torch.softmax(s * math.log(2.0), -1) @ v.to(f64).reshape(Sk, Hh, d).permute(1, 0, 2)).permute(1, 0, 2).reshape(Sq, C)
    out = torch.zeros((Sq, C), device=device, dtype=dt)
    ops.attention(q, k, v, out, batch=1, heads=Hh, head_dim=d, Sq=Sq, Sk=Sk, q_prescaled=True, variant=variant)
    _attn_close(out, ref, f"descending staircase {dt} d{d} variant {variant}", dt)


@pytest.mark.parametrize("variant", [0, 5, 1])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_f16_attention_scores_in_the_thousands(device, variant, sign):
    """scores of +-(4096 .. 7232) log2 units in steps of 64, offset by 2.75: the softmax reference of the tracked form is a half value
    with an ulp of 4 there (f16_ceil's adjustment step, positive and negative), every key block re-bases, and the keys that tie at
    the maximum share the output.  Far beyond what a model produces, inside what the kernel documents (|score| < 60000)."""
    from seervideoldm_amd import ops
    Sq, Sk, Hh, d = 100, 300, 2, 40
    g = torch.Generator().manual_seed(5)
    q = torch.randint(0, 2, (Sq, Hh, d), generator=g).double() * 2.0 ** -5 - 2.0 ** -6
    q[:, :, 0], q[:, :, 1] = 64.0, 1.0
    k = torch.randn((Sk, Hh, d), generator=g).double() * 0.5
    k[:, :, 0] = (sign * (64 + torch.arange(Sk) % 50).double())[:, None]
    k[:, :, 1] = 2.75
    v = torch.randn((Sk, Hh, d), generator=g).double()
    q, k, v = (t.reshape(t.shape[0], Hh * d).to(device).to(f16) for t in (q, k, v))
    out = torch.zeros((Sq, Hh * d), device=device, dtype=f16)
    ops.attention(q, k, v, out, batch=1, heads=Hh, head_dim=d, Sq=Sq, Sk=Sk, q_prescaled=True, variant=variant)
    _attn_close(out, _attn_ref64(q, k, v, 1, Sq, Sk, Hh, d, prescaled=True), f"f16 scores in the thousands, variant {variant}, sign {sign}")
