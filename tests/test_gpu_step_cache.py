"""seer_cache_push / seer_cache_forecast and SeerUNet.enable_step_cache on a real MI355X (tests/step_cache_ref.py; the CPU half is
tests/test_step_cache_host.py): the two kernels bit for bit -- moved bits, an exact construction, the fixed fp32 order, skipped slots,
refusals that write nothing -- at sizes around the 8-element vector and across blocks, inside NaN sentinels; the engine's storing and
cached walks, bit for bit where the definition says so and against the oracle's blocks elsewhere; and the captured steps of the three
samplers against their launch-by-launch runs.

WITHOUT THE FEATURE every test here fails at its first ops.cache_*, enable_step_cache or cache_phase=."""
import pytest
import torch

from seervideoldm_amd import DDIMSampler, DPMSolverSampler, PLMSSampler, SeerUNet, _lib, ops, synth
from tests import sampler_graph_cases as sg
from tests import step_cache_ref as R
from tests.test_gpu_unet import CFG_MINI, REL_L2, REL_L2_F16, REL_MAX

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
SIZES = [1, 7, 8, 9, 320 * 7, 2 ** 15 + 3]       # below, at and past one vector; a tail; several blocks with a tail
PAD = 64                                          # sentinel elements (128 bytes: what sits between them stays 16-byte aligned)
L = CFG_MINI["layers_per_block"]
BRANCHES = list(range(L + 1))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, seed):
    return torch.randn(shape, generator=_gen(seed))


def _bits(t):
    return t.view(torch.int16)


class _Ring:
    """three slots of n elements, a padded stride apart, inside a NaN-filled buffer: PAD sentinels in front, behind, and (with the
    rounding of n to the vector) between the slots"""

    def __init__(self, n, dtype, device):
        self.n, self.stride = n, (n + 7) // 8 * 8 + PAD
        self.buf = torch.full((PAD + 3 * self.stride + PAD,), float("nan"), dtype=dtype, device=device)
        self.ring = self.buf[PAD:PAD + 3 * self.stride].view(3, self.stride)

    def fill(self, slots):
        for k, s in enumerate(slots):
            self.ring[k, :self.n] = s.to(self.buf.device)
        return self

    def expected(self, before, slots):
        """the whole buffer's bits when the slots hold `slots` and everything else is what it was in `before`"""
        want = before.clone()
        for k, s in enumerate(slots):
            want[PAD + k * self.stride:PAD + k * self.stride + self.n] = s.to(want.device)
        return _bits(want)


class _Out:
    def __init__(self, n, dtype, device):
        self.n = n
        self.buf = torch.full((PAD + n + PAD,), float("nan"), dtype=dtype, device=device)
        self.out = self.buf[PAD:PAD + n]

    def guards_untouched(self):
        return bool(torch.isnan(self.buf[:PAD]).all() and torch.isnan(self.buf[PAD + self.n:]).all())


def _patterns(n, dtype, seed):
    """n random 16-bit patterns of the storage type, NaN and infinity patterns among them"""
    b = torch.randint(-2 ** 15, 2 ** 15, (n,), generator=_gen(seed), dtype=torch.int32).to(torch.int16)
    inf = 0x7F80 if dtype == torch.bfloat16 else 0x7C00
    special = torch.tensor([inf, inf - 0x10000, inf + 1, 0x7FFF, -1, 0, -0x8000, 1], dtype=torch.int32).to(torch.int16)
    b[:min(n, 8)] = special[torch.randperm(8, generator=_gen(seed + 1))][:min(n, 8)]
    return b.view(dtype)


def _w(vals, device):
    return torch.tensor(vals, dtype=torch.float32, device=device)


# ---- 1. push --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("n", SIZES)
def test_push_moves_bits_in_order(device, dtype, n):
    r = _Ring(n, dtype, device)
    before = r.buf.clone()
    xs = [_patterns(n, dtype, 10 * n + k).to(device) for k in range(3)]
    keep = [x.clone() for x in xs]
    for k, x in enumerate(xs):
        ops.cache_push(x, r.ring)
        torch.cuda.synchronize()
        newest_first = [keep[j].cpu() for j in range(k, -1, -1)]
        assert torch.equal(_bits(r.buf), r.expected(before, newest_first)), (n, k)      # slots in order; every sentinel untouched
    for x, k in zip(xs, keep):
        assert torch.equal(_bits(x), _bits(k))                                          # x is only read
    # a fourth push drops the oldest
    x4 = _patterns(n, dtype, 10 * n + 7).to(device)
    ops.cache_push(x4, r.ring)
    torch.cuda.synchronize()
    assert torch.equal(_bits(r.buf), r.expected(before, [x4.cpu(), keep[2].cpu(), keep[1].cpu()]))
    # ... which is what the restatement the CPU tests run on says
    assert torch.equal(_bits(r.ring.cpu())[:, :n], _bits(R.push_ref(torch.stack([keep[2], keep[1], keep[0]]).cpu(), x4.cpu())))


# ---- 2. forecast ----------------------------------------------------------------------------------------------------------------------
def _forecast(r, w, dtype, device):
    o = _Out(r.n, dtype, device)
    before = r.buf.clone()
    got = ops.cache_forecast(r.ring, _w(w, device), o.out)
    torch.cuda.synchronize()
    assert got is o.out and o.guards_untouched()
    assert torch.equal(_bits(r.buf), _bits(before))               # the ring is only read
    return o.out.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("n", SIZES)
def test_forecast_exact_construction(device, dtype, n):
    """dyadic weights (interval 2 and 4: u = 1/2, 1/4, 3/4) on slots that hold 32 * small integers, the integers bounded so that every
    result is an integer below 256: representable in either storage type, and every fp32 operation on the way is exact -- the kernel
    has one right answer"""
    for interval, d in ((2, 1), (4, 1), (4, 3)):
        for order in (0, 1, 2):
            w = R.weights(d, interval, order, 3)
            assert all(float(v * 32).is_integer() for v in w), w
            bound = int(255 // sum(abs(v) * 32 for v in w))
            assert bound >= 1
            slots = [(32 * torch.randint(-bound, bound + 1, (n,), generator=_gen(100 * n + 10 * interval + order + k))).to(dtype)
                     for k in range(3)]
            want = R.forecast64(slots, w)
            assert torch.equal(want.to(dtype).double(), want), "the construction is not representable"
            got = _forecast(_Ring(n, dtype, device).fill(slots), w, dtype, device)
            assert torch.equal(got.double(), want), (n, interval, d, order)
            assert torch.equal(_bits(got), _bits(R.forecast_ref(slots, w, dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("n", SIZES)
def test_forecast_follows_the_fixed_fp32_order(device, dtype, n):
    """random slots with magnitudes in [2^-4, 2^4], the weights of intervals 3 and 5: bit for bit the emulation of w0 * f0, fmaf, fmaf,
    one rounding (each float64 operation of the emulation is exact in that range: a 24-bit weight times an 11-bit value next to a
    24-bit sum, within 50 binary places of each other)"""
    for interval in (3, 5):
        for d in range(1, interval):
            for order in (1, 2):
                g = _gen(1000 * n + 100 * interval + 10 * d + order)
                slots = [(torch.exp2(torch.rand((n,), generator=g) * 8 - 4) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)).to(dtype)
                         for _ in range(3)]
                w = R.weights(d, interval, order, 3)
                got = _forecast(_Ring(n, dtype, device).fill(slots), w, dtype, device)
                assert torch.equal(_bits(got), _bits(R.forecast_ref(slots, w, dtype))), (n, interval, d, order)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("n", SIZES)
def test_zero_weights_skip_their_slot(device, dtype, n):
    f0 = _randn((n,), n).to(dtype)
    f2 = _randn((n,), n + 1).to(dtype)
    nan = torch.full((n,), float("nan"), dtype=dtype)
    # reuse: slots 1 and 2 may hold anything, slot 0 comes back bit for bit
    got = _forecast(_Ring(n, dtype, device).fill([f0, nan, nan]), (1.0, 0.0, 0.0), dtype, device)
    assert torch.equal(_bits(got), _bits(f0))
    # a zero w1 with a NaN slot 1 stays finite, and is the two-slot value
    got = _forecast(_Ring(n, dtype, device).fill([f0, nan, f2]), (1.5, 0.0, -0.5), dtype, device)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(_bits(got), _bits(R.forecast_ref([f0, nan, f2], (1.5, 0.0, -0.5), dtype)))
    # ... and the same slot with any weight is seen
    got = _forecast(_Ring(n, dtype, device).fill([f0, nan, f2]), (1.5, 2.0 ** -20, -0.5), dtype, device)
    assert torch.isnan(got.float()).all()


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(device):
    lib = _lib.load()
    n = 1000
    r = _Ring(n, torch.bfloat16, device).fill([_randn((n,), k).to(torch.bfloat16) for k in range(3)])
    x = _randn((n + 64,), 5).to(torch.bfloat16).to(device)
    o = _Out(n + 64, torch.bfloat16, device)
    w = _w((1.5, -0.5, 0.0), device)
    X, O_, RING, W, BF = x.data_ptr(), o.out.data_ptr(), r.ring.data_ptr(), w.data_ptr(), _lib.SEER_DT_BF16
    span = (2 * r.stride + n) * 2                      # bytes of the ring
    stream = torch.cuda.current_stream().cuda_stream
    keep = (r.buf.clone(), x.clone(), o.buf.clone())

    def push(x=X, ring=RING, n=n, stride=r.stride, dt=BF):
        return lib.seer_cache_push(x, ring, n, stride, dt, stream)

    def forecast(out=O_, ring=RING, n=n, stride=r.stride, w=W, dt=BF):
        return lib.seer_cache_forecast(ring, n, stride, w, out, dt, stream)
    for kw in (dict(ring=None), dict(n=0), dict(n=-8), dict(stride=n - 1), dict(stride=n - 8), dict(dt=2), dict(dt=-1),
               dict(ring=RING + 4), dict(stride=r.stride + 4), dict(stride=r.stride + 1)):
        assert push(**kw) == -22 and forecast(**kw) == -22, kw
    # NULL, off 16 bytes, and every way of lying across the ring
    for name, base, call in (("x", X, push), ("out", O_, forecast)):
        for ptr in (None, base + 2, base + 8, RING, RING + 16, RING + span - 16, RING - 1984):
            assert call(**{name: ptr}) == -22, (name, None if ptr is None else ptr - RING)
    assert forecast(w=None) == -22 and forecast(w=W + 2) == -22
    torch.cuda.synchronize()
    assert torch.equal(_bits(r.buf), _bits(keep[0])) and torch.equal(_bits(x), _bits(keep[1])) and torch.equal(_bits(o.buf), _bits(keep[2]))
    # the binding refuses a ring of another type before the library sees it
    with pytest.raises(TypeError):
        ops.cache_push(x[:n].to(torch.float16), r.ring)


# ---- 4. the engine --------------------------------------------------------------------------------------------------------------------
CASES = [(1, 2, 16, 0), (2, 3, 8, 1)]


def _mini(device, **kw):
    m = SeerUNet(**CFG_MINI, **kw)
    m.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI)), strict=True)
    return m.to(device).eval()


@pytest.fixture(scope="module")
def mini(device):
    return _mini(device)


@pytest.fixture(scope="module")
def mini_inv(device):
    return _mini(device, layout_invariant=True)


def _inputs(case, seed):
    B, Fr, H, _ = case
    return _randn((B, 4, Fr, H, H), seed), _randn((B, Fr, 77, 256), 2), torch.tensor([501 - 20 * (seed - 1)] * B)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=["b1f2h16", "b2f3h8c1"])
@pytest.mark.parametrize("inv", [False, True], ids=["default", "layout_invariant"])
def test_phase0_is_the_plain_evaluation_bit_for_bit(device, mini, mini_inv, dtype, case, inv):
    m = mini_inv if inv else mini
    x, ctx, t = (v.to(device) for v in _inputs(case, 1))
    m.compute_dtype = dtype
    try:
        plain = m(x, t, ctx, cond_frame=case[3])
        for b in BRANCHES:
            m.enable_step_cache(3, b, 1)
            assert torch.equal(m(x, t, ctx, cond_frame=case[3]), plain)
            assert torch.equal(m(x, t, ctx, cond_frame=case[3], cache_phase=0), plain), b
            assert m._engine.inv == inv and m._engine.dt == dtype and m._engine.cache_valid == 1
    finally:
        m.disable_step_cache()
        m.compute_dtype = None


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=["b1f2h16", "b2f3h8c1"])
def test_cached_at_the_same_inputs_is_the_full_output_under_layout_invariant(device, mini_inv, dtype, case):
    """order 0 hands back the kept feature's bits and that mode's GroupNorms sum the stored values exactly, with or without their
    producer's sums; at u = 1/2 the weights 1.5 and -0.5 of two equal features are exact on 16-bit data"""
    m = mini_inv
    x, ctx, t = (v.to(device) for v in _inputs(case, 1))
    m.compute_dtype = dtype
    try:
        for b in BRANCHES:
            m.enable_step_cache(3, b, 0)
            full = m(x, t, ctx, cond_frame=case[3], cache_phase=0)
            assert torch.equal(m(x, t, ctx, cond_frame=case[3], cache_phase=1), full), b
            m.enable_step_cache(2, b, 1)
            m(x, t, ctx, cond_frame=case[3], cache_phase=0)
            assert m._engine.cache_valid == 2
            assert m._step_cache.weights(1, 2) == (1.5, -0.5, 0.0)
            assert torch.equal(m(x, t, ctx, cond_frame=case[3], cache_phase=1), full), b
    finally:
        m.disable_step_cache()
        m.compute_dtype = None


_walks = {}


def _oracle_walks(case, branch):
    """the oracle's walks of a case and branch, once for both storage types: full at A (and at A2), cached at B from A's feature
    (order 0) and from the order-1 forecast of A2's and A's"""
    key = (case, branch)
    if key not in _walks:
        sd = synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI))
        (xa, ctx, ta), (xa2, _, ta2), (xb, _, tb) = _inputs(case, 1), _inputs(case, 3), _inputs(case, 2)
        w = R.weights(1, 3, 1, 2)
        with torch.no_grad():
            _, fa = R.full_walk(sd, CFG_MINI, xa, ta, ctx, case[3], branch)
            _, fa2 = R.full_walk(sd, CFG_MINI, xa2, ta2, ctx, case[3], branch)
            _walks[key] = (R.cached_walk(sd, CFG_MINI, xb, tb, ctx, case[3], branch, fa),
                           R.cached_walk(sd, CFG_MINI, xb, tb, ctx, case[3], branch, w[0] * fa2 + w[1] * fa))
    return _walks[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("branch", BRANCHES)
@pytest.mark.parametrize("case", CASES, ids=["b1f2h16", "b2f3h8c1"])
def test_cached_at_other_inputs_matches_the_oracle_walk(device, mini, dtype, case, branch):
    ref_reuse, ref_linear = _oracle_walks(case, branch)
    m = mini
    (xa, ctx, ta), (xa2, _, ta2), (xb, _, tb) = (tuple(v.to(device) for v in _inputs(case, s)) for s in (1, 3, 2))
    m.compute_dtype = dtype
    try:
        m.enable_step_cache(3, branch, 1)
        m(xa, ta, ctx, cond_frame=case[3], cache_phase=0)
        reuse = m(xb, tb, ctx, cond_frame=case[3], cache_phase=1).float().cpu()          # one valid slot: order 0
        m(xa2, ta2, ctx, cond_frame=case[3], cache_phase=0)
        linear = m(xb, tb, ctx, cond_frame=case[3], cache_phase=1).float().cpu()         # two: the linear forecast
    finally:
        m.disable_step_cache()
        m.compute_dtype = None
    for name, got, ref in (("reuse", reuse, ref_reuse), ("linear", linear, ref_linear)):
        rel = ((got - ref).norm() / ref.norm()).item()
        mx = ((got - ref).abs().max() / ref.abs().max()).item()
        print(f"[step_cache] engine {dtype} {case} branch {branch} {name}: rel_l2 {rel:.4g} rel_max {mx:.4g}")
        assert torch.isfinite(got).all()
        assert rel <= (REL_L2 if dtype == torch.bfloat16 else REL_L2_F16) and mx <= REL_MAX, (name, rel, mx)
    assert not torch.equal(reuse, linear)


CFG_TWO_WIDTHS = dict(block_out_channels=(320, 640, 640, 640), layers_per_block=1, cross_attention_dim=256, attention_head_dim=8)


def test_cut_feature_at_the_deepest_branch_has_level_1_width(device):
    """branch = layers_per_block cuts behind the last upsampler, whose output is as wide as level 1 (640 channels here, as at full
    size; CFG_MINI's levels are all 320 wide and cannot tell): the storing walk is the plain one, the cached one the oracle's"""
    sd = synth.synth_state_dict(synth.unet_param_shapes(CFG_TWO_WIDTHS))
    m = SeerUNet(**CFG_TWO_WIDTHS)
    m.load_state_dict(sd, strict=True)
    m = m.to(device).eval()
    xa, xb = _randn((1, 4, 2, 8, 8), 1), _randn((1, 4, 2, 8, 8), 2)
    ctx, t = _randn((1, 2, 77, 256), 3), torch.tensor([501])
    m.enable_step_cache(3, 1, 1)
    plain = m(xa.to(device), t.to(device), ctx.to(device))
    assert torch.equal(m(xa.to(device), t.to(device), ctx.to(device), cache_phase=0), plain)
    got = m(xb.to(device), t.to(device), ctx.to(device), cache_phase=1).float().cpu()
    assert m._engine._cache_cur["fc"].shape == (2 * 8 * 8, 640)
    with torch.no_grad():
        _, feat = R.full_walk(sd, CFG_TWO_WIDTHS, xa, t, ctx, 0, 1)
        ref = R.cached_walk(sd, CFG_TWO_WIDTHS, xb, t, ctx, 0, 1, feat)
    rel = ((got - ref).norm() / ref.norm()).item()
    mx = ((got - ref).abs().max() / ref.abs().max()).item()
    print(f"[step_cache] two widths, branch 1: rel_l2 {rel:.4g} rel_max {mx:.4g}")
    assert rel <= REL_L2 and mx <= REL_MAX, (rel, mx)


# ---- 5. captured steps ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fresh(device):
    """a second model: its rings never see what the model under test ran"""
    return _mini(device)


@pytest.fixture(scope="module")
def never(device):
    """a third one, on which step caching is never enabled"""
    return _mini(device)


def _sample(cls, m, device, graph, seed=1, smp=None):
    b, f1, Fp, H = 1, 1, 2, 16
    x0 = (_randn((b, 4, f1, H, H), seed) * 0.9).to(device)
    c = _randn((b, f1 + Fp, 77, 256), seed + 1).to(device)
    uc = _randn((b, 1, 77, 256), seed + 2).expand(-1, f1 + Fp, -1, -1).contiguous().to(device)
    noise = _randn((b, 4, Fp, H, H), seed + 3).to(device)
    m.use_graph = graph
    try:
        lat, _ = (smp or cls(device)).sample(unet=m, S=6, conditioning=c, batch_size=b, shape=(4, Fp, H, H), x0_emb=x0, verbose=False,
                                             unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=0.0, x_T=noise,
                                             is_3d=True)
    finally:
        m.use_graph = False
    return lat.clone()


@pytest.mark.parametrize("cls,kind", [(DDIMSampler, "step"), (PLMSSampler, "plms"), (DPMSolverSampler, "dpm")], ids=["ddim", "plms", "dpm"])
def test_captured_steps_equal_their_launch_by_launch_runs(device, mini, fresh, never, cls, kind):
    m = mini
    if m._engine is not None:
        m._engine._graphs.clear()
    off = _sample(cls, never, device, False)
    try:
        m.enable_step_cache(3, 1, 1)
        want = _sample(cls, m, device, False)
        with sg.recorded_keys() as keys:
            smp = cls(device)
            got = _sample(cls, m, device, True, smp=smp)
            assert torch.equal(got, want) and not torch.equal(got, off)
            assert len(keys) == 1 and keys[0][0] == kind and keys[0][-2:] == ("cache", 1), keys
            # a second sample on the same sampler, other inputs: it starts from a full step, the first sample's ring is not read
            fresh.enable_step_cache(3, 1, 1)
            assert torch.equal(_sample(cls, m, device, True, seed=50, smp=smp), _sample(cls, fresh, device, False, seed=50))
            # interval and order are policy: the same two graphs
            for interval, order in ((2, 1), (3, 0)):
                m.enable_step_cache(interval, 1, order)
                fresh.enable_step_cache(interval, 1, order)
                moved = _sample(cls, m, device, True, smp=smp)
                assert torch.equal(moved, _sample(cls, fresh, device, False)) and not torch.equal(moved, got), (interval, order)
            assert len(keys) == 1, keys
            # off: the key of before this feature, the bits of a model that never had it
            m.disable_step_cache()
            assert torch.equal(_sample(cls, m, device, True, smp=smp), off)
            assert len(keys) == 2 and keys[1] == keys[0][:-2] and "cache" not in keys[1], keys
    finally:
        m.disable_step_cache()
        fresh.disable_step_cache()
