"""Guidance rescale on a real MI355X: the two launches of seer_cfg_rescale / seer_slot_cfg_rescale -- exact on integers, the multiplier
within 1 ulp of float64 on normals and both rows the one fp32 product, the same bits for a clip wherever it sits in a batch or among
slots, nothing written for an idle or a phi = 0 slot, every refusal --; then the mini UNet: the captured step against the launches for
DDIM, PLMS, DPM-Solver++ and a v-model, and a rescaled clip in a queue against its solo run under the layout-invariant mode."""
import pytest
import torch

from seervideoldm_amd import DDIMSampler, DPMSolverSampler, PLMSSampler, SeerUNet, SlotSampler, _lib, ops, synth
from tests import norm_edge_ref as N
from tests import rescale_ref as R
from tests.test_gpu_dpm import _fence_intact, _fenced, _mini_inputs

pytestmark = pytest.mark.gpu

NAN = float("nan")
TILE = ops.RESCALE_TILE
# (b, C, Ft, cond_f, HW): n = 60 (less than one wave), 1280, 1 and 3600 (four tiles, a ragged last one) elements per clip; then exactly
# one tile, and one tile plus one element
CASES = list(N.CFG_CASES) + [(2, 1, 2, 1, TILE), (2, 1, 2, 1, TILE + 1)]
CASE_IDS = lambda c: "x".join(map(str, c))


def _ints(shape, seed, device):
    return torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(seed)).float().to(device)


def _randn(shape, seed, device):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(device)


def _bits(a, b):
    """bit for bit, NaN included"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _fenced64(n, device, pad=8):
    whole = torch.full((n + 2 * pad,), NAN, device=device, dtype=torch.float64)
    return whole[pad:pad + n], whole


def _ws_doubles(clips, case):
    _, C, Ft, cond_f, HW = case
    n = C * (Ft - cond_f) * HW
    return clips * ((n + TILE - 1) // TILE) * 4


def _run(eps, case, scale, phi):
    """seer_cfg_rescale on a fenced copy of eps with a fenced workspace and multiplier vector -> (rows, mult)"""
    b, _, _, cond_f, _ = case
    out, whole = _fenced(eps.shape, eps.device)
    out.copy_(eps)
    ws, ws_whole = _fenced64(_ws_doubles(b, case), eps.device)
    mult, mult_whole = _fenced((b,), eps.device)
    assert ops.cfg_rescale(out, scale=scale, rescale=phi, cond_f=cond_f, ws=ws, mult=mult) is out
    assert _fence_intact(whole) and _fence_intact(mult_whole) and bool(torch.isnan(ws_whole[:8]).all() and torch.isnan(ws_whole[-8:]).all())
    assert not torch.isnan(ws).any()                     # every partial of every clip was stored
    return out, mult


# ---- 1. exact on integers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_rescale_is_exact_on_integers(device, case):
    """ec integers in -8..8, the conditioning frames NaN.  Four families whose sums, ratio, root and products are exact:
      (a) eu = 0, scale 2, phi 0.5: g = 2 ec, sqrt(q_c / q_g) = 1/2, m = 0.75, out = 1.5 ec
      (b) eu = 0, scale 4, phi 1: m = 0.25, out = ec
      (c) eu = ec - 3, scale 8, phi 0.75: g = ec + 21, q_g = q_c (the mean term cancels exactly), m = 1
      (d) eu = ec, scale 7.5, phi 0.7: g = ec, m = 1
    a clip whose ec is constant (n = 1 always) has q_g = 0: m = 1 and out = g.  mult and both rows bit for bit; the conditioning frames
    keep their NaN bit for bit; fences intact."""
    b, C, Ft, cond_f, HW = case
    ec = _ints((b, C, Ft, HW, 1), 3, device)
    flat = ec[:, :, cond_f:].reshape(b, -1)
    constant = (flat.max(1).values == flat.min(1).values)
    families = [(torch.zeros_like(ec), 2.0, 0.5, 0.75), (torch.zeros_like(ec), 4.0, 1.0, 0.25), (ec - 3.0, 8.0, 0.75, 1.0),
                (ec.clone(), 7.5, 0.7, 1.0)]
    for eu, scale, phi, m in families:
        eps = torch.cat([eu, ec])
        eps[:, :, :cond_f] = NAN
        out, mult = _run(eps, case, scale, phi)
        want_m = torch.where(constant, torch.ones(b, device=device), torch.full((b,), m, device=device))
        g = eu + scale * (ec - eu)                       # exact in fp32: small integers
        want = want_m.view(-1, 1, 1, 1, 1) * g
        assert _bits(mult, want_m), (scale, phi, mult.tolist())
        assert _bits(out[:b, :, cond_f:], want[:, :, cond_f:]) and _bits(out[b:, :, cond_f:], want[:, :, cond_f:]), (scale, phi)
        assert _bits(out[:, :, :cond_f], eps[:, :, :cond_f])
    if C * (Ft - cond_f) * HW == 1:
        assert bool(constant.all())


# ---- 2. normals against float64 -----------------------------------------------------------------------------------------------------------
def _guided(eps, case, scale):
    """the bits of g from the update kernel itself: pred_x0 of a DDIM step with the row (1, 1, 0, 1) at x = 0 is (0 - 1 g) / 1 = -g"""
    b, C, Ft, cond_f, HW = case
    coef = torch.tensor([[1.0, 1.0, 0.0, 1.0]], device=eps.device)
    x = torch.zeros((b, C, Ft - cond_f, HW, 1), device=eps.device)
    return -ops.cfg_ddim_step(eps, x, coef, 0, cfg=True, scale=scale, cond_f=cond_f)[1]


@pytest.mark.parametrize("shift", [0.0, 0.3])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_multiplier_is_within_one_ulp_of_float64_and_rows_are_one_product(device, case, shift):
    """randn and randn + 0.3, scales 1.5 and 7.5, phi 0.3, 0.7 and 1.  g is read off the update kernel (its own bits), m64 is made of
    those g and the c rows in float64 on the CPU, and |mult - m64| <= 2^-23 m64: the double sums err by at most n 2^-53 relative,
    amplified by n S2 / q <= 2 for data with |mean| <= std -- far below 2^-24 -- and the one rounding to float stays within half an ulp
    of the ulp allowed.  Both rows are float32(mult) * g bit for bit.  At phi = 1 the std of a clip's output is the std of its c row
    within 4 * 2^-24 relative."""
    b, C, Ft, cond_f, HW = case
    eps = torch.cat([_randn((b, C, Ft, HW, 1), 11, device), _randn((b, C, Ft, HW, 1), 12, device) + shift])
    eps[:, :, :cond_f] = NAN
    c = eps[b:, :, cond_f:]
    worst = 0.0
    for scale in (1.5, 7.5):
        g = _guided(eps, case, scale)
        for phi in (0.3, 0.7, 1.0):
            out, mult = _run(eps, case, scale, phi)
            m64 = R.multiplier64(g.cpu(), c.cpu(), phi).reshape(-1)
            err = (mult.double().cpu() - m64).abs() / (2.0 ** -23 * m64)
            worst = max(worst, float(err.max()))
            assert (err <= 1.0).all(), (scale, phi, mult.tolist(), m64.tolist())
            want = mult.view(-1, 1, 1, 1, 1) * g
            assert _bits(out[:b, :, cond_f:], want) and _bits(out[b:, :, cond_f:], want), (scale, phi)
            assert _bits(out[:, :, :cond_f], eps[:, :, :cond_f])
            if phi == 1.0 and c[0].numel() > 1:
                s_out, s_c = out[:b, :, cond_f:].double().cpu().reshape(b, -1).std(1), c.double().cpu().reshape(b, -1).std(1)
                assert ((s_out - s_c).abs() <= 4 * 2.0 ** -24 * s_c).all(), (scale, s_out.tolist(), s_c.tolist())
    print(f"[rescale] {case} shift {shift}: worst |mult - m64| / (2^-23 m64) = {worst:.3f}")


# ---- 3. layout independence -----------------------------------------------------------------------------------------------------------------
def _place(clip_u, clip_c, rows, at, seed, device):
    """[2 rows, ...]: the clip at row `at`, other clips (other data) in the other rows"""
    eu, ec = _randn((rows, *clip_u.shape), seed, device), _randn((rows, *clip_u.shape), seed + 1, device) + 0.3
    eu[at], ec[at] = clip_u, clip_c
    return torch.cat([eu, ec])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_a_clip_has_the_same_bits_in_every_layout(device, case):
    """the tiling follows from n alone: b = 1, rows 0 and 2 of b = 3, slots 0 and 3 of four slots (the other slots running other clips at
    other scales and factors, or idle) give one mult and one pair of rows"""
    _, C, Ft, cond_f, HW = case
    scale, phi = 7.5, 0.7
    clip_u, clip_c = _randn((C, Ft, HW, 1), 21, device), _randn((C, Ft, HW, 1), 22, device) + 0.3
    one = (1, C, Ft, cond_f, HW)
    want, want_m = _run(torch.cat([clip_u[None], clip_c[None]]), one, scale, phi)
    assert _bits(want[0, :, cond_f:], want[1, :, cond_f:])
    for at in (0, 2):
        got, mult = _run(_place(clip_u, clip_c, 3, at, 30 + at, device), (3, C, Ft, cond_f, HW), scale, phi)
        assert _bits(mult[at:at + 1], want_m) and _bits(got[at, :, cond_f:], want[0, :, cond_f:])
        assert _bits(got[3 + at, :, cond_f:], want[0, :, cond_f:])
    nsched = 8
    coef = torch.zeros((4, nsched, 4), device=device)
    for at in (0, 3):
        buf = _place(clip_u, clip_c, 4, at, 40 + at, device)
        scales = torch.tensor([3.0, 1.5, 5.0, 2.0], device=device)
        phis = torch.tensor([0.3, 1.0, 0.0, 0.5], device=device)
        steps = torch.tensor([[9, 2], [9, 0], [9, 5], [9, -1]], dtype=torch.int32, device=device)
        scales[at], phis[at], steps[at, 1] = scale, phi, nsched - 1
        mult = torch.full((4,), NAN, device=device)
        ops.slot_cfg_rescale(buf, scales, phis, coef, steps, cond_f=cond_f, mult=mult)
        assert _bits(mult[at:at + 1], want_m) and _bits(buf[at, :, cond_f:], want[0, :, cond_f:])
        assert _bits(buf[4 + at, :, cond_f:], want[0, :, cond_f:])


# ---- 4. the slot form -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[5]], ids=CASE_IDS)
def test_idle_and_plain_slots_are_left_alone(device, case):
    """four slots: one idle (step -1), one past its table (index == nsched), one at phi = 0 -- their rows, planted with NaN in every
    word, their part of ws and their mult keep their bits -- and one running, which gets the bits of its solo call; then the same with
    two running.  No step word changes."""
    _, C, Ft, cond_f, HW = case
    nsched, slots = 8, 4
    coef = torch.zeros((slots, nsched, 4), device=device)
    per_ws = _ws_doubles(1, case)
    for running in ((1,), (0, 2)):
        eu, ec = _randn((slots, C, Ft, HW, 1), 51, device), _randn((slots, C, Ft, HW, 1), 52, device) + 0.3
        scales = torch.tensor([7.5, 3.0, 1.5, 5.0], device=device)
        phis = torch.tensor([0.7, 1.0, 0.7, 0.3], device=device)
        steps = torch.tensor([[4, 1], [4, 0], [4, nsched - 1], [4, 3]], dtype=torch.int32, device=device)
        quiet = [s for s in range(slots) if s not in running]
        for how, s in zip(("idle", "past", "plain"), quiet):
            if how == "idle":
                steps[s, 1] = -1
            elif how == "past":
                steps[s, 1] = nsched
            else:
                phis[s] = 0.0
            eu[s], ec[s] = NAN, NAN
        eps = torch.cat([eu, ec])
        eps[:, :, :cond_f] = NAN
        out, whole = _fenced(eps.shape, device)
        out.copy_(eps)
        ws, ws_whole = _fenced64(slots * per_ws, device)
        mult, mult_whole = _fenced((slots,), device)
        before = steps.clone()
        ops.slot_cfg_rescale(out, scales, phis, coef, steps, cond_f=cond_f, ws=ws, mult=mult)
        assert _fence_intact(whole) and _fence_intact(mult_whole) and bool(torch.isnan(ws_whole[:8]).all() and torch.isnan(ws_whole[-8:]).all())
        assert torch.equal(steps, before)
        for s in quiet:
            assert _bits(out[s], eps[s]) and _bits(out[slots + s], eps[slots + s])
            assert bool(torch.isnan(ws[s * per_ws:(s + 1) * per_ws]).all()) and bool(torch.isnan(mult[s]))
        for s in running:
            solo, solo_m = _run(torch.cat([eps[s:s + 1], eps[slots + s:slots + s + 1]]), (1, C, Ft, cond_f, HW), float(scales[s]),
                                float(phis[s]))
            assert _bits(out[s], solo[0]) and _bits(out[slots + s], solo[1]) and _bits(mult[s:s + 1], solo_m)
            assert not torch.isnan(ws[s * per_ws:(s + 1) * per_ws]).any()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------
def _refusals(out, ws, mult, words, f32s):
    good = dict(out=out, b=2, C=2, Ft=3, cond_f=1, HW=5, scale=7.5, rescale=0.7, ws=ws, mult=mult)
    for why, kw in [("out NULL", dict(out=None)), ("ws NULL", dict(ws=None)), ("b = 0", dict(b=0)), ("b < 0", dict(b=-1)),
                    ("C = 0", dict(C=0)), ("HW = 0", dict(HW=0)), ("HW < 0", dict(HW=-4)), ("F_total = 0", dict(Ft=0, cond_f=0)),
                    ("cond_f < 0", dict(cond_f=-1)), ("cond_f = F_total", dict(cond_f=3)), ("rescale < 0", dict(rescale=-0.25)),
                    ("rescale > 1", dict(rescale=1.5)), ("rescale NaN", dict(rescale=NAN)), ("rescale inf", dict(rescale=float("inf"))),
                    ("out misaligned", dict(out=out + 2)), ("ws misaligned", dict(ws=ws + 4)), ("mult misaligned", dict(mult=mult + 1)),
                    ("more clips than a grid's second dimension", dict(b=65536)),
                    ("more tiles than a grid's first dimension", dict(C=1 << 20, Ft=(1 << 20) + 1, HW=1 << 10))]:
        yield "seer_cfg_rescale", tuple({**good, **kw}.values()), why
    good = dict(out=out, slots=2, C=2, Ft=3, cond_f=1, HW=5, scale=f32s, rescale=f32s + 16, nsched=4, step=words, ws=ws, mult=mult)
    for why, kw in [("out NULL", dict(out=None)), ("scale NULL", dict(scale=None)), ("rescale NULL", dict(rescale=None)),
                    ("step NULL", dict(step=None)), ("ws NULL", dict(ws=None)), ("slots = 0", dict(slots=0)), ("slots = 5", dict(slots=5)),
                    ("C = 0", dict(C=0)), ("HW = 0", dict(HW=0)), ("F_total = 0", dict(Ft=0, cond_f=0)), ("cond_f < 0", dict(cond_f=-1)),
                    ("cond_f = F_total", dict(cond_f=3)), ("nsched = 0", dict(nsched=0)), ("nsched < 0", dict(nsched=-3)),
                    ("out misaligned", dict(out=out + 1)), ("scale misaligned", dict(scale=f32s + 2)),
                    ("rescale misaligned", dict(rescale=f32s + 3)), ("step misaligned", dict(step=words + 2)),
                    ("ws misaligned", dict(ws=ws + 4)), ("mult misaligned", dict(mult=mult + 2)),
                    ("more tiles than a grid's first dimension", dict(C=1 << 20, Ft=(1 << 20) + 1, HW=1 << 10))]:
        yield "seer_slot_cfg_rescale", tuple({**good, **kw}.values()), why


def test_entry_points_refuse_bad_arguments_and_launch_nothing(device):
    """real, aligned buffers: a refused call returns SEER_EINVAL and leaves every buffer as it was; rescale == 0 is SEER_OK and
    launches nothing either; the workspace query refuses what the calls refuse"""
    lib = _lib.load()
    out, whole = _fenced((4, 2, 3, 5, 1), device)
    ws, ws_whole = _fenced64(64, device)
    mult, mult_whole = _fenced((4,), device)
    words = torch.tensor([[3, 2], [3, 1], [3, 0], [3, 3]], dtype=torch.int32, device=device)
    f32s = torch.full((32,), 0.5, device=device)
    n = 0
    for fn, args, why in _refusals(out.data_ptr(), ws.data_ptr(), mult.data_ptr(), words.data_ptr(), f32s.data_ptr()):
        assert getattr(lib, fn)(*args, None) == -22, (fn, why)
        n += 1
    assert lib.seer_cfg_rescale(out.data_ptr(), 2, 2, 3, 1, 5, 7.5, 0.0, ws.data_ptr(), mult.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert n == 40 and torch.isnan(whole).all() and torch.isnan(ws_whole).all() and torch.isnan(mult_whole).all()
    assert words.tolist() == [[3, 2], [3, 1], [3, 0], [3, 3]] and bool((f32s == 0.5).all())
    assert lib.seer_cfg_rescale_ws_bytes(3, 4, 5, 2, 300) == 3 * 4 * 4 * 8 and lib.seer_cfg_rescale_ws_bytes(1, 1, 2, 1, 1) == 32
    for bad in ((0, 4, 5, 2, 300), (3, 0, 5, 2, 300), (3, 4, 5, 5, 300), (3, 4, 5, -1, 300), (3, 4, 5, 2, 0)):
        assert lib.seer_cfg_rescale_ws_bytes(*bad) == -22
    # the wrappers: a factor outside [0, 1] is a ValueError; a missing workspace is made; phi = 0 returns the tensor untouched
    eps = _randn((4, 2, 3, 5, 1), 1, device)
    with pytest.raises(ValueError, match="guidance_rescale"):
        ops.cfg_rescale(eps.clone(), scale=7.5, rescale=1.5, cond_f=1)
    same = eps.clone()
    assert ops.cfg_rescale(same, scale=7.5, rescale=0.0, cond_f=1) is same and torch.equal(same, eps)
    made = ops.cfg_rescale(eps.clone(), scale=7.5, rescale=0.7, cond_f=1)
    given = ops.cfg_rescale(eps.clone(), scale=7.5, rescale=0.7, cond_f=1, ws=ops.cfg_rescale_workspace(2, 2, 3, 1, 5, device))
    assert torch.equal(made, given) and not torch.equal(made, eps)


# ---- 6. the mini UNet: captured against launch by launch ----------------------------------------------------------------------------------
SAMPLERS = {"ddim": (DDIMSampler, "step", "epsilon"), "plms": (PLMSSampler, "plms", "epsilon"), "dpm": (DPMSolverSampler, "dpm", "epsilon"),
            "ddim-v": (DDIMSampler, "step", "v_prediction")}
_unets = {}


def _unet(device, cfg, **kw):
    """this module's own models (synthetic weights): the graphs these tests capture stay out of the engines other modules' tests count"""
    key = (tuple(sorted(cfg.items())), tuple(sorted(kw.items())))
    if key not in _unets:
        m = SeerUNet(**cfg, **kw)
        m.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(cfg)), strict=True)
        _unets[key] = m.to(device).eval()
    return _unets[key]


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_captured_rescaled_step_equals_the_launch_by_launch_step(device, name):
    """CFG 7.5, phi = 0.7, S = 5: the node is part of the captured step.  Same bits as the launches of a fresh sampler over a whole sample,
    every pred_x0 included; the graph key ends in ("rescale", 0.7), behind "v_prediction" for a v-model; the same sampler at phi = 0
    captures under the key it always had and gives another latent"""
    cls, kind, prediction_type = SAMPLERS[name]
    from tests.test_dist_gpu import CFG_MINI as cfg
    m = _unet(device, cfg)
    b, Fp, H, S = 1, 2, 16, 5
    x0, c, uc, noise = (t.to(device) for t in _mini_inputs(cfg, seed=80))
    ptype = {} if prediction_type == "epsilon" else dict(prediction_type=prediction_type)

    def sample(sampler, graph, **kw):
        m.use_graph = graph
        torch.manual_seed(5)
        preds = []
        lat, _ = sampler.sample(unet=m, S=S, conditioning=c, batch_size=b, shape=(4, Fp, H, H), x0_emb=x0, verbose=False,
                                unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=0.0, x_T=noise, is_3d=True,
                                img_callback=lambda p, i: preds.append(p), **kw)
        return lat, preds, torch.rand(3, device=device)

    def keys():
        return [k for k in m._engine._graphs if isinstance(k, tuple) and k and k[0] == kind
                and (("v_prediction" in k) == (prediction_type != "epsilon"))]
    try:
        want, wp, wr = sample(cls(device, guidance_rescale=0.7, **ptype), False)
        captured = cls(device, **ptype)
        got, gp, gr = sample(captured, True, guidance_rescale=0.7)          # the per-call keyword, against the constructor's
        assert not captured._capture_refused and torch.isfinite(got).all()
        assert torch.equal(got, want) and torch.equal(gr, wr) and len(gp) == len(wp) == S
        assert all(torch.equal(a, b_) for a, b_ in zip(gp, wp))
        mine = keys()
        assert len(mine) == 1 and mine[0][-2:] == ("rescale", 0.7)
        assert (mine[0][-3] == "v_prediction") == (prediction_type != "epsilon")
        plain, _, _ = sample(cls(device, **ptype), True)
        both = keys()
        assert len(both) == 2 and [k for k in both if "rescale" not in k][0] == mine[0][:-2]
        assert not torch.equal(plain, got)
    finally:
        m.use_graph = False


# ---- 7. a queue against solo runs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("method", ["ddim", "dpmpp"])
def test_a_rescaled_clip_in_a_queue_equals_its_solo_run_under_the_invariant_mode(device, method, use_graph):
    """SeerUNet(layout_invariant=True), two slots, three staggered requests: two rescaled at phi = 0.7 (the sampler under test) around a
    plain DDIM neighbour.  A rescaled clip's latent is torch.equal to the solo sampler's sample(guidance_rescale=0.7) of the clip alone;
    the neighbour's to its latent in a queue built without the keyword."""
    from tests.test_gpu_slots import CFG_MINI, F1, FP, HL, _requests
    m = _unet(device, CFG_MINI, layout_invariant=True)
    extra = dict(method="dpmpp") if method == "dpmpp" else {}
    reqs = _requests(device)
    reqs[0].update(guidance_rescale=0.7, **extra)
    reqs[2].update(guidance_rescale=0.7, **extra)
    cls = DPMSolverSampler if method == "dpmpp" else DDIMSampler
    build = lambda **kw: SlotSampler(m, 2, shape=(4, FP, HL, HL), cond_frames=F1, context_shape=(77, CFG_MINI["cross_attention_dim"]),
                                     device=device, model_cond_frame=F1, **(dict(dpm=True) if method == "dpmpp" else {}), **kw)
    m.use_graph = False
    want = {}
    for r in (reqs[0], reqs[2]):
        want[r["tag"]], _ = cls(device).sample(
            m, r["S"], batch_size=1, shape=(4, FP, HL, HL), x0_emb=r["x0_emb"], conditioning=r["c"], verbose=False, cond_frames=F1,
            unconditional_guidance_scale=r["scale"], unconditional_conditioning=r["uc"], eta=0., x_T=r["x_T"], is_3d=True,
            guidance_rescale=0.7)
    m.use_graph = use_graph
    try:
        want[reqs[1]["tag"]] = dict(build().run(iter([reqs[1]])))[reqs[1]["tag"]]
        smp = build(rescale=True)
        got = dict(smp.run(iter(reqs)))
        mine = [k for k, G in m._engine._graphs.items() if isinstance(k, tuple) and k and G.get("owner") is smp]
        assert len(mine) == (1 if use_graph else 0) and all(k[-1] == "rescale" for k in mine)
    finally:
        m.use_graph = False
    for r in reqs:
        w = want[r["tag"]]
        assert torch.isfinite(w).all() and torch.equal(got[r["tag"]], w), (r["tag"], (got[r["tag"]] - w).abs().max().item())
    plain = dict(build().run(iter([{k: v for k, v in reqs[0].items() if k != "guidance_rescale"}])))[reqs[0]["tag"]]
    assert not torch.equal(plain, got[reqs[0]["tag"]])
