"""DDIM inversion on a real MI355X: seer_cfg_ddim_invert_step per element against float64 with a derived bound, its aliasing, NULL
and refusal edges inside NaN sentinels, the DDIM step as its inverse, the device-counter form against the host-index form bit for bit
and past its limit, DDIMSampler.encode as a captured step against the launches, its layout invariance, the round trip on the
analytic Gaussian model, and edit_clips(invert=True).

Measured values: profiles/invert_sampler.md."""
import math

import pytest
import torch

from seervideoldm_amd import (AutoencoderKL, DDIMSampler, FSTextTransformer, SeerUNet, _lib, edit_clips, ops, pipeline, synth)
from seervideoldm_amd.ddim import frames_to_latents
from seervideoldm_amd.vae import ldm_to_diffusers_vae
from tests import invert_ref as R
from tests import norm_edge_ref as N
from tests.test_gpu_train_matrix import _bound
from tests.test_invert_host import refusal_cases

pytestmark = pytest.mark.gpu

f32, f64, i32 = torch.float32, torch.float64, torch.int32
CFG_MINI = dict(block_out_channels=(320, 320, 320, 320), layers_per_block=1, cross_attention_dim=256, attention_head_dim=8)
GUARD = 64
SCALE = 7.5
EINVAL = -22
_cache = {}


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _rel(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).norm() / ref.norm()).item()


def _bits(t):
    return t.contiguous().view(i32)


def _p(t):
    return None if t is None else t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


class _Arena:
    """an output of n fp32 elements with GUARD NaN sentinels in front of it and behind it, one allocation, all NaN to begin with"""

    def __init__(self, n, device, fill=None):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), device=device, dtype=f32)
        self.out = self.buf[GUARD:GUARD + n]
        if fill is not None:
            self.out.copy_(fill.reshape(-1))

    def guards_hold(self, what):
        assert bool(self.buf[:GUARD].isnan().all()) and bool(self.buf[GUARD + self.n:].isnan().all()), f"{what}: a store outside the output"

    def untouched(self, what):
        assert bool(self.buf.isnan().all()), f"{what}: something was written"


def _table(device, S=30):
    if S not in _cache:
        smp = DDIMSampler(device)
        smp.make_schedule(S, verbose=False)
        _cache[S] = smp
    return _cache[S]


def _invert(eps, x, coef, index, cfg, case, pred=True, alias=False):
    """one launch of seer_cfg_ddim_invert_step through the raw binding -> (x_next, pred_x0 or None), both inside sentinels"""
    b, C, Ft, cond_f, HW = case
    n = x.numel()
    xn = _Arena(n, x.device, fill=x if alias else None)
    px = _Arena(n, x.device) if pred else None
    rc = _lib.load().seer_cfg_ddim_invert_step(_p(eps), int(cfg), b, C, Ft, cond_f, HW, SCALE, _p(coef), index, None, None,
                                               _p(xn.out if alias else x), _p(xn.out), _p(px.out) if pred else None, _s())
    assert rc == 0, rc
    torch.cuda.synchronize()
    xn.guards_hold("x_next")
    if pred:
        px.guards_hold("pred_x0")
    return xn.out.reshape(x.shape), (px.out.reshape(x.shape) if pred else None)


def _cfg64(eps, cfg, case):
    """the CFG-combined eps of the prediction frames in float64, and the sum of its operands' magnitudes"""
    b, cond_f = case[0], case[3]
    ev = eps[:, :, cond_f:]
    if not cfg:
        return ev, ev.abs()
    return ev[:b] + SCALE * (ev[b:] - ev[:b]), ev[:b].abs() + (SCALE + 1) * (ev[b:] - ev[:b]).abs() + ev[b:].abs()


def _invert_allowance(emag, x, row):
    """Per element, counted on the kernel's fp32 operations, each rounding at most 2^-24 of a magnitude that the sum of its operands'
    magnitudes bounds.  pred_x0 = (x - sqrtf(1 - a_prev) e) / sqrtf(a_prev) is reached through 9 roundings: the CFG pair's
    difference, product and sum (3); 1 - a_prev, its sqrtf and the product with e (3); the subtraction from x; sqrtf(a_prev); the
    division.  Magnitude X0 = (|x| + sqrt(1 - a_prev) E) / sqrt(a_prev), E the magnitude of e: 10 x 2^-24 x X0, one rounding in hand
    for the second-order terms.  x_next = sqrtf(a_t) x0 + s1m e adds sqrtf(a_t) and its product to the 9 of x0 (11, on sqrt(a_t) X0),
    the product s1m e to the 3 of e (4, on s1m E), and the final sum: at most 12 on T = sqrt(a_t) X0 + s1m E, so 13 x 2^-24 x T.
    A contracted multiply-add only removes roundings."""
    a_t, a_prev, _, s1m = row
    x0m = (x.abs() + math.sqrt(1.0 - a_prev) * emag) / math.sqrt(a_prev)
    tot = math.sqrt(a_t) * x0m + s1m * emag
    return 13 * 2.0 ** -24 * tot + 2.0 ** -126, 10 * 2.0 ** -24 * x0m + 2.0 ** -126


# ---- 1. the kernel against float64, per element -------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("cond_f", [0, 2])
@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "nocfg"])
def test_invert_kernel_against_float64(device, cfg, cond_f, b):
    """[b, 4, cond_f + 3, HW = 50]: b x 600 elements, no multiple of the 256-thread block; rows 0, 15 and 30 of the S = 30 schedule,
    a_prev from 0.9999 down to 5e-3, where the division amplifies 14 times.  The conditioning frames of eps hold NaN: never read."""
    case = (b, 4, cond_f + 3, cond_f, 50)
    smp = _table(device)
    coef = smp.ddim_coef
    top = coef.shape[0] - 1
    assert top == 30 and abs(float(coef[0, 1]) - 0.9999) < 1e-4 and float(coef[top, 1]) < 1e-2
    eps, x, _ = N.cfg_problem(case, cfg, device, 300 + 7 * b + cond_f, exact=False)
    e32, x32 = eps.to(f32).contiguous(), x.to(f32).contiguous()
    e64, emag = _cfg64(eps, cfg, case)
    shares = []
    for index in (0, 15, top):
        row = [float(v) for v in coef[index]]
        want_next, want_x0 = R.invert_step64(e64, x, row)
        allow_next, allow_x0 = _invert_allowance(emag, x, row)
        xn, px = _invert(e32, x32, coef, index, cfg, case)
        what = f"seer_cfg_ddim_invert_step {case} cfg{int(cfg)} row {index}"
        shares.append((_bound(xn, want_next, allow_next, f"{what}: x_next"), _bound(px, want_x0, allow_x0, f"{what}: pred_x0")))
        # pred_x0 = NULL and x_next aliasing x change no bit of x_next; the wrapper is the same launch
        xn2, none = _invert(e32, x32, coef, index, cfg, case, pred=False)
        assert none is None and torch.equal(_bits(xn2), _bits(xn)), f"{what}: pred_x0 NULL changes x_next"
        xa, pa = _invert(e32, x32, coef, index, cfg, case, alias=True)
        assert torch.equal(_bits(xa), _bits(xn)) and torch.equal(_bits(pa), _bits(px)), f"{what}: x_next aliasing x"
        shape5 = (b, 4, 3, 5, 10)
        wn, wp = ops.cfg_ddim_invert_step(e32.reshape(-1, 4, cond_f + 3, 5, 10), x32.reshape(shape5), coef, index, cfg=cfg, scale=SCALE,
                                          cond_f=cond_f)
        assert torch.equal(_bits(wn.reshape(x.shape)), _bits(xn)) and torch.equal(_bits(wp.reshape(x.shape)), _bits(px))
    print(f"invert | {case} cfg{int(cfg)} | share of the allowance used (x_next, pred_x0) rows 0, 15, 30: "
          + ", ".join(f"({a:.3f}, {c:.3f})" for a, c in shares))
    if cond_f:
        assert bool(e32[:, :, :cond_f].isnan().all())


# ---- 2. the DDIM step is its inverse ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "nocfg"])
def test_the_ddim_step_takes_the_inverted_latent_back(device, cfg):
    """seer_cfg_ddim_step on the same eps and row undoes the inversion exactly in exact arithmetic (sigma = 0); on the device it
    returns x within the sum of the two kernels' bounds, the DDIM step's taken at the latent it was given"""
    b, cond_f = 2, 2
    case = (b, 4, cond_f + 3, cond_f, 50)
    coef = _table(device).ddim_coef
    eps, x, _ = N.cfg_problem(case, cfg, device, 300 + 7 * b + cond_f, exact=False)
    e32, x32 = eps.to(f32).contiguous(), x.to(f32).contiguous()
    _, emag = _cfg64(eps, cfg, case)
    for index in (0, 15, 30):
        row = [float(v) for v in coef[index]]
        assert row[2] == 0.0
        xn, _ = _invert(e32, x32, coef, index, cfg, case)
        back = _Arena(x.numel(), device)
        rc = _lib.load().seer_cfg_ddim_step(_p(e32), int(cfg), b, 4, cond_f + 3, cond_f, 50, SCALE, _p(coef), index, None,
                                            _p(xn.contiguous()), None, None, 0.0, _p(back.out), None, _s())
        assert rc == 0
        torch.cuda.synchronize()
        back.guards_hold("x_prev")
        allow = _invert_allowance(emag, x, row)[0] + N.cfg_ddim_allowance(eps, xn.to(f64), None, row, cfg, SCALE, case)[0]
        share = _bound(back.out.reshape(x.shape), x, allow, f"invert then seer_cfg_ddim_step, row {index}")
        print(f"invert | inverse property cfg{int(cfg)} row {index} | share of the summed allowance used {share:.3f}")


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------
def test_invert_refusals_write_nothing(device):
    """every SEER_EINVAL branch, decided on the host, with real buffers behind the pointers: the NaN-filled outputs keep their bits"""
    n = 2 * 4 * 3 * 50
    a = _Arena(4 * n, device)                            # eps, coef, x, outputs: every pointer lands inside this allocation
    words = torch.zeros((4,), dtype=i32, device=device)
    lib, count = _lib.load(), 0
    for fn, args, why in refusal_cases(a.out.data_ptr(), words.data_ptr()):
        assert getattr(lib, fn)(*args, _s()) == EINVAL, (fn, why)
        count += 1
    torch.cuda.synchronize()
    a.untouched("a refused call")
    assert count >= 30 and words.tolist() == [0, 0, 0, 0]


# ---- 4. the device-counter form -------------------------------------------------------------------------------------------------------
def test_device_counter_chain_equals_host_index_kernel_and_stops_at_the_limit(device):
    smp = _table(device, 6)
    n = smp.ddim_coef.shape[0]
    limit = 3
    assert n == 7 >= limit + 2                           # seer_ddim_step_begin reads t_table[index] on the two launches past the limit too
    b, C, Fp, cond_f, h, w = 2, 4, 3, 1, 5, 10
    eps_seq = [_randn((2 * b, C, Fp + cond_f, h, w), 100 + k).to(device) for k in range(limit + 2)]
    x0 = _randn((b, C, Fp, h, w), 99, 0.8).to(device)
    x, want = x0, []
    for k in range(limit):
        x, pred = ops.cfg_ddim_invert_step(eps_seq[k], x, smp.ddim_coef, k, cfg=True, scale=SCALE, cond_f=cond_f)
        want.append((x, pred))
    step = torch.tensor([0, 77], dtype=i32, device=device)
    lim = torch.tensor([limit], dtype=i32, device=device)
    xd, pd = _Arena(x0.numel(), device, fill=x0), _Arena(x0.numel(), device)
    xv, pv = xd.out.reshape(x0.shape), pd.out.reshape(x0.shape)
    sample, t_out = torch.empty((b, C, Fp, h, w), device=device), torch.empty((b,), dtype=torch.long, device=device)
    for k in range(limit + 2):
        ops.ddim_step_begin(None, xv, smp._t_table, step, 1, sample, t_out)
        ops.cfg_ddim_invert_step_dev(eps_seq[k], xv, smp.ddim_coef, step, lim, cfg=True, scale=SCALE, cond_f=cond_f, x_next=xv, pred_x0=pv)
        torch.cuda.synchronize()
        j = min(k, limit - 1)                            # past the limit the buffers keep the last step's bits
        assert torch.equal(_bits(xv), _bits(want[j][0])) and torch.equal(_bits(pv), _bits(want[j][1])), k
        assert step.tolist() == [k + 1, k] and lim.tolist() == [limit], (k, step.tolist())
        assert torch.equal(t_out, smp._t_table[k].expand(b))
        xd.guards_hold("x_next")
        pd.guards_hold("pred_x0")
    # limit = 0: the launch writes its counter word and nothing else; a counter below 0 likewise
    for start in (0, -2):
        step = torch.tensor([99, start], dtype=i32, device=device)
        lim = torch.tensor([0 if start == 0 else 5], dtype=i32, device=device)
        xd, pd = _Arena(x0.numel(), device), _Arena(x0.numel(), device)
        ops.cfg_ddim_invert_step_dev(eps_seq[0], x0, smp.ddim_coef, step, lim, cfg=True, scale=SCALE, cond_f=cond_f,
                                     x_next=xd.out.reshape(x0.shape), pred_x0=pd.out.reshape(x0.shape))
        torch.cuda.synchronize()
        xd.untouched(f"index {start}, limit {lim.tolist()}")
        pd.untouched(f"index {start}, limit {lim.tolist()}")
        assert step.tolist() == [start + 1, start]


# ---- 5. the captured step -------------------------------------------------------------------------------------------------------------
def _mini(device, **kw):
    """the mini UNet of tests/test_gpu_plms.py as instances of this file's own: the graphs captured here stay out of the caches that
    other test files count"""
    key = ("mini", tuple(sorted(kw.items())))
    if key not in _cache:
        m = SeerUNet(**CFG_MINI, **kw)
        m.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI)), strict=True)
        _cache[key] = m.to(device).eval()
    return _cache[key]


def _draw(device, seed, b=1, f1=1, Fp=2, H=16):
    D = CFG_MINI["cross_attention_dim"]
    return dict(x0_emb=_randn((b, 4, f1, H, H), seed, 0.9).to(device), c=_randn((b, f1 + Fp, 77, D), seed + 1).to(device),
                uc=_randn((1, 1, 77, D), seed + 2).expand(b, f1 + Fp, -1, -1).contiguous().to(device),
                x0=_randn((b, 4, Fp, H, H), seed + 3, 0.8).to(device))


def _encode(smp, m, graph, i, t_enc, scale, **kw):
    m.use_graph = graph
    try:
        return smp.encode(m, i["x0"], i["c"], t_enc, return_intermediates=1, unconditional_guidance_scale=scale,
                          unconditional_conditioning=i["uc"], x0_emb=i["x0_emb"], cond_frames=1, **kw)
    finally:
        m.use_graph = False


def test_captured_inversion_step_equals_the_launch_by_launch_step(device):
    """unet.use_graph: every step of encode is ONE hipGraph (seer_ddim_step_begin, the UNet, seer_cfg_ddim_invert_step_dev).  The same
    bits as the launches over whole chains: new inputs on the same graph, t_enc 4 and then 2, scale 7.5 and 1.0; what the caller keeps
    is not written again; torch's generator is not touched; the kinds other samplers capture keep their keys."""
    m = _mini(device)
    smp = DDIMSampler(device)
    smp.make_schedule(4, verbose=False)
    torch.manual_seed(5)
    state = torch.cuda.get_rng_state(device)
    kept = []
    for seed, t_enc, scale in ((1, 4, SCALE), (11, 2, SCALE), (21, 4, SCALE), (31, 3, 1.0)):
        i = _draw(device, seed)
        x0_before = i["x0"].clone()
        want, wi = _encode(smp, m, False, i, t_enc, scale)
        got, gi = _encode(smp, m, True, i, t_enc, scale)
        assert torch.isfinite(got).all() and torch.equal(got, want), (seed, t_enc, scale)
        assert len(gi["x_inter"]) == len(gi["pred_x0"]) == t_enc
        assert all(torch.equal(a, b_) for a, b_ in zip(gi["x_inter"] + gi["pred_x0"], wi["x_inter"] + wi["pred_x0"])), (seed, t_enc)
        assert torch.equal(i["x0"], x0_before)
        kept.append((got, got.clone(), gi, [t.clone() for t in gi["x_inter"] + gi["pred_x0"]]))
        # one key per CFG form (a context of another batch empties the cache): t_enc, the inputs and the prompt are no part of it
        keys = [k for k in m._engine._graphs if isinstance(k, tuple) and k and k[0] == "invert"]
        assert len(keys) == 1 and keys[0][3] == (scale != 1.0) and keys[0][5] == (scale if scale != 1.0 else None), keys
    for got, copy, gi, copies in kept:                   # nothing a later step or chain wrote reached what the caller kept
        assert torch.equal(got, copy) and all(torch.equal(a, b_) for a, b_ in zip(gi["x_inter"] + gi["pred_x0"], copies))
    assert torch.equal(torch.cuda.get_rng_state(device), state)
    # a decode through the same model puts the key it always put, the kind "step", and the "invert" key beside it differs in that
    # word alone
    i = _draw(device, 1)
    m.use_graph = True
    try:
        down = smp.decode(m, kept[0][0], i["c"], 4, SCALE, i["uc"], x0_emb=i["x0_emb"], cond_frames=1)
    finally:
        m.use_graph = False
    assert torch.isfinite(down).all()
    assert torch.equal(_encode(smp, m, True, i, 4, SCALE)[0], kept[0][0])
    by_kind = {k[0]: k for k in m._engine._graphs if isinstance(k, tuple) and k}
    assert set(by_kind) == {"invert", "step"} and by_kind["step"][1:] == by_kind["invert"][1:], by_kind
    # p_invert_ddim on its own: the caller's tensors, captured or not
    outs = {}
    for graph in (False, True):
        m.use_graph = graph
        try:
            x, seq = i["x0"], []
            for index in range(3):
                x, pred = smp.p_invert_ddim(m, x, i["c"], smp._t_table[index].expand(1), index, x0_emb=i["x0_emb"], cond_frames=1,
                                            unconditional_guidance_scale=SCALE, unconditional_conditioning=i["uc"])
                seq.append((x, pred))
        finally:
            m.use_graph = False
        outs[graph] = seq
    for (xa, pa), (xb, pb) in zip(outs[False], outs[True]):
        assert torch.equal(xa, xb) and torch.equal(pa, pb)
    assert len({t.data_ptr() for s in outs[True] for t in s}) == 6
    assert all(torch.equal(a, b_) for (a, _), b_ in zip(outs[True], kept[0][2]["x_inter"]))


# ---- 6. layout invariance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
def test_encode_of_a_batch_equals_the_solo_encodes(device, use_graph):
    m = _mini(device, layout_invariant=True)
    smp = DDIMSampler(device)
    smp.make_schedule(4, verbose=False)
    rows = [_draw(device, 51, H=8), _draw(device, 61, H=8)]
    pair = {k: torch.cat([r[k] for r in rows]).contiguous() for k in rows[0]}
    got, gi = _encode(smp, m, use_graph, pair, 3, SCALE)
    for r, row in enumerate(rows):
        want, wi = _encode(smp, m, use_graph, row, 3, SCALE)
        assert torch.isfinite(want).all() and torch.equal(got[r:r + 1], want), r
        assert all(torch.equal(a[r:r + 1], b_) for a, b_ in zip(gi["x_inter"] + gi["pred_x0"], wi["x_inter"] + wi["pred_x0"])), r


# ---- 7. the round trip on the analytic model ------------------------------------------------------------------------------------------
def test_round_trip_on_the_gaussian_model(device):
    """the analytic Gaussian model as a Python model on the eager path (the real kernels, S = 20, t_enc = the whole schedule):
    encode -> decode follows the float64 restatement of the same chain, and comes at least five times closer to the clip it started
    from than stochastic_encode(seed=) -> decode"""
    smp = DDIMSampler(device)
    smp.make_schedule(20, verbose=False)
    n = int(smp.ddim_timesteps.shape[0])
    G = R.gaussian_case(smp.alphas_cumprod.cpu())
    coef, ts, x0 = smp.ddim_coef.cpu(), smp.ddim_timesteps, G["x0"]
    model = lambda x, t, c, cond_frame=0: G["eps"](x.double().cpu(), t).float().to(x.device)
    c = torch.zeros((1, x0.shape[2], 1, 1), device=device)
    x32 = x0.float().to(device)
    lat, _ = smp.encode(model, x32, c, n)
    back = smp.decode(model, lat, c, n)
    sde = smp.decode(model, smp.stochastic_encode(x32, n - 1, seed=7), c, n)
    lat64, _ = R.encode64(G["eps"], x0.float(), coef, ts, n)
    back64 = R.decode64(G["eps"], lat64, coef, ts, n)
    r_lat, r_back = _rel(lat, lat64), _rel(back, back64)
    trip, trip_sde = _rel(back, x0), _rel(sde, x0)
    print(f"invert | Gaussian model S=20: encode to float64 {r_lat:.3g}, round trip to float64 {r_back:.3g}; round trip to the clip "
          f"{trip:.3g}, stochastic_encode's {trip_sde:.3g}")
    assert r_lat <= 1e-5 and r_back <= 1e-5, (r_lat, r_back)
    assert trip <= trip_sde / 5, (trip, trip_sde)


# ---- 8. edit_clips(invert=True) -------------------------------------------------------------------------------------------------------
def test_edit_clips_invert_on_the_tiny_pipeline(device, monkeypatch):
    unet_cfg = dict(block_out_channels=(320, 320, 320, 320), layers_per_block=1, cross_attention_dim=192, attention_head_dim=8)
    fst_cfg = dict(num_frames=6, num_layers=2, channels=192, n_heads=2, cross_attention_dim=192)
    vae_kw = dict(ch=128, ch_mult=(1, 1, 2, 2), num_res_blocks=1)
    unet = SeerUNet(**unet_cfg, layout_invariant=True)
    unet.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(unet_cfg)), strict=True)
    fst = FSTextTransformer(num_frames=6, in_channels=192, out_channels=192, n_heads=2, num_layers=2, cross_attention_dim=192)
    fst.load_state_dict(synth.synth_state_dict(synth.fstext_param_shapes(**fst_cfg)), strict=True)
    vsd = {**synth.synth_state_dict(synth.vae_param_shapes(**vae_kw)),
           **synth.synth_state_dict(synth.vae_encoder_param_shapes(**vae_kw, z_channels=4))}
    vae = AutoencoderKL(block_out_channels=(128, 128, 256, 256), layers_per_block=1)
    vae.load_state_dict(ldm_to_diffusers_vae(vsd, 4), strict=True)
    unet, fst, vae = unet.to(device).eval(), fst.to(device).eval(), vae.to(device)
    video = torch.tanh(_randn((1, 3, 3, 64, 64), 50)).to(device)
    text, source, empty = (_randn((1, 77, 192), s).to(device) for s in (60, 61, 3))
    latents = []
    real = pipeline.latents_to_clip
    monkeypatch.setattr(pipeline, "latents_to_clip", lambda v, lat: (latents.append(lat.clone()), real(v, lat))[1])
    gen = lambda: torch.Generator(device=device).manual_seed(5)
    run = lambda **kw: edit_clips(unet, fst, vae, DDIMSampler(device), video, text, empty, cond_frames=1, ddim_steps=4, seed=None,
                                  latent_generator=gen(), invert=True, strength=0.75, **kw)
    unet.use_graph = True                                # the captured steps here, the launches in the round trip below
    clip = run(source_emb=source, source_scale=2.0, scale=7.5)
    assert clip.shape == (1, 3, 2, 64, 64) and torch.isfinite(clip).all() and clip.min() >= 0 and clip.max() <= 1
    assert torch.equal(run(source_emb=source, source_scale=2.0, scale=7.5), clip)
    assert not torch.equal(run(source_emb=text, source_scale=2.0, scale=7.5), clip)        # the source prompt is in the result
    # source prompt = target prompt, both scales 1: the latents are the round trip's, bit for bit
    del latents[:]
    clip1 = run(source_emb=text, source_scale=1.0, scale=1.0)
    unet.use_graph = False
    lat = frames_to_latents(vae, video, gen())
    x0_emb, given = lat[:, :, :1].contiguous(), lat[:, :, 1:].contiguous()
    fst.set_numframe(3)
    c = fst(context=text)
    smp = DDIMSampler(device)
    smp.make_schedule(4, verbose=False)
    t_enc = pipeline.edit_t_enc(0.75, 4)
    assert t_enc == 3
    up, _ = smp.encode(unet, given, c, t_enc, x0_emb=x0_emb)
    down = smp.decode(unet, up, c, t_enc, x0_emb=x0_emb)
    assert len(latents) == 1 and torch.equal(latents[0], down)
    assert torch.isfinite(clip1).all() and clip1.min() >= 0 and clip1.max() <= 1
    print(f"invert | edit_clips round trip on the tiny pipeline, 3 of 4 entries: rel_l2 of the latents to the given ones {_rel(down, given):.3g}")
