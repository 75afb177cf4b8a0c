"""PLMSSampler on a real MI355X: the fused CFG + PLMS kernel against float64, its device-counter / ring form against the host-index
form bit for bit, the sampler on the mini UNet against the CPU restatement (tests/plms_oracle.py over the oracle), the captured
step against the launches, the solver on an analytic model with an exact answer, and a frame-sharded two-process run."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import seer_oracle as O
from seervideoldm_amd import (AutoencoderKL, DDIMSampler, FSTextTransformer, PLMSSampler, SeerUNet, ddim_sample, ops,
                              synth)
from seervideoldm_amd.pipeline import generate_clips
from seervideoldm_amd.vae import ldm_to_diffusers_vae
from tests import plms_oracle as P
from tests.test_dist_gpu import ROOT, _backend, _host_staged_gathers, _spawn

pytestmark = pytest.mark.gpu

CFG_MINI = dict(block_out_channels=(320, 320, 320, 320), layers_per_block=1, cross_attention_dim=256, attention_head_dim=8)
NEED = (0, 1, 1, 2, 3)          # earlier eps read by order 0..4
_cache = {}


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _rel(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).norm() / ref.norm()).item()


def _model(device):
    if "mini" not in _cache:
        sd = synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI))
        m = SeerUNet(**CFG_MINI)
        m.load_state_dict(sd, strict=True)
        _cache["mini"] = (CFG_MINI, sd, m.to(device).eval())
    return _cache["mini"]


def _update64(eps, x, coef, index, order, hist, cfg, scale, cond_f):
    """the kernel's arithmetic in float64 -> (x_prev, pred_x0, e)"""
    eps, x = eps.double().cpu(), x.double().cpu()
    b = x.shape[0]
    e = eps[:, :, cond_f:]
    if cfg:
        e = e[:b] + scale * (e[b:] - e[:b])
    h = [t.double().cpu() for t in hist]
    if order == 0:
        ep = e
    elif order == 1:
        ep = (h[0] + e) / 2
    elif order == 2:
        ep = (3 * e - h[0]) / 2
    elif order == 3:
        ep = (23 * e - 16 * h[0] + 5 * h[1]) / 12
    else:
        ep = (55 * e - 59 * h[0] + 37 * h[1] - 9 * h[2]) / 24
    a_t, a_prev, sigma, s1m = coef[index].double().cpu().tolist()
    x0 = (x - s1m * ep) / a_t ** 0.5
    return a_prev ** 0.5 * x0 + (1 - a_prev - sigma ** 2) ** 0.5 * ep, x0, e


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("cond_f", [0, 2])
@pytest.mark.parametrize("cfg", [True, False])
@pytest.mark.parametrize("order", range(5))
def test_plms_kernel_matches_float64(device, order, cfg, cond_f, b):
    smp = DDIMSampler(device)
    smp.make_schedule(10, verbose=False)
    C, Fp, h, w = 4, 3, 8, 12
    eps = _randn(((2 if cfg else 1) * b, C, Fp + cond_f, h, w), 1).to(device)
    x = _randn((b, C, Fp, h, w), 2).to(device)
    hist = [_randn(x.shape, 3 + k).to(device) for k in range(NEED[order])]
    nan = torch.full(x.shape, float("nan"), device=device)
    padded = hist + [nan] * (3 - len(hist))                 # slots the order does not use hold NaN: never read
    index = 6
    x_prev, pred, e = ops.cfg_plms_step(eps, x, smp.ddim_coef, index, order, cfg=cfg, scale=7.5, cond_f=cond_f, history=padded)
    rx, rp, re = _update64(eps, x, smp.ddim_coef, index, order, hist, cfg, 7.5, cond_f)
    outs = [(x_prev, rx, "x_prev"), (pred, rp, "pred_x0")] + ([(e, re, "e")] if order != 1 else [])
    for got, want, what in outs:
        assert torch.isfinite(got).all(), what
        rel = _rel(got, want)
        assert rel <= 1e-6, (what, rel)
    assert (e is None) == (order == 1)
    # x aliasing x_prev, and the new eps written over the oldest history slot the order reads
    xa = x.clone()
    ha = [t.clone() for t in padded]
    e_out = ha[NEED[order] - 1] if order >= 2 else None
    x2, p2, e2 = ops.cfg_plms_step(eps, xa, smp.ddim_coef, index, order, cfg=cfg, scale=7.5, cond_f=cond_f, history=ha,
                                   x_prev=xa, e_out=e_out)
    assert x2 is xa and torch.equal(xa, x_prev) and torch.equal(p2, pred)
    if order != 1:
        assert torch.equal(e2, e) and (e_out is None or e2 is e_out)


# ---- 2. the device-counter form ------------------------------------------------------------------------------------------
def test_device_counter_chain_equals_host_index_kernel(device):
    smp = DDIMSampler(device)
    smp.make_schedule(6, verbose=False)
    n = smp.ddim_coef.shape[0]
    b, C, Fp, cond_f, h, w = 2, 4, 3, 1, 8, 8
    eps_seq = [_randn((2 * b, C, Fp + cond_f, h, w), 100 + k).to(device) for k in range(n)]
    x_T = _randn((b, C, Fp, h, w), 99).to(device)
    x, hist, want = x_T, [], []               # hist: newest first
    for k in range(n):
        order = 0 if not hist else len(hist) + 1
        x, pred, e = ops.cfg_plms_step(eps_seq[k], x, smp.ddim_coef, n - 1 - k, order, cfg=True, scale=7.5, cond_f=cond_f,
                                       history=hist)
        want.append((x, pred))
        hist = ([e] + hist)[:3]
    step = torch.tensor([n - 1, 0], dtype=torch.int32, device=device)
    ring = torch.full((3, b, C, Fp, h, w), float("nan"), device=device)        # stale contents: never read while not valid
    rs = torch.zeros(4, dtype=torch.int32, device=device)
    p = 2 * ((n - 1) & 1)
    rs[p], rs[p + 1] = 0, 2
    xd, pd = x_T.clone(), torch.empty_like(x_T)
    sample, t_out = torch.empty((b, C, Fp, h, w), device=device), torch.empty((b,), dtype=torch.long, device=device)
    for k in range(n):
        ops.ddim_step_begin(None, xd, smp._t_table, step, 1, sample, t_out)
        ops.cfg_plms_step_dev(eps_seq[k], xd, smp.ddim_coef, step, ring, rs, cfg=True, scale=7.5, cond_f=cond_f, x_prev=xd,
                              pred_x0=pd)
        assert torch.equal(xd, want[k][0]) and torch.equal(pd, want[k][1]), k
        assert torch.equal(t_out, smp._t_table[n - 1 - k].expand(b))
    assert int(step[0]) == -1
    for j, e in enumerate(hist):             # the last three eps, newest in the slot of step n - 1
        assert torch.equal(ring[(n - 1 - j) % 3], e), j
    assert rs[2:4].tolist() == [3, (n - 1) % 3]


# ---- 3. the sampler on the mini UNet ---------------------------------------------------------------------------------------
def test_plms_sampler_and_decode_match_oracle(device):
    cfg, sd, m = _model(device)
    b, f1, Fp, H = 1, 1, 2, 16
    x0_emb = _randn((b, 4, f1, H, H), 1) * 0.9
    c = _randn((b, f1 + Fp, 77, cfg["cross_attention_dim"]), 2)
    uc = _randn((b, 1, 77, cfg["cross_attention_dim"]), 3).expand(-1, f1 + Fp, -1, -1).contiguous()
    noise = _randn((b, 4, Fp, H, H), 4)
    unet_fn = lambda x, t, cc, cf: O.unet_forward(sd, cfg, x, t, cc, cond_frame=cf)
    with torch.no_grad():
        ref_lat, _ = P.plms_sampling(P.seer_eps_fn(unet_fn, c, x0_emb, 7.5, uc), 4, noise)
    sampler = PLMSSampler(device)
    lat, inter = sampler.sample(unet=m, S=4, conditioning=c.to(device), batch_size=b, shape=(4, Fp, H, H),
                                x0_emb=x0_emb.to(device), verbose=False, unconditional_guidance_scale=7.5,
                                unconditional_conditioning=uc.to(device), eta=0.0, x_T=noise.to(device), is_3d=True)
    assert sampler.ddim_timesteps.tolist() == [1, 251, 501, 751]
    assert len(inter["x_inter"]) == 3 and len(inter["pred_x0"]) == 3
    rel = _rel(lat, ref_lat)
    print(f"[parity] plms latent after 4 CFG steps: rel_l2={rel:.4g}")
    assert rel <= 8e-2, rel
    # ddim_sample drives the PLMS sampler unchanged: the same latent, decoded
    vae_kw = dict(ch=128, ch_mult=(1, 1, 2, 2), num_res_blocks=1)
    vae = AutoencoderKL(block_out_channels=(128, 128, 256, 256), layers_per_block=1)
    vae.load_state_dict(ldm_to_diffusers_vae(synth.synth_state_dict(synth.vae_param_shapes(**vae_kw)), 4), strict=True)
    vae = vae.to(device)
    clip = ddim_sample(sampler, m, vae, (b, 4, Fp, H, H), c.to(device), noise.to(device), x0_emb.to(device), ddim_steps=4,
                       scale=7.5, uc=uc.to(device))
    z = (lat.permute(0, 2, 1, 3, 4).reshape(b * Fp, 4, H, H) * (1 / 0.18215)).contiguous()
    x = vae.decode(z).sample
    want = ops.clamp01_(x.reshape(b, Fp, *x.shape[1:]).permute(0, 2, 1, 3, 4).contiguous().float())
    assert clip.shape == (b, 3, Fp, 8 * H, 8 * H) and torch.equal(clip, want)


def test_generate_clips_accepts_the_plms_sampler(device):
    unet_cfg = dict(block_out_channels=(320, 320, 320, 320), layers_per_block=1, cross_attention_dim=192, attention_head_dim=8)
    fst_cfg = dict(num_frames=6, num_layers=2, channels=192, n_heads=2, cross_attention_dim=192)
    vae_kw = dict(ch=128, ch_mult=(1, 1, 2, 2), num_res_blocks=1)
    unet = SeerUNet(**unet_cfg)
    unet.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(unet_cfg)), strict=True)
    fst = FSTextTransformer(num_frames=6, in_channels=192, out_channels=192, n_heads=2, num_layers=2, cross_attention_dim=192)
    fst.load_state_dict(synth.synth_state_dict(synth.fstext_param_shapes(**fst_cfg)), strict=True)
    vsd = {**synth.synth_state_dict(synth.vae_param_shapes(**vae_kw)),
           **synth.synth_state_dict(synth.vae_encoder_param_shapes(**vae_kw, z_channels=4))}
    vae = AutoencoderKL(block_out_channels=(128, 128, 256, 256), layers_per_block=1)
    vae.load_state_dict(ldm_to_diffusers_vae(vsd, 4), strict=True)
    unet, fst, vae = unet.to(device).eval(), fst.to(device).eval(), vae.to(device)
    img = torch.tanh(_randn((1, 3, 1, 64, 64), 1)).to(device)
    text, empty = _randn((1, 77, 192), 2).to(device), _randn((1, 77, 192), 3).to(device)

    def run(sampler):
        return generate_clips(unet, fst, vae, sampler, img, text, empty, num_frames=3, cond_frames=1, ddim_steps=4, scale=7.5,
                              noise_generator=torch.Generator().manual_seed(4),
                              latent_generator=torch.Generator(device=device).manual_seed(5))[0]
    a, b_ = run(PLMSSampler(device)), run(PLMSSampler(device))
    assert a.shape == (1, 3, 2, 64, 64) and torch.isfinite(a).all() and a.min() >= 0 and a.max() <= 1
    assert torch.equal(a, b_)
    assert not torch.equal(a, run(DDIMSampler(device)))


# ---- 4. the captured step --------------------------------------------------------------------------------------------------
def test_captured_plms_step_equals_the_launch_by_launch_step(device):
    """unet.use_graph: every PLMS step after the first is ONE hipGraph (seer_ddim_step_begin, the UNet, seer_cfg_plms_step_dev
    over the eps ring).  Same bits as the eager launches over whole samples: a second sample with new inputs, another schedule
    length (the ring wraps), scale 1.0, the RNG stream in the same state afterwards, and returned tensors the caller keeps."""
    cfg, sd, m = _model(device)
    b, f1, Fp, H = 1, 1, 2, 16
    sampler = PLMSSampler(device)

    def draw(seed):
        x0 = (_randn((b, 4, f1, H, H), seed) * 0.9).to(device)
        c = _randn((b, f1 + Fp, 77, cfg["cross_attention_dim"]), seed + 1).to(device)
        uc = _randn((b, 1, 77, cfg["cross_attention_dim"]), seed + 2).expand(-1, f1 + Fp, -1, -1).contiguous().to(device)
        return x0, c, uc, _randn((b, 4, Fp, H, H), seed + 3).to(device)

    def sample(graph, S, args, scale):
        x0, c, uc, noise = args
        m.use_graph = graph
        torch.manual_seed(5)
        preds = []
        lat, inter = sampler.sample(unet=m, S=S, conditioning=c, batch_size=b, shape=(4, Fp, H, H), x0_emb=x0, verbose=False,
                                    unconditional_guidance_scale=scale, unconditional_conditioning=uc, eta=0.0, x_T=noise,
                                    is_3d=True, img_callback=lambda p, i: preds.append(p))
        return lat, inter, preds, torch.rand(3, device=device)

    try:
        kept = []
        for S, seed, scale in ((4, 1, 7.5), (4, 11, 7.5), (6, 21, 7.5), (4, 31, 1.0)):
            args = draw(seed)
            want, wi, wp, wr = sample(False, S, args, scale)
            got, gi, gp, gr = sample(True, S, args, scale)
            assert torch.equal(got, want) and torch.equal(gr, wr), (S, seed)
            assert all(torch.equal(a, b_) for a, b_ in zip(gi["x_inter"] + gi["pred_x0"], wi["x_inter"] + wi["pred_x0"]))
            assert len(gp) == len(wp) == sampler.ddim_timesteps.shape[0]
            assert all(torch.equal(a, b_) for a, b_ in zip(gp, wp)), (S, seed)
            kept.append((got, got.clone(), gp, [p.clone() for p in gp]))
        for got, copy, gp, gcopy in kept:      # nothing a later step or sample wrote reached what the caller kept
            assert torch.equal(got, copy) and all(torch.equal(a, b_) for a, b_ in zip(gp, gcopy))
        assert any(isinstance(k, tuple) and k and k[0] == "plms" for k in m._engine._graphs), "the captured step never ran"
        # direct p_sample_plms calls run the launches whatever use_graph says; the returned tensors are the caller's
        x0, c, uc, noise = draw(41)
        sampler.make_schedule(4, verbose=False)
        outs = {}
        for graph in (False, True):
            m.use_graph = graph
            x, old, seq = noise, [], []
            for index in (3, 2, 1, 0):
                x, pred, e = sampler.p_sample_plms(m, x, c, sampler._t_table[index].expand(b), index, x0_emb=x0,
                                                   unconditional_guidance_scale=7.5, unconditional_conditioning=uc,
                                                   old_eps=old, t_next=sampler._t_table[max(index - 1, 0)].expand(b))
                old.append(e)
                seq.append((x, pred, e))
            outs[graph] = seq
        for (xa, pa, ea), (xb, pb, eb) in zip(outs[False], outs[True]):
            assert torch.equal(xa, xb) and torch.equal(pa, pb) and torch.equal(ea, eb)
        assert len({t.data_ptr() for s in outs[True] for t in s}) == 12
    finally:
        m.use_graph = False


# ---- 5. the solver on an analytic model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [10, 20])
def test_plms_solves_the_gaussian_probability_flow_ode(device, S):
    """Gaussian data N(mu, s^2) has the exact eps = sigma (x - alpha mu) / (alpha^2 s^2 + sigma^2), CFG-combined over one mu per
    half; the probability-flow ODE then has a closed-form end point.  The GPU run (eager path, real kernel, a Python model) follows
    its float64 restatement, and lands much closer to the exact answer than DDIM with the same steps."""
    s, scale, shape = 0.5, 7.5, (1, 4, 5, 20, 50)            # N = 20 000
    g = torch.Generator().manual_seed(3)
    mu_u = 0.3 * torch.randn(shape, generator=g, dtype=torch.float64)
    mu_c = mu_u + 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)
    x_T = torch.randn(shape, generator=g, dtype=torch.float64).float()
    ref_smp = DDIMSampler("cpu")
    ref_smp.make_schedule(S, verbose=False)
    ac = ref_smp.alphas_cumprod.double()

    def exact_eps(x, t, mu):
        a2 = ac[t.cpu().long()].view(-1, 1, 1, 1, 1)
        return (1 - a2).sqrt() * (x - a2.sqrt() * mu) / (a2 * s * s + (1 - a2))

    def analytic_unet(x, t, c, cond_frame=0):
        mu = torch.cat([mu_u, mu_c]) if x.shape[0] == 2 else mu_c
        return exact_eps(x.double().cpu(), t, mu).float().to(x.device)

    c = torch.zeros((1, 5, 1, 1), device=device)
    uc = torch.zeros((1, 5, 1, 1), device=device)

    def run(sampler):
        lat, inter = sampler.sample(unet=analytic_unet, S=S, conditioning=c, batch_size=1, shape=shape[1:], verbose=False,
                                    unconditional_guidance_scale=scale, unconditional_conditioning=uc, eta=0.0,
                                    x_T=x_T.to(device), is_3d=True, log_every_t=1)
        return lat.double().cpu(), inter["x_inter"][1:]

    plms, traj = run(PLMSSampler(device))
    ddim, _ = run(DDIMSampler(device))
    eps64 = lambda x, t: exact_eps(x, t, mu_u) + scale * (exact_eps(x, t, mu_c) - exact_eps(x, t, mu_u))
    lat64, steps64 = P.plms_sampling(eps64, S, x_T.double(), dtype=torch.float64)
    # the latent after every step (pred_x0 of the noisiest steps divides by sqrt(a_t) ~ 0.07: its fp32 rounding is not the
    # solver's)
    assert len(traj) == len(steps64)
    rels = [_rel(x, st[0]) for x, st in zip(traj, steps64)]
    assert max(rels) <= 1e-5, rels
    assert _rel(plms, lat64) <= 1e-5
    a0, aT = float(ac[0]), float(ac[int(ref_smp.ddim_timesteps[-1])])
    mu_g = mu_u + scale * (mu_c - mu_u)
    exact = a0 ** 0.5 * mu_g + ((a0 * s * s + 1 - a0) / (aT * s * s + 1 - aT)) ** 0.5 * (x_T.double() - aT ** 0.5 * mu_g)
    e_plms, e_ddim = _rel(plms, exact), _rel(ddim, exact)
    print(f"[solver] S={S}: DDIM rel err {e_ddim:.3g}, PLMS rel err {e_plms:.3g}")
    assert e_plms <= e_ddim / 5, (e_plms, e_ddim)


# ---- 6. frame-sharded -------------------------------------------------------------------------------------------------------
def _plms_worker(rank, world, port, out_path):
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    backend, dev = _backend(rank, world)
    if backend == "nccl":
        torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        from seervideoldm_amd import PLMSSampler, SeerUNet, parallel, synth
        if backend == "gloo":
            _host_staged_gathers()
        m = SeerUNet(**CFG_MINI).to(dev)
        m.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI), device=dev), strict=True)
        m.eval()
        g = torch.Generator().manual_seed(7)
        b, f1, Fp, H = 1, 1, 3, 16
        x0 = (torch.randn((b, 4, f1, H, H), generator=g) * 0.9).to(dev)
        c = torch.randn((b, f1 + Fp, 77, 256), generator=g).to(dev)
        noise = torch.randn((b, 4, Fp, H, H), generator=g).to(dev)

        # unguided: CFG at 7.5 multiplies the bf16 difference of two blockings of one evaluation by up to 16 (measured with it:
        # 3.4e-2 after the three evaluations of two steps), and the bound below is that of ONE evaluation
        def run():
            torch.manual_seed(5)
            return PLMSSampler(dev).sample(unet=m, S=2, conditioning=c, batch_size=b, shape=(4, Fp, H, H), x0_emb=x0,
                                           verbose=False, eta=0.0, x_T=noise, is_3d=True)[0].cpu()
        ref = run()
        shard = parallel.attach(m, world, rank, batch_groups=1)
        got = run()
        torch.save(dict(ref=ref, got=got, desc=shard.describe()), f"{out_path}.{rank}")
    finally:
        dist.destroy_process_group()


def test_frame_sharded_plms_sample(tmp_path):
    out = tmp_path / "res.pt"
    _spawn(_plms_worker, 2, str(out))
    r0, r1 = torch.load(f"{out}.0"), torch.load(f"{out}.1")
    assert r0["desc"].startswith("batch_groups1xframe_shards2")
    rel = ((r0["got"] - r0["ref"]).norm() / r0["ref"].norm()).item()
    print(f"[parity] 2 PLMS steps frame-sharded ({r0['desc']}) vs one process: rel_l2={rel:.4g}")
    assert rel < 3e-2, rel                                     # test_dist_gpu.py::test_sharded_step_on_hip_kernels' bound
    assert torch.equal(r0["got"], r1["got"]), "every rank runs the same update on rank 0's inputs"
