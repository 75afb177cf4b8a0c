"""The scenarios of tests/test_gpu_sampler_graphs.py and oracle/make_goldens_sampler_keys.py: one sample per kind of captured sampler
step, through the public surface of DDIMSampler / PLMSSampler / SlotSampler only, so the same file runs on either side of a change to
the samplers' host code.

The mini UNet of tests/test_gpu_unet.py (layout-invariant, an instance of its own: its graph cache is cleared per scenario), b = 1, one
conditioning latent, two predicted frames, a 16 x 16 latent, S = 4, scale 7.5 unless the scenario says otherwise: the smallest shape at
which every captured step exists (h and w are multiples of 8).

    inputs(device, p)                 the tensors of pass p, made afresh from CPU generators (pass 0 and pass 1 differ in every one)
    sampler(name, model, device)      a fresh sampler of the scenario
    sample(name, smp, model, inp)     one sample; a list of latents
    recorded_keys()                   context manager: every key handed to the engine's graph_put, in order
"""
import contextlib

import torch

from seervideoldm_amd import DDIMSampler, PLMSSampler, SeerUNet, SlotSampler, synth
from seervideoldm_amd import unet as unet_module

CFG_MINI = dict(block_out_channels=(320, 320, 320, 320), layers_per_block=1, cross_attention_dim=256, attention_head_dim=8)
F1, FP, HL, S, SCALE, D = 1, 2, 16, 4, 7.5, 256
SHAPE = (4, FP, HL, HL)

# name -> (sampler class, constructor keywords, sample keywords)
SCENARIOS = {
    "ddim_cfg": (DDIMSampler, {}, {}),
    "ddim_plain": (DDIMSampler, {}, dict(scale=1.0)),
    "ddim_seeded": (DDIMSampler, {}, dict(eta=0.5, seeded=True)),
    "ddim_masked": (DDIMSampler, {}, dict(seeded=True, masked=True)),
    "plms_cfg": (PLMSSampler, {}, {}),
    "slots": (SlotSampler, {}, {}),
    "slots_plms": (SlotSampler, dict(plms=True), dict(methods=("ddim", "plms"))),
    "slots_rng": (SlotSampler, dict(stochastic=True), dict(eta=0.5, seeded=True)),
    "slots_edit": (SlotSampler, dict(editing=True), dict(seeded=True, masked=True)),
    "slots_edit_rng": (SlotSampler, dict(editing=True, stochastic=True), dict(eta=0.5, seeded=True, masked=True)),
}
TORCH_SEED = 1234          # torch's generator in front of pass 1: the unseeded steps draw from it, the seeded ones leave it alone

_models = {}


def model(device):
    if "m" not in _models:
        m = SeerUNet(**CFG_MINI, layout_invariant=True)
        m.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI)), strict=True)
        _models["m"] = m.to(device).eval()
    return _models["m"]


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def inputs(device, p):
    """two requests' worth of everything a scenario may take (the single-clip samplers use the first)"""
    k = 1000 * (p + 1)
    reqs = []
    for r in range(2):
        u = torch.rand((1, 1, FP, HL, HL), generator=torch.Generator().manual_seed(k + 60 + r))
        reqs.append(dict(x_T=_randn((1, *SHAPE), k + r).to(device), x0_emb=_randn((1, 4, F1, HL, HL), k + 10 + r, 0.9).to(device),
                         c=_randn((1, F1 + FP, 77, D), k + 20 + r).to(device),
                         uc=_randn((1, 1, 77, D), k + 30 + r).expand(-1, F1 + FP, -1, -1).contiguous().to(device),
                         seed=(k + 40 + r) * 0x9E3779B97F4A7C15 % (1 << 64),
                         mask=torch.where(u < 0.4, torch.zeros_like(u), torch.where(u > 0.6, torch.ones_like(u), u)).to(device),
                         known=_randn((1, *SHAPE), k + 50 + r, 0.8).to(device), scale=(SCALE, 3.0)[r]))
    return reqs


def sampler(name, m, device):
    cls, ctor, _ = SCENARIOS[name]
    if cls is SlotSampler:
        return SlotSampler(m, 2, shape=SHAPE, cond_frames=F1, context_shape=(77, D), device=device, model_cond_frame=F1, **ctor)
    return cls(device)


def sample(name, smp, m, reqs):
    cls, _, kw = SCENARIOS[name]
    eta, seeded, masked = kw.get("eta", 0.), kw.get("seeded", False), kw.get("masked", False)
    if cls is not SlotSampler:
        r = reqs[0]
        edit = dict(mask=r["mask"], x0=r["known"]) if masked else {}
        lat, _ = smp.sample(m, S, batch_size=1, shape=SHAPE, x0_emb=r["x0_emb"], conditioning=r["c"], verbose=False, cond_frames=F1,
                            unconditional_guidance_scale=kw.get("scale", SCALE), unconditional_conditioning=r["uc"], eta=eta,
                            x_T=None if seeded and not masked else r["x_T"], is_3d=True, **(dict(seed=r["seed"]) if seeded else {}),
                            **edit)
        return [lat]
    for r, method in zip(reqs, kw.get("methods", ("ddim", "ddim"))):
        extra = dict(method=method) if "methods" in kw else {}
        if seeded:
            extra.update(seed=r["seed"], **(dict(eta=eta) if eta else {}))
        if masked:
            extra.update(mask=r["mask"], x0=r["known"])
        smp.submit(r["x_T"], r["x0_emb"], r["c"], r["uc"], S, r["scale"], **extra)
    done = []
    while smp.active():
        done += smp.step()
    return [lat for _, lat in sorted(done, key=lambda d: d[0])]


@contextlib.contextmanager
def recorded_keys():
    keys, real = [], unet_module._Engine.graph_put

    def put(self, key, g):
        keys.append(key)
        return real(self, key, g)
    unet_module._Engine.graph_put = put
    try:
        yield keys
    finally:
        unet_module._Engine.graph_put = real


def two_passes(name, m, device):
    """the scenario twice on one fresh sampler under use_graph, the second time on fresh inputs of the same shapes (the first pass's
    tensors are gone before the second's are made, so their addresses may come back) -> (keys put by pass 0, by pass 1, pass 1's
    latents with a torch.rand(3) drawn after them: torch's generator is seeded in front of pass 1, as reference_pass seeds it)"""
    if m._engine is None:
        m.prepare()
    m._engine._graphs.clear()
    smp = sampler(name, m, device)
    m.use_graph = True
    try:
        with recorded_keys() as keys:
            reqs = inputs(device, 0)
            sample(name, smp, m, reqs)
            del reqs
            first = list(keys)
            del keys[:]
            reqs = inputs(device, 1)
            torch.manual_seed(TORCH_SEED)
            got = sample(name, smp, m, reqs) + [torch.rand(3, device=device)]
            return first, list(keys), got
    finally:
        m.use_graph = False


def reference_pass(name, m, device):
    """pass 1's inputs through a fresh sampler of the scenario, launch by launch"""
    m.use_graph = False
    torch.manual_seed(TORCH_SEED)
    return sample(name, sampler(name, m, device), m, inputs(device, 1)) + [torch.rand(3, device=device)]
