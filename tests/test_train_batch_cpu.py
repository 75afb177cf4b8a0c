"""CPU side of SeerTrainer.step_from_batch (train.py:330-387 from a dataloader batch): the DDPM table without diffusers, and the
step's host logic -- call order, ONE VAE encode over all frames in (b f) order, the random draws in train.py's order -- on the
plain-torch stand-ins (tests/torch_ops_backend.py, tests/torch_train_ops_backend.py + the train_inputs stand-in of
tests/train_inputs_ref.py).  NOT a product path: on a GPU box the same code runs on libseer_hip.so (tests/test_gpu_train_batch.py)."""
from types import SimpleNamespace

import pytest
import torch

from seervideoldm_amd import FSTextTransformer, SeerUNet, synth
from seervideoldm_amd.trainer import SeerTrainer, ddpm_alphas_cumprod
from tests import torch_ops_backend as tob
from tests.train_inputs_ref import TrainOpsWithInputs, reference

CFG = dict(block_out_channels=(320, 320, 320, 320), layers_per_block=1, cross_attention_dim=192, attention_head_dim=8)
FS = dict(num_frames=16, num_layers=1, channels=192, n_heads=2, cross_attention_dim=192)
HP = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, max_grad_norm=0.3)


# ------------------------------------------------------------------------------------------------------ the DDPM table
@pytest.mark.parametrize("schedule", ["scaled_linear", "linear"])
def test_ddpm_alphas_cumprod_matches_the_closed_form(schedule):
    """against the same two schedules in float64 (diffusers itself is not a dependency: this pins the arithmetic, not the package)"""
    T, b0, b1 = 1000, 0.00085, 0.012
    a = ddpm_alphas_cumprod(T, b0, b1, schedule)
    assert a.dtype == torch.float32 and a.shape == (T,)
    if schedule == "scaled_linear":
        betas = torch.linspace(b0 ** 0.5, b1 ** 0.5, T, dtype=torch.float64) ** 2
    else:
        betas = torch.linspace(b0, b1, T, dtype=torch.float64)
    ref = torch.cumprod(1.0 - betas, 0)
    assert float(((a.double() - ref).abs() / ref).max()) < 1e-6
    assert bool((a[1:] < a[:-1]).all()) and 0.0 < float(a[-1]) and float(a[0]) < 1.0
    assert torch.equal(ddpm_alphas_cumprod(), ddpm_alphas_cumprod(1000, 0.00085, 0.012, "scaled_linear"))


def test_ddpm_alphas_cumprod_rejects_other_schedules():
    with pytest.raises(NotImplementedError):
        ddpm_alphas_cumprod(beta_schedule="squaredcos_cap_v2")


# ------------------------------------------------------------------------------------------------------ the step's host logic
class _Vae:
    """records every encode; moments [N, 8, H/8, W/8] as a fixed function of the pixels"""

    def __init__(self, events):
        self.events, self.inputs = events, []

    def encode(self, x):
        self.events.append("vae.encode")
        self.inputs.append(x)
        p = torch.nn.functional.avg_pool2d(x.float(), 8)                       # [N, 3, h, w]
        m = torch.cat([p, p.flip(1), p[:, :2] * 0.5], 1)                        # [N, 8, h, w]: 4 means | 4 log-variances
        return SimpleNamespace(latent_dist=SimpleNamespace(parameters=m))


class _Text:
    def __init__(self, events, table):
        self.events, self.table, self.masks = events, table, []

    def __call__(self, input_ids, attention_mask=None):
        self.events.append("text_encoder")
        self.masks.append(attention_mask)
        return (self.table[input_ids[:, 0]],)


@pytest.fixture(scope="module")
def models():
    usd = synth.synth_state_dict(synth.unet_param_shapes(CFG))
    fsd = synth.synth_state_dict(synth.fstext_param_shapes(**FS))
    unet = SeerUNet(**CFG)
    unet.load_state_dict(usd, strict=True)
    fst = FSTextTransformer(num_frames=FS["num_frames"], in_channels=192, out_channels=192, n_heads=2, num_layers=1,
                            cross_attention_dim=192)
    fst.load_state_dict(fsd, strict=True)
    return unet, fst


def _trainer(models, Fr, events, real_step, **kw):
    """a trainer on the stand-ins whose forward_backward / optimizer_step are logged (and, for real_step=False, replaced: the draws and
    the call order do not need the network)"""
    unet, fst = models
    fst.set_numframe(Fr)
    tops = TrainOpsWithInputs()
    tr = SeerTrainer(unet, fst, ops=tob, tops=tops, **HP, **kw)
    inner_fb, inner_opt, inner_ti = tr.forward_backward, tr.optimizer_step, tops.train_inputs

    def fb(*a, **k):
        events.append("forward_backward")
        tr.fb_args = (a, k)
        return inner_fb(*a, **k) if real_step else torch.zeros(1)

    def opt(lr=None):
        events.append(("optimizer_step", lr))
        if real_step:
            inner_opt(lr)

    def ti(*a, **k):
        events.append("train_inputs")
        return inner_ti(*a, **k)

    tr.forward_backward, tr.optimizer_step, tops.train_inputs = fb, opt, ti
    return tr, tops


def _batch(b, Fr, seed):
    g = torch.Generator().manual_seed(seed)
    video = torch.rand((b, 3, Fr, 64, 64), generator=g) * 2 - 1
    ids = torch.randint(0, 8, (b, 77), generator=g)
    return video, ids, torch.ones((b, 77), dtype=torch.int64)


def test_step_runs_on_the_stand_ins_in_the_reference_order(models):
    """text encoder -> ONE encode of all b*F frames, (b f) order -> ONE train_inputs -> forward_backward on what it returned -> optimizer"""
    events = []
    b, Fr, cond = 1, 3, 1
    tr, tops = _trainer(models, Fr, events, real_step=True)
    vae, text = _Vae(events), _Text(events, torch.randn((8, 77, 192), generator=torch.Generator().manual_seed(4)))
    video, ids, mask = _batch(b, Fr, 1)
    g = torch.Generator().manual_seed(2)
    noise, pn = torch.randn((b, 4, Fr - cond, 8, 8), generator=g), torch.randn((b * Fr, 4, 8, 8), generator=g)
    t, acp = torch.tensor([417]), ddpm_alphas_cumprod()
    p0 = tr.pu.p.clone()
    loss = tr.step_from_batch(video, ids, mask, vae=vae, text_encoder=text, cond_frames=cond, alphas_cumprod=acp, lr=5e-4,
                              noise=noise, timesteps=t, posterior_noise=pn)
    assert events == ["text_encoder", "vae.encode", "train_inputs", "forward_backward", ("optimizer_step", 5e-4)]
    assert text.masks[0] is mask
    assert len(vae.inputs) == 1 and vae.inputs[0].shape == (b * Fr, 3, 64, 64)
    for bi in range(b):
        for f in range(Fr):
            assert torch.equal(vae.inputs[0][bi * Fr + f], video[bi, :, f])
    call = tops.calls[0]
    assert len(tops.calls) == 1 and call["cond_frames"] == cond and call["latent_scale"] == 0.18215
    assert torch.equal(call["eps_post"], pn) and torch.equal(call["noise"], noise) and torch.equal(call["timesteps"], t)
    x_ref = reference(vae.encode(vae.inputs[0]).latent_dist.parameters, pn, noise, t, acp, cond, 0.18215)[0].float()
    model_input, noise_l, t_l, text_l = tr.last_inputs
    assert torch.equal(model_input, x_ref) and model_input.shape == (b, 4, Fr, 8, 8)
    assert torch.equal(noise_l, noise) and torch.equal(t_l, t) and torch.equal(text_l, text.table[ids[:, 0]])
    (a, k) = tr.fb_args
    assert a[0] is model_input and a[1] is noise_l and a[2] is t_l and a[3] is text_l and a[4] == cond and k["use_graph"] is False
    assert torch.isfinite(loss).all() and tr.step_count == 1 and not torch.equal(tr.pu.p, p0)


def test_uninjected_draws_follow_train_py(models):
    """train.py:349 (posterior noise of the frames to predict), :350 (of the conditioning frames), :357 (torch.randn(latents.shape), CPU
    generator), :360 (randint): on the CPU all four come from one generator, so a restatement in that order reproduces them"""
    events = []
    b, Fr, cond, T = 2, 4, 1, 1000
    f2 = Fr - cond
    tr, tops = _trainer(models, Fr, events, real_step=False)
    vae, text = _Vae(events), _Text(events, torch.zeros((8, 77, 192)))
    video, ids, mask = _batch(b, Fr, 3)
    torch.manual_seed(77)
    tr.step_from_batch(video, ids, mask, vae=vae, text_encoder=text, cond_frames=cond, alphas_cumprod=ddpm_alphas_cumprod(T))
    torch.manual_seed(77)
    e2 = torch.randn((b * f2, 4, 8, 8))                                       # train.py:349
    e1 = torch.randn((b * cond, 4, 8, 8))                                     # train.py:350
    noise = torch.randn((b, 4, f2, 8, 8))                                     # train.py:357
    t = torch.randint(0, T, (b,))                                             # train.py:360
    call = tops.calls[0]
    eps = call["eps_post"].view(b, Fr, 4, 8, 8)
    assert torch.equal(eps[:, :cond], e1.view(b, cond, 4, 8, 8)) and torch.equal(eps[:, cond:], e2.view(b, f2, 4, 8, 8))
    assert torch.equal(call["noise"], noise) and torch.equal(call["timesteps"], t) and call["_timesteps_in_range"] is True
    assert torch.equal(tr.last_inputs[1], noise) and torch.equal(tr.last_inputs[2], t)
    assert events.count("vae.encode") == 1 and events.count("train_inputs") == 1


def test_accumulation_and_errors(models):
    events = []
    b, Fr, cond = 1, 3, 2
    tr, _ = _trainer(models, Fr, events, real_step=False, gradient_accumulation_steps=2)
    vae, text = _Vae(events), _Text(events, torch.zeros((8, 77, 192)))
    video, ids, mask = _batch(b, Fr, 5)
    kw = dict(vae=vae, text_encoder=text, cond_frames=cond, alphas_cumprod=ddpm_alphas_cumprod())
    tr.step_from_batch(video, ids, mask, **kw)
    assert not any(isinstance(e, tuple) for e in events)                       # first micro-batch: no optimizer step
    tr.step_from_batch(video, ids, mask, **kw)
    assert sum(isinstance(e, tuple) for e in events) == 1
    with pytest.raises(ValueError):
        tr.step_from_batch(video, ids, mask, **{**kw, "cond_frames": Fr})      # nothing left to predict
    with pytest.raises(ValueError, match="set_numframe"):
        tr.step_from_batch(_batch(b, Fr + 1, 5)[0], ids, mask, **kw)           # the FSTextTransformer is set to Fr frames
    with pytest.raises(ValueError):
        tr.step_from_batch(video, ids, mask, timesteps=torch.tensor([1000]), **kw)
