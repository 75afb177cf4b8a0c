"""SeerTrainer.step_from_batch on a real MI355X: the whole call from pixels and token ids (train.py:330-387) -- its inputs to the
network against the float64 formula on the moments of one VAE encode, the step behind them against a twin trainer that is handed
those inputs through forward_backward (the same kernels on the same inputs: bit for bit), hipGraph replay, gradient accumulation, and
the random draws of a seeded run against a restatement of train.py:349-362.

Sizes: the 320-wide one-layer SeerUNet / FSTextTransformer of tests/test_gpu_train.py, the small VAE of tests/test_vae_encode.py, two
videos of four 64x64 frames (8x8 latents)."""
import pytest
import torch

from seervideoldm_amd import AutoencoderKL, FSTextTransformer, SeerUNet, synth
from seervideoldm_amd.trainer import SeerTrainer, ddpm_alphas_cumprod
from seervideoldm_amd.vae import ldm_to_diffusers_vae
from tests.train_inputs_ref import reference, worst_ratio

pytestmark = pytest.mark.gpu

CFG_MINI = dict(block_out_channels=(320, 320, 320, 320), layers_per_block=1, cross_attention_dim=192, attention_head_dim=8)
FS = dict(num_frames=16, num_layers=1, channels=192, n_heads=2, cross_attention_dim=192)
HP = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, max_grad_norm=0.3)
B, FR, PIX, LAT, T = 2, 4, 64, 8, 1000
SCALE = 0.18215


class StubTextEncoder:
    """a fixed random [8, 77, 192] table looked up by input_ids[:, 0], returned the way transformers returns it"""

    def __init__(self, device):
        self.table = torch.randn((8, 77, 192), generator=torch.Generator().manual_seed(40)).to(device)
        self.calls = 0

    def __call__(self, input_ids, attention_mask=None):
        self.calls += 1
        return (self.table[input_ids[:, 0].to(self.table.device)],)


@pytest.fixture(scope="module")
def world(device):
    usd = synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI), device=device)
    fsd = synth.synth_state_dict(synth.fstext_param_shapes(**FS), device=device)
    unet = SeerUNet(**CFG_MINI).to(device)
    unet.load_state_dict(usd, strict=True)
    fst = FSTextTransformer(num_frames=FS["num_frames"], in_channels=192, out_channels=192, n_heads=2, num_layers=1,
                            cross_attention_dim=192).to(device)
    fst.load_state_dict(fsd, strict=True)
    fst.set_numframe(FR)
    vsd = synth.synth_state_dict(synth.vae_encoder_param_shapes(ch=128, ch_mult=(1, 1, 2, 2), num_res_blocks=1, z_channels=4))
    vae = AutoencoderKL(block_out_channels=(128, 128, 256, 256), layers_per_block=1)
    vae.load_state_dict(ldm_to_diffusers_vae(vsd, 4), strict=True)
    return dict(unet=unet, fst=fst, vae=vae.to(device), text=StubTextEncoder(device), acp=ddpm_alphas_cumprod(T))


def _batch(seed, cond, device, timesteps):
    """(video, input_ids, attention_mask) + the three injected random tensors of one step"""
    g = torch.Generator().manual_seed(seed)
    video = torch.rand((B, 3, FR, PIX, PIX), generator=g) * 2 - 1
    ids = torch.randint(0, 8, (B, 77), generator=g)
    inj = dict(noise=torch.randn((B, 4, FR - cond, LAT, LAT), generator=g).to(device), timesteps=torch.tensor(timesteps),
               posterior_noise=torch.randn((B * FR, 4, LAT, LAT), generator=g).to(device))
    return (video, ids, torch.ones((B, 77), dtype=torch.int64)), inj


def _step(tr, world, batch, cond, **kw):
    return tr.step_from_batch(*batch, vae=world["vae"], text_encoder=world["text"], cond_frames=cond, alphas_cumprod=world["acp"], **kw)


def _moments(world, video, device):
    frames = video.to(device).permute(0, 2, 1, 3, 4).reshape(B * FR, 3, PIX, PIX)
    return world["vae"].encode(frames).latent_dist.parameters


@pytest.mark.parametrize("cond", [2, 1])
def test_inputs_meet_the_formula_and_the_step_is_forward_backward_on_them(device, world, cond):
    batch, inj = _batch(10 + cond, cond, device, [0, T - 1])
    tr = SeerTrainer(world["unet"], world["fst"], **HP)
    twin = SeerTrainer(world["unet"], world["fst"], **HP)                       # the same weights: neither has stepped yet
    loss = _step(tr, world, batch, cond, **inj)
    model_input, noise, t, text = tr.last_inputs
    assert model_input.shape == (B, 4, FR, LAT, LAT) and torch.equal(noise, inj["noise"]) and t.tolist() == [0, T - 1]
    assert torch.equal(text, world["text"].table[batch[1][:, 0].to(device)])
    # the inputs: the float64 formula on the moments of ONE encode over all frames, under the kernel's bound
    mom = _moments(world, batch[0], device)
    rx, _, bound, _ = reference(mom.cpu(), inj["posterior_noise"].cpu(), noise.cpu(), t.cpu(), world["acp"], cond, SCALE)
    r = worst_ratio(model_input, rx, bound)
    print(f"cond_frames {cond}: model_input worst |err| / bound {r:.3f}")
    assert r <= 1.0
    # the step: a twin handed those inputs runs the same kernels on the same inputs
    loss2 = twin.forward_backward(model_input, noise, t, text, cond)
    assert torch.equal(loss, loss2) and torch.isfinite(loss).all()
    assert torch.equal(tr.pu.g, twin.pu.g) and torch.equal(tr.pf.g, twin.pf.g)
    twin.optimizer_step()
    assert tr.step_count == twin.step_count == 1
    assert torch.equal(tr.pu.p, twin.pu.p) and torch.equal(tr.pf.p, twin.pf.p) and torch.equal(tr.pu.pb, twin.pu.pb)


def test_graph_replay_is_bit_identical_to_the_eager_call(device, world):
    """two batches with different pixels and timesteps: the second one is a pure replay of the graphs the first one captured"""
    cond = 2
    batches = [_batch(21, cond, device, [417, 93]), _batch(22, cond, device, [5, 800])]
    runs = []
    for use_graph in (False, True):
        tr = SeerTrainer(world["unet"], world["fst"], **HP)
        out = []
        for batch, inj in batches:
            loss = _step(tr, world, batch, cond, use_graph=use_graph, **inj)
            out.append((loss.clone(), tr.last_inputs[0].clone(), tr.pu.g.clone(), tr.pf.g.clone(), tr.pu.p.clone(), tr.pf.p.clone()))
        assert use_graph is False or not getattr(tr, "_graph_broken", False)
        runs.append(out)
    assert not torch.equal(runs[0][0][1], runs[0][1][1])
    for eager, graph in zip(*runs):
        assert all(torch.equal(a, b) for a, b in zip(eager, graph))


def test_optimizer_runs_on_every_second_call_under_accumulation(device, world):
    cond = 2
    tr = SeerTrainer(world["unet"], world["fst"], gradient_accumulation_steps=2, **HP)
    p0 = tr.pu.p.clone()
    _step(tr, world, _batch(31, cond, device, [100, 200])[0], cond)
    assert tr.step_count == 0 and torch.equal(tr.pu.p, p0)
    _step(tr, world, _batch(32, cond, device, [300, 400])[0], cond)
    assert tr.step_count == 1 and not torch.equal(tr.pu.p, p0)


def test_seeded_run_draws_as_train_py_does(device, world):
    """nothing injected: torch.manual_seed seeds the CPU and the device generator; the four draws of train.py:349-362 restated here in
    that order give the same noise and timesteps exactly, and the same posterior noise (through the formula on model_input)"""
    cond, f2 = 1, FR - 1
    batch, _ = _batch(41, cond, device, [0, 0])
    losses = []
    for _ in range(2):
        tr = SeerTrainer(world["unet"], world["fst"], **HP)
        torch.manual_seed(123)
        losses.append(_step(tr, world, batch, cond).clone())
    assert torch.equal(losses[0], losses[1])
    torch.manual_seed(123)
    e2 = torch.randn((B * f2, 4, LAT, LAT), device=device)                     # train.py:349  vae.encode(images).latent_dist.sample()
    e1 = torch.randn((B * cond, 4, LAT, LAT), device=device)                   # train.py:350  vae.encode(x0_image).latent_dist.sample()
    noise = torch.randn((B, 4, f2, LAT, LAT)).to(device)                       # train.py:357  torch.randn(latents.shape).to(device)
    t = torch.randint(0, T, (B,), device=device).long()                        # train.py:360-362
    model_input, noise_l, t_l, _ = tr.last_inputs
    assert torch.equal(noise_l, noise) and torch.equal(t_l, t)
    eps = torch.cat([e1.view(B, cond, 4, LAT, LAT), e2.view(B, f2, 4, LAT, LAT)], 1).reshape(B * FR, 4, LAT, LAT)
    rx, _, bound, _ = reference(_moments(world, batch[0], device).cpu(), eps.cpu(), noise.cpu(), t.cpu(), world["acp"], cond, SCALE)
    assert worst_ratio(model_input, rx, bound) <= 1.0


def test_value_errors(device, world):
    cond = 2
    batch, inj = _batch(51, cond, device, [1, 2])
    tr = SeerTrainer(world["unet"], world["fst"], **HP)
    with pytest.raises(ValueError):
        _step(tr, world, batch, FR, **{**inj, "noise": None})                  # video.shape[2] <= cond_frames
    longer = (torch.zeros((B, 3, FR + 1, PIX, PIX)),) + batch[1:]
    with pytest.raises(ValueError, match="set_numframe"):
        _step(tr, world, longer, cond)
    with pytest.raises(ValueError):
        _step(tr, world, batch, cond, **{**inj, "timesteps": torch.tensor([0, T])})
    assert tr.step_count == 0
