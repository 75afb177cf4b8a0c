"""The oracle restatement against the REAL reference modules on FRESH seeded inputs -- configurations and inputs the other goldens
do not contain -- to fp32 round-off.  The reference's outputs are stored fixtures (tests/golden/fresh_*.npz and
reference_names.json, written by oracle/make_goldens_fresh.py from the reference modules on exactly the inputs and closed-form
weights drawn here); the oracle runs live.  See also tests/test_oracle_golden.py, test_fstext.py, test_vae_encode.py."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import make_goldens_fresh as F
from oracle import seer_oracle as O
from seervideoldm_amd import synth

TOL = dict(rtol=1e-4, atol=3e-5)
G = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def fresh():
    return {n: np.load(G / f"fresh_{n}.npz") for n in ("unet", "unet_attn", "misc")}


def _inputs_are_the_generators(stored, *tensors):
    assert np.array_equal(np.stack([F.fingerprint(t) for t in tensors]).reshape(np.shape(stored)), stored), \
        "the seeded inputs drawn here are not the ones the reference ran on"


@pytest.mark.parametrize("cond_frame,Fr,H", F.UNET_CASES)
@torch.no_grad()
def test_unet_forward(fresh, cond_frame, Fr, H):
    # layers_per_block >= 2: with one layer the reference builds Downsample3D(in_channels, ...) from the block's INPUT width
    # (unet_3d_blocks.py:354-356 reads `in_channels` after the resnet loop re-bound it) and asserts on a widening block
    cfg = F.UNET_CFG
    shapes = synth.unet_param_shapes(cfg)
    assert set(shapes) == set(json.loads((G / "reference_names.json").read_text())["unet_state_dict_keys"])
    sd = synth.synth_state_dict(shapes)
    x, ctx, t = F.unet_inputs(Fr, H)
    k = f"unet_{cond_frame}_{Fr}_{H}"
    _inputs_are_the_generators(fresh["unet"][k + "_in"], x, ctx)
    torch.testing.assert_close(O.unet_forward(sd, cfg, x, t, ctx, cond_frame=cond_frame), torch.from_numpy(fresh["unet"][k]), **TOL)


@torch.no_grad()
def test_unet_forward_return_attn(fresh):
    """`unet(..., return_attn=True)` -> (out, attn_list): 7 entries (3 down, mid, 3 up) of pre-softmax text cross-attention
    scores [b, heads, f, h, w, L] from the LAST text block of each container (unet_3d_condition.py:291-292,317-323,372-374).
    The fixture holds each map's exact sums over L and over (h, w) with the sums of |score| that bound them, and a seeded sample
    of exact entries: every marginal must agree within what TOL allows element by element, every sampled entry within TOL."""
    cfg = F.UNET_CFG
    sd = synth.synth_state_dict(synth.unet_param_shapes(cfg))
    g = fresh["unet_attn"]
    x, ctx, t = F.attn_inputs()
    _inputs_are_the_generators(g["in"], x, ctx)
    got, got_attn = O.unet_forward(sd, cfg, x, t, ctx, cond_frame=1, return_attn=True)
    torch.testing.assert_close(got, torch.from_numpy(g["y"]), **TOL)
    assert len(got_attn) == int(g["levels"]) == 7
    for i, a in enumerate(got_attn):
        assert tuple(a.shape) == tuple(g[f"a{i}_shape"]) and a.shape[:3] == (2, 8, 3) and a.shape[-1] == 77
        a64 = a.double()
        for marg, dims, n in (("row", (-1,), a.shape[-1]), ("col", (3, 4), a.shape[3] * a.shape[4])):
            err = (a64.sum(dims) - torch.from_numpy(g[f"a{i}_{marg}sum"])).abs()
            bound = n * TOL["atol"] + TOL["rtol"] * torch.from_numpy(g[f"a{i}_{marg}abs"])
            assert bool((err <= bound).all()), (i, marg, float((err - bound).max()))
        idx = torch.from_numpy(g[f"a{i}_idx"])
        assert np.array_equal(g[f"a{i}_idx"], F.attn_sample_index(i, a.numel()))
        torch.testing.assert_close(a.flatten()[idx], torch.from_numpy(g[f"a{i}_val"]), **TOL)
    torch.testing.assert_close(got, O.unet_forward(sd, cfg, x, t, ctx, cond_frame=1), rtol=0, atol=0)


@pytest.mark.parametrize("H,W", F.NONSQ_CASES)
@torch.no_grad()
def test_unet_forward_non_square(fresh, H, W):
    """window geometry (8x8 / 4x4 windows, un-windowed levels) and frame-coupled GroupNorm at H != W"""
    cfg = F.NONSQ_CFG
    sd = synth.synth_state_dict(synth.unet_param_shapes(cfg))
    x, ctx, t = F.nonsq_inputs(H, W)
    _inputs_are_the_generators(fresh["unet"][f"nonsq_{H}_{W}_in"], x, ctx)
    torch.testing.assert_close(O.unet_forward(sd, cfg, x, t, ctx, cond_frame=1), torch.from_numpy(fresh["unet"][f"nonsq_{H}_{W}"]), **TOL)


@torch.no_grad()
def test_sampler_step_and_schedule(fresh):
    sched = O.make_schedule(10)
    assert list(sched["ddim_timesteps"]) == list(fresh["misc"]["ddim_timesteps"])
    torch.testing.assert_close(torch.as_tensor(sched["alphas"], dtype=torch.float32), torch.from_numpy(fresh["misc"]["ddim_alphas"]),
                               rtol=1e-6, atol=0)


@pytest.mark.parametrize("Fr,heads,C,l", F.FSTEXT_CASES)
@torch.no_grad()
def test_fstext(fresh, Fr, heads, C, l):
    sd = synth.synth_state_dict(synth.fstext_param_shapes(num_frames=7, num_layers=1, channels=C, n_heads=heads,
                                                          cross_attention_dim=C))
    ctx = F.fstext_input(C, l)
    k = f"fstext_{Fr}_{heads}_{C}_{l}"
    _inputs_are_the_generators(fresh["misc"][k + "_in"], ctx)
    torch.testing.assert_close(O.fstext_forward(sd, ctx, Fr, heads=heads), torch.from_numpy(fresh["misc"][k]), **TOL)


@torch.no_grad()
def test_vae_both_halves(fresh):
    kw = F.VAE_KW
    esd = synth.synth_state_dict(synth.vae_encoder_param_shapes(**kw))
    dsd = synth.synth_state_dict(synth.vae_param_shapes(**kw))
    x, z = F.vae_inputs()
    _inputs_are_the_generators(fresh["misc"]["vae_in"], x, z)
    torch.testing.assert_close(O.vae_encode_moments(esd, x, ch_mult=(1, 2, 4), num_res_blocks=2),
                               torch.from_numpy(fresh["misc"]["vae_moments"]), **TOL)
    torch.testing.assert_close(O.vae_decode(dsd, z, ch_mult=(1, 2, 4), num_res_blocks=2),
                               torch.from_numpy(fresh["misc"]["vae_decoded"]), **TOL)
