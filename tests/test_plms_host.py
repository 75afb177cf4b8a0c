"""PLMSSampler on the host: the PLMS restatement (tests/plms_oracle.py) over the oracle's tiny UNet against the REAL reference
PLMSSampler's outputs (tests/golden/plms_sample_tiny.npz, written by scripts/make_goldens_plms.py), the schedule it shares with
DDIMSampler, its argument checks and the compat runner's sampler switch.  Runs everywhere (CPU)."""
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import ref_import
from oracle import seer_oracle as O
from seervideoldm_amd import DDIMSampler, PLMSSampler, compat, synth
from tests import plms_oracle as P

G = Path(__file__).resolve().parent / "golden"
TINY_UNET = dict(sample_size=16, in_channels=4, out_channels=4, block_out_channels=(32, 64, 64, 64),
                 cross_attention_dim=64, attention_head_dim=8, layers_per_block=2)


@pytest.fixture(scope="module")
def tiny_unet_fn():
    sd = synth.synth_state_dict(synth.unet_param_shapes(TINY_UNET))
    return lambda x, t, c, cf: O.unet_forward(sd, TINY_UNET, x, t, c, cond_frame=cf)


def _run_restatement(unet_fn, S, scale, x0_emb, c, uc, x_T, seed):
    draws = [0]

    def draw():
        draws[0] += 1
        torch.randn(x_T.shape)
    torch.manual_seed(seed)
    with torch.no_grad():
        lat, steps = P.plms_sampling(P.seer_eps_fn(unet_fn, c, x0_emb, scale, uc), S, x_T, draw)
    return lat, steps, draws[0], torch.rand(4)


@pytest.mark.parametrize("case", ["cfg", "s1", "S1"])
def test_restatement_reproduces_the_reference_sampler(tiny_unet_fn, case):
    g = {k: torch.from_numpy(v) if v.ndim else v for k, v in np.load(G / "plms_sample_tiny.npz").items()}
    S, scale = int(g[f"{case}_S"]), float(g[f"{case}_scale"])
    lat, steps, draws, rng = _run_restatement(tiny_unet_fn, S, scale, g["x0_emb"], g["c"], g["uc"], g["x_T"], int(g["seed"]))
    assert len(steps) == g[f"{case}_x_prev"].shape[0] == (S if S > 1 else 1)
    # test_oracle_golden.py::test_ddim_step_and_sample's tolerances: a step, and the sample
    for i, (x_prev, pred_x0, e_t) in enumerate(steps):
        torch.testing.assert_close(x_prev, g[f"{case}_x_prev"][i], rtol=1e-4, atol=1e-4, msg=f"{case} step {i} x_prev")
        torch.testing.assert_close(pred_x0, g[f"{case}_pred_x0"][i], rtol=1e-4, atol=2e-4, msg=f"{case} step {i} pred_x0")
        torch.testing.assert_close(e_t, g[f"{case}_e_t"][i], rtol=1e-4, atol=2e-4, msg=f"{case} step {i} e_t")
    torch.testing.assert_close(lat, g[f"{case}_latent"], rtol=1e-3, atol=1e-3)
    # the reference draws twice on the first step and once on every later one; the seeded stream ends where it does
    assert draws == int(g[f"{case}_draws"]) == len(steps) + 1
    assert torch.equal(rng, g[f"{case}_rng_after"])


def test_every_order_runs_in_the_four_step_case():
    g = np.load(G / "plms_sample_tiny.npz")
    assert int(g["cfg_S"]) == 4 and g["cfg_e_t"].shape[0] == 4
    # the steps differ from a DDIM walk: the multistep combination is not the plain eps
    assert not np.allclose(g["cfg_latent"], g["s1_latent"])


@pytest.mark.skipif(not ref_import.available(), reason="the reference checkout is not on this machine")
def test_restatement_against_the_reference_sampler_on_fresh_inputs(tiny_unet_fn):
    from scripts import make_goldens_plms as M
    ref = ref_import.load_reference()
    plms = M.load_plms(ref)
    unet = M.tiny_unet(ref)
    x0_emb, c, uc, x_T = M.inputs(seed=901)
    for S, scale, cf in ((5, 7.5, 1), (6, 1.0, 0)):
        r = M.run_reference(ref, plms, unet, S, scale, x0_emb, c, uc, x_T, cond_frames=cf, seed=77)
        torch.manual_seed(77)
        with torch.no_grad():
            lat, steps = P.plms_sampling(P.seer_eps_fn(tiny_unet_fn, c, x0_emb, scale, uc, cf), S, x_T,
                                         lambda: torch.randn(x_T.shape))
        for i, (x_prev, pred_x0, e_t) in enumerate(steps):
            torch.testing.assert_close(x_prev, r["x_prev"][i], rtol=1e-4, atol=1e-4)
            torch.testing.assert_close(pred_x0, r["pred_x0"][i], rtol=1e-4, atol=2e-4)
            torch.testing.assert_close(e_t, r["e_t"][i], rtol=1e-4, atol=2e-4)
        torch.testing.assert_close(lat, r["latent"], rtol=1e-3, atol=1e-3)
        assert torch.equal(torch.rand(4), r["rng_after"])


@pytest.mark.parametrize("S", [4, 30, 50])
def test_schedule_is_ddims(S):
    d, p = DDIMSampler("cpu"), PLMSSampler("cpu")
    d.make_schedule(S, verbose=False)
    p.make_schedule(S, verbose=False)
    assert np.array_equal(p.ddim_timesteps, d.ddim_timesteps)
    for name in ("ddim_alphas", "ddim_alphas_prev", "ddim_sigmas", "ddim_sqrt_one_minus_alphas"):
        assert np.array_equal(getattr(p, name), getattr(d, name)), name
    assert torch.equal(p.ddim_coef, d.ddim_coef) and torch.equal(p._t_table, d._t_table)
    assert torch.equal(p.alphas_cumprod, d.alphas_cumprod) and torch.equal(p.betas, d.betas)


def test_eta_is_refused():
    with pytest.raises(ValueError):
        PLMSSampler("cpu").make_schedule(4, ddim_eta=0.1, verbose=False)
    with pytest.raises(ValueError):
        PLMSSampler("cpu").sample(unet=None, S=4, batch_size=1, shape=(4, 2, 8, 8), eta=0.1, verbose=False, is_3d=True)


def test_four_d_sampling_and_unbuilt_options_are_refused():
    s = PLMSSampler("cpu")
    with pytest.raises(NotImplementedError):
        s.sample(unet=None, S=4, batch_size=1, shape=(4, 8, 8), verbose=False, is_3d=False)
    with pytest.raises(NotImplementedError):
        s.sample(unet=None, S=4, batch_size=1, shape=(4, 2, 8, 8), verbose=False, is_3d=True, noise_dropout=0.1)
    s.make_schedule(4, verbose=False)
    x, t = torch.zeros(1, 4, 2, 8, 8), torch.ones(1, dtype=torch.long)
    for kw in (dict(noise_dropout=0.5), dict(use_original_steps=True), dict(repeat_noise=True)):
        with pytest.raises(NotImplementedError):
            s.p_sample_plms(None, x, None, t, 3, old_eps=[], t_next=t, **kw)
    with pytest.raises(NotImplementedError):
        s.p_sample_ddim(None, x, None, t, 3)


@pytest.fixture
def compat_env(monkeypatch):
    yield monkeypatch
    compat.uninstall()


def test_compat_sampler_switch(compat_env):
    compat_env.setenv("SEER_COMPAT_SAMPLER", "plms")
    compat.install()
    from ldm.models.diffusion.ddim_video import DDIMSampler as Aliased
    assert Aliased is PLMSSampler


@pytest.mark.parametrize("value", [None, "", "ddim", "dpm"])
def test_compat_sampler_default(compat_env, value):
    if value is None:
        compat_env.delenv("SEER_COMPAT_SAMPLER", raising=False)
    else:
        compat_env.setenv("SEER_COMPAT_SAMPLER", value)
    compat.install()
    from ldm.models.diffusion.ddim_video import DDIMSampler as Aliased
    assert Aliased is DDIMSampler
