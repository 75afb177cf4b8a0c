"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/plms_sample_tiny.npz by driving the REAL reference PLMSSampler
(ldm/models/diffusion/plms.py, imported through oracle/ref_import.py) over the reference's tiny SeerUNet on CPU fp32:

    python -m scripts.make_goldens_plms

The reference sampler calls a 4-D `model.apply_model`; `SeerPLMSAdapter` turns that into Seer's model call (x0_emb in front of the
latent along frames, cond_frame on the CFG pair, conditioning frames sliced off) and carries the float32 tables that the reference
DDIMSampler.make_schedule builds, so both samplers see one schedule.  Weights are the closed-form synth weights (not stored);
inputs and the reference's outputs are stored, nothing else.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from oracle import ref_import  # noqa: E402
from seervideoldm_amd import synth  # noqa: E402

OUT = ROOT / "tests" / "golden" / "plms_sample_tiny.npz"
TINY_UNET = dict(sample_size=16, in_channels=4, out_channels=4, block_out_channels=(32, 64, 64, 64),
                 cross_attention_dim=64, attention_head_dim=8, layers_per_block=2)
B, F1, FP, H = 1, 2, 2, 16
CASES = {"cfg": dict(S=4, scale=7.5), "s1": dict(S=4, scale=1.0), "S1": dict(S=1, scale=7.5)}
SEED = 123


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def inputs(seed=60):
    """x0_emb, c, uc (one prompt repeated over frames, batched-CFG form), x_T"""
    x0_emb = _randn((B, 4, F1, H, H), seed) * 0.9
    c = _randn((B, F1 + FP, 77, 64), seed + 1)
    uc = _randn((B, 1, 77, 64), seed + 2).expand(-1, F1 + FP, -1, -1).contiguous()
    return x0_emb, c, uc, _randn((B, 4, FP, H, H), seed + 3)


class SeerPLMSAdapter:
    """the `model` the reference PLMSSampler expects, over a Seer UNet: apply_model on [b, C*Fp, H, W]"""

    def __init__(self, ref, unet, x0_emb, cond_frames):
        smp = ref.ddim.DDIMSampler("cpu")
        smp.make_schedule(ddim_num_steps=4, ddim_eta=0.0, verbose=False)      # the tables do not depend on S
        self.num_timesteps = smp.ddpm_num_timesteps
        self.betas, self.alphas_cumprod, self.alphas_cumprod_prev = smp.betas, smp.alphas_cumprod, smp.alphas_cumprod_prev
        self.device = torch.device("cpu")
        self.unet, self.x0_emb, self.cond_frames = unet, x0_emb, cond_frames

    def apply_model(self, x4d, t, c):
        bb, CF, h, w = x4d.shape
        b, C, f1 = self.x0_emb.shape[:3]
        x = x4d.reshape(bb, C, CF // C, h, w)
        reps = bb // b
        x_cat = torch.cat([self.x0_emb.repeat(reps, 1, 1, 1, 1), x], dim=2)
        # ddim_video.py:195-204: cond_frame goes with the CFG pair only
        out = self.unet(x_cat, t, c, cond_frame=self.cond_frames if reps == 2 else 0)
        return out[:, :, f1:].reshape(bb, CF, h, w)


def load_plms(ref):
    import importlib
    plms = importlib.import_module("ldm.models.diffusion.plms")
    # as oracle/ref_import.py does for DDIMSampler: no forced .to("cuda") (plms.py:18-22)
    plms.PLMSSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)
    return plms


def tiny_unet(ref):
    unet = ref.unet.SeerUNet(**TINY_UNET).eval()
    ref_import.enable_xformers_path(unet)
    unet.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(TINY_UNET)), strict=True)
    return unet


@torch.no_grad()
def run_reference(ref, plms, unet, S, scale, x0_emb, c, uc, x_T, cond_frames=0, seed=SEED):
    """the reference sampler -> dict(latent, x_prev [S', ...], pred_x0, e_t, draws, rng_after)"""
    model = SeerPLMSAdapter(ref, unet, x0_emb, cond_frames)
    smp = plms.PLMSSampler(model)
    steps, draws = [], [0]
    orig = smp.p_sample_plms

    def record(*a, **k):
        out = orig(*a, **k)
        steps.append([o.reshape(x_T.shape) for o in out])
        return out
    smp.p_sample_plms = record
    noise_like = plms.noise_like

    def counting(*a, **k):
        draws[0] += 1
        return noise_like(*a, **k)
    plms.noise_like = counting
    try:
        torch.manual_seed(seed)
        b, C, Fp, h, w = x_T.shape
        lat, _ = smp.sample(S=S, batch_size=b, shape=(C * Fp, h, w), conditioning=c, verbose=False, eta=0.0,
                            x_T=x_T.reshape(b, C * Fp, h, w), unconditional_guidance_scale=scale,
                            unconditional_conditioning=uc)
        rng_after = torch.rand(4)
    finally:
        plms.noise_like = noise_like
    return dict(latent=lat.reshape(x_T.shape), x_prev=torch.stack([s[0] for s in steps]),
                pred_x0=torch.stack([s[1] for s in steps]), e_t=torch.stack([s[2] for s in steps]),
                draws=np.int64(draws[0]), rng_after=rng_after)


def main():
    ref = ref_import.load_reference()
    plms = load_plms(ref)
    unet = tiny_unet(ref)
    x0_emb, c, uc, x_T = inputs()
    arrs = dict(x0_emb=x0_emb, c=c, uc=uc, x_T=x_T, seed=np.int64(SEED))
    for name, cs in CASES.items():
        r = run_reference(ref, plms, unet, cs["S"], cs["scale"], x0_emb, c, uc, x_T)
        arrs.update({f"{name}_{k}": v for k, v in r.items()})
        arrs[f"{name}_S"], arrs[f"{name}_scale"] = np.int64(cs["S"]), np.float64(cs["scale"])
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
    print(f"wrote {OUT.name} ({OUT.stat().st_size} bytes): " + ", ".join(sorted(arrs)))


if __name__ == "__main__":
    main()
