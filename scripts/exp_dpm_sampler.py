"""DPM-Solver++ against DDIM at BASELINE config 2 (b = 1 with batched CFG, F = 12 with 2 conditioning frames, 32x32 latent, bf16,
full-size UNet with closed-form weights), every sampler captured (unet.use_graph):

  * the steady captured step of each sampler, ms (median over the replayed steps of a sample; events recorded by `callback`), and
    the first step of a sample, which is a replay too;
  * the end-to-end clip latency -- ddim_sample: the sampler, then the VAE decode of the 10 predicted frames to 256x256 -- at S = 50
    with DDIM against S = 25 ('uniform') and S = 20 ('logsnr') with DPMSolverSampler;
  * the analytic Gaussian model (tests/dpm_ref.py: data N(0.3, 0.7^2) per element, the exact eps, a closed-form end point): max
    error of the final latent over x_T in [-3, 3] for DDIM and 2M on both grids, on the GPU kernels.  An ODE-accuracy figure on an
    analytic model, not a statement about sample quality on real weights.

    python scripts/exp_dpm_sampler.py [--samples 3] [--skip-unet]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def analytic_table(dev):
    from seervideoldm_amd import DDIMSampler, DPMSolverSampler
    from tests import dpm_ref as R
    x_T = R.start_codes()
    c = torch.zeros((1, 1, 1, 1), device=dev)
    rows = {}
    for S in (10, 20, 25, 40, 50, 100):
        row = {}
        for name, make in (("ddim_uniform", lambda: DDIMSampler(dev)), ("2m_uniform", lambda: DPMSolverSampler(dev)),
                           ("2m_logsnr", lambda: DPMSolverSampler(dev, discretize="logsnr"))):
            smp = make()
            smp.make_schedule(S, verbose=False)
            eps, _ = R.gaussian(smp.alphas_cumprod)
            model = lambda x, t, cc, cond_frame=0: eps(x.double().cpu(), t).float().to(x.device)
            lat, _ = smp.sample(model, S, 1, x_T.shape[1:], conditioning=c, x_T=x_T.float().to(dev), verbose=False, is_3d=True)
            row[name] = float(f"{R.max_error(lat, smp, x_T):.3g}")
            row[name + "_entries"] = int(smp.ddim_timesteps.shape[0])
        rows[S] = row
        print(f"analytic S={S}: {row}", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--skip-unet", action="store_true", help="the analytic table only")
    args = ap.parse_args()
    from seervideoldm_amd import AutoencoderKL, DDIMSampler, DPMSolverSampler, SeerUNet, ddim_sample, synth
    from seervideoldm_amd.vae import ldm_to_diffusers_vae
    dev = torch.device("cuda:0")
    res = dict(analytic_max_error=analytic_table(dev))
    if args.skip_unet:
        print(json.dumps(res))
        return
    cfg = dict(synth.SD15_UNET_CFG)
    model = SeerUNet(**cfg).to(dev)
    model.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(cfg), device=dev), strict=True)
    model.eval()
    model.use_graph = True
    vae = AutoencoderKL().to(dev)
    vae.load_state_dict(ldm_to_diffusers_vae(synth.synth_state_dict(synth.vae_param_shapes(), device=dev), 4))
    g = torch.Generator().manual_seed(0)
    b, f1, F, h = 1, 2, 12, 32
    x_T = torch.randn((b, 4, F - f1, h, h), generator=g).to(dev)
    x0_emb = (torch.randn((b, 4, f1, h, h), generator=g) * 0.18215 * 5).to(dev)
    c = torch.randn((b, F, 77, 768), generator=g).to(dev)
    uc = torch.randn((b, 1, 77, 768), generator=g).expand(-1, F, -1, -1).contiguous().to(dev)

    def one_sample(sampler, S):
        events = []

        def cb(i):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            events.append(ev)
        torch.cuda.synchronize()
        start = torch.cuda.Event(enable_timing=True)
        start.record()
        lat, _ = sampler.sample(unet=model, S=S, conditioning=c, batch_size=b, shape=(4, F - f1, h, h), x0_emb=x0_emb,
                                verbose=False, unconditional_guidance_scale=7.5, unconditional_conditioning=uc, eta=0.0,
                                x_T=x_T, is_3d=True, callback=cb)
        torch.cuda.synchronize()
        marks = [start] + events
        assert torch.isfinite(lat).all()
        return [marks[i].elapsed_time(marks[i + 1]) for i in range(len(events))]

    def clip_ms(sampler, S):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ddim_sample(sampler, model, vae, (b, 4, F - f1, h, h), c, x_T, x0_emb, ddim_steps=S, scale=7.5, uc=uc)
        torch.cuda.synchronize()
        assert out.shape == (b, 3, F - f1, 8 * h, 8 * h) and torch.isfinite(out).all()
        return (time.perf_counter() - t0) * 1e3

    samplers = {"ddim": DDIMSampler(dev), "dpm_uniform": DPMSolverSampler(dev), "dpm_logsnr": DPMSolverSampler(dev, discretize="logsnr")}
    # the steady step: S = 50 for both, so that the two medians are over the same number of replays
    for name in ("ddim", "dpm_uniform"):
        one_sample(samplers[name], 50)                 # capture + caches
        firsts, steady = [], []
        for _ in range(args.samples):
            per = one_sample(samplers[name], 50)
            firsts.append(per[0])
            steady.append(statistics.median(per[1:]))
        res[name + "_step"] = dict(steps=len(per), first_step_ms=[round(v, 3) for v in firsts],
                                   steady_step_ms_median=[round(v, 4) for v in steady])
        print(f"{name}: {len(per)} steps/sample; first step {statistics.median(firsts):.3f} ms; steady step (median) "
              f"{statistics.median(steady):.4f} ms", flush=True)
    d, p = (statistics.median(res[k + "_step"]["steady_step_ms_median"]) for k in ("ddim", "dpm_uniform"))
    res["dpm_over_ddim_steady_step"] = round(p / d, 4)
    print(f"steady DPM step / DDIM step = {p / d:.4f} ({(p - d) * 1e3:+.1f} us)")
    for name, S in (("ddim", 50), ("dpm_uniform", 25), ("dpm_logsnr", 20)):
        clip_ms(samplers[name], S)                     # the VAE's packed weights, the schedule's tables
        ms = [clip_ms(samplers[name], S) for _ in range(args.samples)]
        res[f"clip_ms_{name}_S{S}"] = dict(entries=int(samplers[name].ddim_timesteps.shape[0]), ms=[round(v, 2) for v in ms])
        print(f"clip latency {name} S={S} ({samplers[name].ddim_timesteps.shape[0]} entries): median {statistics.median(ms):.2f} ms",
              flush=True)
    res["graph_keys"] = sorted({str(k[0]) for k in model._engine._graphs if isinstance(k, tuple) and k})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
