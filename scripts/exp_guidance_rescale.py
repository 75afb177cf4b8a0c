"""What the guidance-rescale node (two launches, seer_cfg_rescale / seer_slot_cfg_rescale) costs a captured step at BASELINE config 2
(bench.py's workload: CFG batch 2 x 12 frames x 32x32 latent, full-width SeerUNet, synthetic weights, bf16), and whether the default
step moved.  Two loops, the factor phi as the one variable:
    --slots 0   bench.py's own loop: one p_sample_ddim per step on the captured path, a new sample every 50 steps;
    --slots N   a SlotSampler of N slots, every slot running a 50-step DDIM clip of the same workload: N clips are admitted, the step
                is replayed until they finish (the timed window: the step() calls alone), and the next N are admitted.
A round is one 50-step sample under a host clock that ends in a device synchronise.  `--root DIR` imports the package from another
checkout (the parent commit's, built there) so that two commits are timed by the same script in one job, alternating; a parent knows
no factor and is run with --rescale 0.  Usage:
    python scripts/exp_guidance_rescale.py [--root DIR] [--rescale 0.7] [--slots 0|4] [--rounds 3] [--warmup 2]
prints one JSON line: ms per step of every round, their median, min and max, and how the captured keys end."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parents[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=str(HERE))
    ap.add_argument("--rescale", type=float, default=0.0)
    ap.add_argument("--slots", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3, help="timed 50-step samples")
    ap.add_argument("--warmup", type=int, default=2, help="untimed 50-step samples in front of them")
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import bench                                          # (bench.py puts its own directory in front: the package comes from --root)
    sys.path.insert(0, args.root)
    from seervideoldm_amd import DDIMSampler, SeerUNet, SlotSampler, synth
    import seervideoldm_amd
    assert Path(seervideoldm_amd.__file__).resolve().parents[1] == Path(args.root).resolve(), seervideoldm_amd.__file__
    device = torch.device("cuda", 0)
    cfg = dict(synth.SD15_UNET_CFG)
    model = SeerUNet(**cfg, compute_dtype=torch.bfloat16).to(device)
    model.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(cfg), device=device), strict=True)
    model.eval()
    model.use_graph = True
    x_T, x0_emb, c, uc = bench.build_inputs(device)
    w = bench.WORKLOAD
    S, phi = w["ddim_steps"], float(args.rescale)
    factor = dict(guidance_rescale=phi) if phi else {}

    if args.slots:
        f1, Fp, h = w["cond_frames"], w["frames"] - w["cond_frames"], w["latent"]
        smp = SlotSampler(model, args.slots, shape=(4, Fp, h, h), cond_frames=f1, context_shape=(77, 768), device=device,
                          **(dict(rescale=True) if phi else {}))

        def sample():
            for _ in range(args.slots):
                smp.submit(x_T[:1], x0_emb[:1], c[:1], uc[:1], S, w["scale"], **factor)
            torch.cuda.synchronize()
            steps, last = 0, None
            t0 = time.perf_counter()
            while smp.active():
                done = smp.step()
                steps += 1
                last = done[-1][1] if done else last
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3, last
    else:
        sampler = DDIMSampler(device)
        sampler.make_schedule(ddim_num_steps=S, ddim_eta=0.0, verbose=False)
        sampler.static_step_outputs = True
        nidx = len(sampler.ddim_timesteps)

        def sample():
            torch.cuda.synchronize()
            x = x_T
            t0 = time.perf_counter()
            for index in reversed(range(nidx)):
                x = sampler.p_sample_ddim(model, x, c, sampler._t_table[index].expand(w["b"]), index=index, x0_emb=x0_emb,
                                          unconditional_guidance_scale=w["scale"], unconditional_conditioning=uc, **factor)[0]
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / nidx * 1e3, x

    for _ in range(args.warmup):
        sample()
    ms, x = [], None
    for _ in range(args.rounds):
        t, x = sample()
        ms.append(t)
    assert torch.isfinite(x).all()
    keys = [k for k in model._engine._graphs if isinstance(k, tuple) and k and str(k[0]).startswith(("step", "slots"))]
    print(json.dumps(dict(label=args.label or args.root, rescale=phi, slots=args.slots, rounds=args.rounds,
                          ms_per_step=[round(v, 4) for v in ms], median=round(statistics.median(ms), 4), min=round(min(ms), 4),
                          max=round(max(ms), 4), keys=[[str(k[0]), *[str(v) for v in k[-2:]]] for k in keys])))


if __name__ == "__main__":
    main()
