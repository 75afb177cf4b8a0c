"""What the v-prediction node costs a captured DDIM step at BASELINE config 2 (bench.py's workload: CFG batch 2 x 12 frames x 32x32
latent, full-width SeerUNet, synthetic weights, bf16), and whether the default step moved.  bench.py's own loop -- one
p_sample_ddim per step on the captured path, a new sample every 50 steps, a host clock around a synchronised window -- with the
sampler's prediction_type as the one variable.  `--root DIR` imports the package from another checkout (the parent commit's, built
there) so that two commits are timed by the same script in the same job, alternating.  Usage:
    python scripts/exp_vpred_step.py [--root DIR] [--prediction epsilon|v_prediction] [--steps 300] [--warmup 60] [--rounds 5]
prints one JSON line: ms per step of every round, their median, min and max."""
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
    ap.add_argument("--prediction", default="epsilon", choices=("epsilon", "v_prediction"))
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import bench                                          # (bench.py puts its own directory in front: the package comes from --root)
    sys.path.insert(0, args.root)
    from seervideoldm_amd import DDIMSampler, SeerUNet, synth
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
    sampler = DDIMSampler(device, **({} if args.prediction == "epsilon" else dict(prediction_type=args.prediction)))
    sampler.make_schedule(ddim_num_steps=w["ddim_steps"], ddim_eta=0.0, verbose=False)
    sampler.static_step_outputs = True
    nidx = len(sampler.ddim_timesteps)

    def run(first, count, x):
        for i in range(first, first + count):
            index = nidx - 1 - (i % nidx)
            x = sampler.p_sample_ddim(model, x_T if i % nidx == 0 else x, c, sampler._t_table[index].expand(w["b"]), index=index,
                                      x0_emb=x0_emb, unconditional_guidance_scale=w["scale"], unconditional_conditioning=uc)[0]
        return x
    x = run(0, args.warmup, x_T)
    torch.cuda.synchronize()
    ms, i0 = [], args.warmup
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        x = run(i0, args.steps, x)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / args.steps * 1e3)
        i0 += args.steps
    assert torch.isfinite(x).all()
    kinds = sorted({k[0] for k in model._engine._graphs if isinstance(k, tuple) and k}, key=str)
    print(json.dumps(dict(label=args.label or args.root, prediction=args.prediction, steps=args.steps, rounds=args.rounds,
                          ms_per_step=[round(v, 4) for v in ms], median=round(statistics.median(ms), 4), min=round(min(ms), 4),
                          max=round(max(ms), 4), captured=kinds,
                          key_tail=[k[-1] for k in model._engine._graphs if isinstance(k, tuple) and k and k[0] == "step"])))


if __name__ == "__main__":
    main()
