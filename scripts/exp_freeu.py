"""What FreeU (SeerUNet.enable_freeu: six seer_freeu launches and the statistics passes of the six norm1s behind them) costs a captured
step at BASELINE config 2 (bench.py's workload: CFG batch 2 x 12 frames x 32x32 latent, full-width SeerUNet, synthetic weights, bf16),
and whether the default step moved.  bench.py's own loop: one p_sample_ddim per step on the captured path, a round is one 50-step
sample under a host clock that ends in a device synchronise.  `--root DIR` imports the package from another checkout (the parent
commit's, built there) so that two commits are timed by the same script in one job, alternating; a parent knows no FreeU and is run
without --freeu.  Usage:
    python scripts/exp_freeu.py [--root DIR] [--freeu 0.9,0.2,1.2,1.4] [--rounds 3] [--warmup 2] [--steps-only N]
prints one JSON line: ms per step of every round, their median, min and max, and how the captured keys end.  --steps-only N: N steps
after the warm-up and nothing else (the run to put under rocprofv3 --kernel-trace --stats)."""
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
    ap.add_argument("--freeu", default="", help="s1,s2,b1,b2")
    ap.add_argument("--rounds", type=int, default=3, help="timed 50-step samples")
    ap.add_argument("--warmup", type=int, default=2, help="untimed 50-step samples in front of them")
    ap.add_argument("--steps-only", type=int, default=0)
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
    if args.freeu:
        model.enable_freeu(*(float(v) for v in args.freeu.split(",")))
    x_T, x0_emb, c, uc = bench.build_inputs(device)
    w = bench.WORKLOAD
    S = w["ddim_steps"]
    sampler = DDIMSampler(device)
    sampler.make_schedule(ddim_num_steps=S, ddim_eta=0.0, verbose=False)
    sampler.static_step_outputs = True
    nidx = len(sampler.ddim_timesteps)

    def sample(n=nidx):
        torch.cuda.synchronize()
        x = x_T
        t0 = time.perf_counter()
        for index in list(reversed(range(nidx)))[:n]:
            x = sampler.p_sample_ddim(model, x, c, sampler._t_table[index].expand(w["b"]), index=index, x0_emb=x0_emb,
                                      unconditional_guidance_scale=w["scale"], unconditional_conditioning=uc)[0]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, x

    for _ in range(args.warmup):
        sample()
    if args.steps_only:
        t, x = sample(args.steps_only)
        assert torch.isfinite(x).all()
        print(json.dumps(dict(label=args.label or args.root, freeu=args.freeu, steps=args.steps_only, ms_per_step=round(t, 4))))
        return
    ms, x = [], None
    for _ in range(args.rounds):
        t, x = sample()
        ms.append(t)
    assert torch.isfinite(x).all()
    keys = [k for k in model._engine._graphs if isinstance(k, tuple) and k and str(k[0]).startswith("step")]
    print(json.dumps(dict(label=args.label or args.root, freeu=args.freeu, rounds=args.rounds,
                          ms_per_step=[round(v, 4) for v in ms], median=round(statistics.median(ms), 4), min=round(min(ms), 4),
                          max=round(max(ms), 4), keys=[[str(k[0]), *[str(v) for v in k[-2:]]] for k in keys])))


if __name__ == "__main__":
    main()
