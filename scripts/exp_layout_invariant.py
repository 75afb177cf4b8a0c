"""What the layout-invariant mode costs: the replayed UNet step of BASELINE config 2 (SD-v1-5 widths, 12 frames, 32x32 latent) with
the switch off and on, at CFG batch 2 (the bench's workload) and at one CFG half (b = 1, the layout the mode exists for).

Both engines are warmed and captured first; then the two settings ALTERNATE in one process, device events around `--steps` replayed
steps each, `--repeats` times; the table gives every repeat, the median and the spread.  `python scripts/exp_layout_invariant.py
[--steps 50] [--repeats 3]` prints markdown (profiles/layout_invariant.md keeps a run).

`--trace off|on`: ONE setting, warmed and captured, then `--steps` replayed steps at b = 2 and nothing else -- the process to put
behind `rocprofv3 --kernel-trace --stats --` once per setting; the two kernel tables side by side are the per-class launch times."""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from seervideoldm_amd import SeerUNet, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--trace", choices=("off", "on"), default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    cfg = dict(synth.SD15_UNET_CFG)
    sd = synth.synth_state_dict(synth.unet_param_shapes(cfg), device=dev)
    models = {}
    for name, inv in (("off", False), ("on", True)):
        if args.trace not in (None, name):
            continue
        m = SeerUNet(**cfg, layout_invariant=inv).to(dev)
        m.load_state_dict(sd, strict=True)
        m.eval()
        m.use_graph = True
        models[name] = m
    g = torch.Generator().manual_seed(0)
    F = args.frames
    if args.trace:
        m = models[args.trace]
        x = torch.randn((2, 4, F, 32, 32), generator=g).to(dev)
        ctx = torch.randn((2, F, 77, cfg["cross_attention_dim"]), generator=g).to(dev)
        t = torch.full((2,), 501, dtype=torch.long, device=dev)
        with torch.no_grad():
            for _ in range(3 + args.steps):           # eager warm-up, capture, replays
                m(x, t, ctx, cond_frame=2)
        torch.cuda.synchronize()
        print(f"switch {args.trace}: eager warm-up + capture + {1 + args.steps} replayed steps at b = 2")
        return
    print(f"| layout | switch | ms / step per repeat ({args.steps} replayed steps each) | median | spread |")
    print("|---|---|---|---|---|")
    for b in (2, 1):
        x = torch.randn((b, 4, F, 32, 32), generator=g).to(dev)
        ctx = torch.randn((b, F, 77, cfg["cross_attention_dim"]), generator=g).to(dev)
        t = torch.full((b,), 501, dtype=torch.long, device=dev)
        with torch.no_grad():
            for m in models.values():                 # warm both: eager warm-up, capture, two replays
                for _ in range(3):
                    m(x, t, ctx, cond_frame=2)
            torch.cuda.synchronize()
            ms = {k: [] for k in models}
            for _ in range(args.repeats):
                for name, m in models.items():        # alternate the two settings
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.steps):
                        m(x, t, ctx, cond_frame=2)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[name].append(e0.elapsed_time(e1) / args.steps)
        med = {k: statistics.median(v) for k, v in ms.items()}
        for name in models:
            v = ms[name]
            print(f"| b = {b} ({b * F * 1024} rows at the 32x32 level) | {name} | {', '.join(f'{u:.3f}' for u in v)} | {med[name]:.3f} | "
                  f"{max(v) - min(v):.3f} |")
        print(f"| b = {b} | on / off | | {med['on'] / med['off']:.3f} | |")
        eng = models["on"]._engine
        print(f"<!-- b = {b}: invariant engine: {eng.rowchains} row chains, {eng.ln_folded} folded LayerNorms per step -->")


if __name__ == "__main__":
    main()
