"""What continuous batching gains: a queue of clips through DDIMSampler one after another at b = 1 (the only way before SlotSampler)
against the same queue through SlotSampler with 2 and with 4 slots.

Workload: BASELINE config 2's clip (SD-v1-5 widths on closed-form weights, 12 frames of which 2 condition, 32x32 latent, bf16, default
mode, captured steps), `--requests` requests (8) of S = 30 (31 schedule entries) at CFG 7.5, every request with its own prompt.
Every setting has its own model (the engine keeps ONE static context: settings that took turns on one engine would re-capture at
every turn) and is warmed with one request first (step captured; the device memory that takes is reported).  Then the settings ALTERNATE in one process,
`--repeats` times; a pass is timed on the host clock from the first admission to a device synchronise after the last clip, so
admissions (schedule upload, context and K|V refresh) are inside.  Prints markdown (profiles/slot_sampler.md keeps a run):
clips/s and ms per replayed step = pass time / replays of the pass.  `python scripts/exp_slot_sampler.py [--requests 8] [--repeats 3]`

`--method plms` measures the step that carries a sampler per slot instead (profiles/slot_plms.md keeps a run), at 4 slots: the
plms=True step against the plms=False step with DDIM requests in both, and a PLMS queue against PLMSSampler one clip after another
(S steps are S + 1 model evaluations either way: "replays" counts evaluations there)."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from seervideoldm_amd import DDIMSampler, PLMSSampler, SeerUNet, SlotSampler, synth  # noqa: E402

F1, FP, HL, S, SCALE = 2, 10, 32, 30, 7.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--method", choices=("ddim", "plms"), default="ddim")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda")
    cfg = dict(synth.SD15_UNET_CFG)
    D = cfg["cross_attention_dim"]
    sd = synth.synth_state_dict(synth.unet_param_shapes(cfg), device=dev)

    def model():
        m = SeerUNet(**cfg).to(dev)
        m.load_state_dict(sd, strict=True)
        m.eval()
        m.use_graph = True
        return m

    g = torch.Generator().manual_seed(0)
    uc = torch.randn((1, 1, 77, D), generator=g).expand(-1, F1 + FP, -1, -1).contiguous().to(dev)
    reqs = [dict(x_T=torch.randn((1, 4, FP, HL, HL), generator=g).to(dev),
                 x0_emb=(torch.randn((1, 4, F1, HL, HL), generator=g) * 0.18215 * 5).to(dev),
                 c=torch.randn((1, F1 + FP, 77, D), generator=g).to(dev), uc=uc, S=S, scale=SCALE, tag=k) for k in range(args.requests)]

    def sequential(m, cls=DDIMSampler):
        smp = cls(dev)

        def run(rs):
            out = []
            for r in rs:
                lat, _ = smp.sample(m, r["S"], batch_size=1, shape=(4, FP, HL, HL), x0_emb=r["x0_emb"], conditioning=r["c"], verbose=False,
                                    cond_frames=F1, unconditional_guidance_scale=r["scale"], unconditional_conditioning=r["uc"], eta=0.,
                                    x_T=r["x_T"], is_3d=True)
                out.append(lat)
            return out, len(rs) * (int(smp.ddim_coef.shape[0]) + (cls is PLMSSampler))
        return run

    def slotted(m, slots, plms=False, method="ddim"):
        smp = SlotSampler(m, slots, shape=(4, FP, HL, HL), cond_frames=F1, context_shape=(77, D), device=dev, model_cond_frame=F1,
                          plms=plms)

        def run(rs):
            rs = [dict(r, method=method) for r in rs]
            replays, step = [0], smp.step

            def counted():
                replays[0] += 1
                return step()
            smp.step = counted
            try:
                out = [lat for _, lat in smp.run(iter(rs))]
            finally:
                smp.step = step
            return out, replays[0]
        return run

    settings, taken = {}, {}
    makers = (("DDIMSampler, b = 1, one clip after another", sequential), ("SlotSampler, 2 slots", lambda m: slotted(m, 2)),
              ("SlotSampler, 4 slots", lambda m: slotted(m, 4)))
    if args.method == "plms":
        makers = (("PLMSSampler, b = 1, one clip after another", lambda m: sequential(m, PLMSSampler)),
                  ("SlotSampler(plms=True), 4 slots, PLMS requests", lambda m: slotted(m, 4, True, "plms")),
                  ("SlotSampler(plms=False), 4 slots, DDIM requests", lambda m: slotted(m, 4)),
                  ("SlotSampler(plms=True), 4 slots, DDIM requests", lambda m: slotted(m, 4, True, "ddim")))
    for name, make in makers:
        m = model()
        m.prepare()                                   # the packed weights are the model's, not the step's
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        settings[name] = run = make(m)
        out, _ = run(reqs[:1])                        # warm-up: the step captured, one clip through
        assert torch.isfinite(out[0]).all()
        torch.cuda.synchronize()
        taken[name] = torch.cuda.memory_allocated() - before      # static buffers, K|V of the context, the captured step's pool
    times = {name: [] for name in settings}
    replays = {}
    for _ in range(args.repeats):
        for name, run in settings.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, replays[name] = run(reqs)
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            assert len(out) == len(reqs)
    base = statistics.median(times[next(iter(settings))])
    print(f"{torch.cuda.get_device_name(0)}; {args.requests} requests of S = {S} ({replays[next(iter(settings))] // args.requests} schedule "
          f"{'entries' if args.method == 'ddim' else 'entries + 1 = evaluations of a PLMS clip'}), CFG {SCALE}, {F1} + {FP} frames, "
          f"{HL}x{HL} latent, bf16, default mode, captured steps; {args.repeats} alternated repeats")
    print()
    print("| setting | replays per pass | s per pass, every repeat | median clips/s | median ms per replay | clips/s against b = 1 |")
    print("|---|---|---|---|---|---|")
    for name in settings:
        med = statistics.median(times[name])
        print(f"| {name} | {replays[name]} | {', '.join(f'{t:.3f}' for t in times[name])} | {args.requests / med:.2f} | "
              f"{1e3 * med / replays[name]:.2f} | {base / med:.2f}x |")
    print()
    print("device memory a setting takes beyond its model and packed weights (static buffers, the context's K|V, the captured step): "
          + "; ".join(f"{name}: {taken[name] / 2 ** 20:.0f} MiB" for name in settings))


if __name__ == "__main__":
    main()
