"""What DPM-Solver++ in slots gains, and what its step costs: SlotSampler(dpm=True) at 4 slots against the plain SlotSampler at 4 slots
and against DPMSolverSampler one clip after another.

Workload: BASELINE config 2's clip (SD-v1-5 widths on closed-form weights, 12 frames of which 2 condition, 32x32 latent, bf16, default
mode, captured steps), `--requests` requests (8) at CFG 7.5, every request with its own prompt: DDIM requests run S = 50, DPM-Solver++
requests (2M, the defaults of DPMSolverSampler) S = 25 -- where 2M is on the analytic model what DDIM is at 50 (profiles/dpm_sampler.md;
no claim about trained weights).  Four settings, each with its own model (the engine keeps ONE static context) and warmed with one
request first (step captured):

    SlotSampler(dpm=False), 4 slots, DDIM S = 50       the step as it was before the keyword: same kernels, same graph key
    SlotSampler(dpm=True),  4 slots, DDIM S = 50       the step that carries a sampler per slot, on the same requests
    SlotSampler(dpm=True),  4 slots, 2M S = 25         the queue this feature is for
    DPMSolverSampler, b = 1, 2M S = 25                 one clip after another

Then the settings ALTERNATE in one process, `--repeats` times; a pass is timed on the host clock from the first admission to a device
synchronise after the last clip, so admissions (schedule upload, context and K|V refresh) are inside.  With 8 requests in 4 slots every
slot is full in every step.  Prints markdown (profiles/slot_dpm.md keeps a run): clips/s, ms per replayed step = pass time / replays
of the pass with its spread (max - min over the repeats), and the comparisons.
`python scripts/exp_slot_dpm.py [--requests 8] [--repeats 3]`"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from seervideoldm_amd import SeerUNet, SlotSampler, synth  # noqa: E402
from seervideoldm_amd.dpm import DPMSolverSampler  # noqa: E402

F1, FP, HL, S_DDIM, S_DPM, SCALE, SLOTS = 2, 10, 32, 50, 25, 7.5, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
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
                 c=torch.randn((1, F1 + FP, 77, D), generator=g).to(dev), uc=uc, scale=SCALE, tag=k) for k in range(args.requests)]

    def sequential(m):
        smp = DPMSolverSampler(dev)

        def run(rs):
            out = []
            for r in rs:
                lat, _ = smp.sample(m, S_DPM, batch_size=1, shape=(4, FP, HL, HL), x0_emb=r["x0_emb"], conditioning=r["c"], verbose=False,
                                    cond_frames=F1, unconditional_guidance_scale=r["scale"], unconditional_conditioning=r["uc"], eta=0.,
                                    x_T=r["x_T"], is_3d=True)
                out.append(lat)
            return out, len(rs) * int(smp.dpm_coef.shape[0])
        return run

    def slotted(m, dpm, method, S):
        smp = SlotSampler(m, SLOTS, shape=(4, FP, HL, HL), cond_frames=F1, context_shape=(77, D), device=dev, model_cond_frame=F1,
                          **(dict(dpm=True) if dpm else {}))

        def run(rs):
            rs = [dict(r, S=S, method=method) for r in rs]
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

    plain, carried, queue, solo = (f"SlotSampler(dpm=False), {SLOTS} slots, DDIM S = {S_DDIM}",
                                   f"SlotSampler(dpm=True), {SLOTS} slots, DDIM S = {S_DDIM}",
                                   f"SlotSampler(dpm=True), {SLOTS} slots, 2M S = {S_DPM}",
                                   f"DPMSolverSampler, b = 1, 2M S = {S_DPM}, one clip after another")
    makers = ((plain, lambda m: slotted(m, False, "ddim", S_DDIM)), (carried, lambda m: slotted(m, True, "ddim", S_DDIM)),
              (queue, lambda m: slotted(m, True, "dpmpp", S_DPM)), (solo, sequential))
    settings, taken = {}, {}
    for name, make in makers:
        m = model()
        m.prepare()                                   # the packed weights are the model's, not the step's
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        settings[name] = run = make(m)
        out, _ = run(reqs[:1])                        # warm-up: the step captured, one clip through
        assert torch.isfinite(out[0]).all()
        torch.cuda.synchronize()
        taken[name] = torch.cuda.memory_allocated() - before
    times = {name: [] for name in settings}
    replays = {}
    for _ in range(args.repeats):
        for name, run in settings.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, replays[name] = run(reqs)
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            assert len(out) == len(reqs) and all(torch.isfinite(o).all() for o in out)
    per = {name: [1e3 * t / replays[name] for t in times[name]] for name in settings}           # ms per replay, every repeat
    med = {name: statistics.median(per[name]) for name in settings}
    spread = {name: max(per[name]) - min(per[name]) for name in settings}
    rate = {name: args.requests / statistics.median(times[name]) for name in settings}
    print(f"{torch.cuda.get_device_name(0)}; {args.requests} requests, CFG {SCALE}, {F1} + {FP} frames, {HL}x{HL} latent, bf16, default "
          f"mode, captured steps; {args.repeats} alternated repeats, medians")
    print()
    print("| setting | replays per pass | s per pass, every repeat | median clips/s | median ms per replay | spread of ms per replay |")
    print("|---|---|---|---|---|---|")
    for name in settings:
        print(f"| {name} | {replays[name]} | {', '.join(f'{t:.3f}' for t in times[name])} | {rate[name]:.2f} | {med[name]:.3f} | "
              f"{spread[name]:.3f} |")
    print()
    print(f"the step: dpm=True {med[carried]:.3f} ms on DDIM requests, {med[queue]:.3f} ms on 2M requests, against dpm=False "
          f"{med[plain]:.3f} ms (spread {spread[plain]:.3f} ms): {med[carried] - med[plain]:+.3f} ms and {med[queue] - med[plain]:+.3f} ms")
    print(f"the queue: 2M at S = {S_DPM} in {SLOTS} slots {rate[queue]:.2f} clips/s; {rate[queue] / rate[plain]:.2f}x DDIM at S = {S_DDIM} in "
          f"{SLOTS} slots ({rate[plain]:.2f}), {rate[queue] / rate[solo]:.2f}x 2M at S = {S_DPM} one clip after another ({rate[solo]:.2f})")
    print()
    print("device memory a setting takes beyond its model and packed weights (static buffers, the context's K|V, the captured step): "
          + "; ".join(f"{name}: {taken[name] / 2 ** 20:.0f} MiB" for name in settings))


if __name__ == "__main__":
    main()
