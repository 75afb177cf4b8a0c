"""What step caching (SeerUNet.enable_step_cache) costs and saves at BASELINE config 2 (bench.py's workload: a CFG pair x 12 frames x
32x32 latent, full-width SeerUNet, synthetic weights, bf16), measured on the GPU in one process.  Four modes, one JSON line each:

    --mode step     the captured DDIM step with the cache off: ms per replay (device events around each p_sample_ddim).  `--root DIR`
                    imports the package from another checkout -- the parent commit's, built there -- so that one job times both
                    commits with this script, alternating processes.  A parent knows no step cache: this is the only mode it runs.
    --mode replay   per branch: the full (storing) and the cached captured step, ALTERNATED replay by replay, device events around
                    each; and the cache-off step the same way in the same process.
    --mode chain    whole samples under a host clock that ends in a device synchronise: DDIM S = 50 and DPM-Solver++ S = 25 with the
                    cache off and with interval 2, 3 and 5 (alternated round by round); and the drift on SYNTHETIC weights: the relative
                    L2 between the final latents of a cached and the uncached chain for order 0, 1 and 2 (no quality figure).
    --mode kernels  seer_cache_push and seer_cache_forecast alone at this workload's feature size: us per launch from device events
                    around a train of launches that walks more buffer sets than the memory-side cache holds, the bytes each moves
                    (computed from the shapes) and their share of the HBM peak.

Every figure comes with its spread (min / median / max over the rounds).  No GPU: the script fails, it does not fall back."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parents[1]
HBM_PEAK_GBS = 8000.0        # HBM3E, spec


def spread(v):
    return dict(min=round(min(v), 4), median=round(statistics.median(v), 4), max=round(max(v), 4), n=len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=str(HERE))
    ap.add_argument("--mode", choices=("step", "replay", "chain", "kernels"), required=True)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import bench                                          # (bench.py puts its own directory in front: the package comes from --root)
    sys.path.insert(0, args.root)
    import seervideoldm_amd
    from seervideoldm_amd import DDIMSampler, DPMSolverSampler, SeerUNet, ops, synth
    assert Path(seervideoldm_amd.__file__).resolve().parents[1] == Path(args.root).resolve(), seervideoldm_amd.__file__
    assert torch.cuda.is_available(), "bench_step_cache.py measures on the GPU"
    device = torch.device("cuda", 0)
    w = bench.WORKLOAD
    out = dict(mode=args.mode, label=args.label or args.root)
    rows = 2 * w["b"] * w["frames"] * w["latent"] ** 2

    if args.mode == "kernels":
        n = rows * 320
        sets = 12                                          # 12 x 4 x n x 2 bytes = 755 MB: three times the memory-side cache
        rings = [torch.randn((3, n), device=device).to(torch.bfloat16) for _ in range(sets)]
        xs = [torch.randn((n,), device=device).to(torch.bfloat16) for _ in range(sets)]
        wts = torch.tensor([1.5, -0.5, 0.0], dtype=torch.float32, device=device)
        wts3 = torch.tensor([1.875, -1.25, 0.375], dtype=torch.float32, device=device)

        def train(fn, reps=10):
            us = []
            for r in range(args.warmup + args.rounds):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    for k in range(sets):
                        fn(k)
                b.record()
                torch.cuda.synchronize()
                if r >= args.warmup:
                    us.append(a.elapsed_time(b) * 1e3 / (reps * sets))
            return us
        for name, fn, slots in (("push", lambda k: ops.cache_push(xs[k], rings[k]), 6),
                                ("forecast_2_slots", lambda k: ops.cache_forecast(rings[k], wts, xs[k]), 3),
                                ("forecast_3_slots", lambda k: ops.cache_forecast(rings[k], wts3, xs[k]), 4)):
            us = train(fn)
            nbytes = slots * n * 2                         # push: 3 reads + 3 writes of n 16-bit elements; forecast: its reads + 1 write
            med = statistics.median(us)
            out[name] = dict(us=spread(us), bytes=nbytes, gbs=round(nbytes / med / 1e3, 1),
                             share_of_hbm_peak=round(nbytes / med / 1e3 / HBM_PEAK_GBS, 3))
        out["elements"] = n
        print(json.dumps(out))
        return

    cfg = dict(synth.SD15_UNET_CFG)
    model = SeerUNet(**cfg, compute_dtype=torch.bfloat16).to(device)
    model.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(cfg), device=device), strict=True)
    model.eval()
    model.use_graph = True
    x_T, x0_emb, c, uc = bench.build_inputs(device)
    L = cfg["layers_per_block"]

    if args.mode in ("step", "replay"):
        sampler = DDIMSampler(device)
        sampler.make_schedule(ddim_num_steps=w["ddim_steps"], ddim_eta=0.0, verbose=False)
        sampler.static_step_outputs = True
        nidx = len(sampler.ddim_timesteps)
        state = dict(index=nidx - 1, x=x_T)

        def one(phase=None):
            """one captured p_sample_ddim at the chain's next index -> ms between two device events"""
            pol = getattr(model, "_step_cache", None)
            if pol is not None:
                pol.k = 0 if phase == "full" else 1       # the policy's counter decides the phase of the next evaluation
            i = state["index"]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            state["x"] = sampler.p_sample_ddim(model, state["x"], c, sampler._t_table[i].expand(w["b"]), index=i, x0_emb=x0_emb,
                                               unconditional_guidance_scale=w["scale"], unconditional_conditioning=uc)[0]
            b.record()
            torch.cuda.synchronize()
            state["index"] = i - 1 if i else nidx - 1
            if not i:
                state["x"] = x_T
            return a.elapsed_time(b)

        def timed(phases, n):
            for _ in range(args.warmup * 10):
                for p in phases:
                    one(p)
            ms = {p: [] for p in phases}
            for _ in range(n):
                for p in phases:                           # alternated replay by replay
                    ms[p].append(one(p))
            return {str(p): spread(v) for p, v in ms.items()}
        n = args.rounds * 50
        out["off"] = timed([None], n)["None"]
        if args.mode == "replay":
            for b in range(L + 1):
                model.enable_step_cache(3, b, 1)
                one("full")                                # (captures both graphs; the ring holds a feature from here on)
                out[f"branch_{b}"] = timed(["full", "cached"], n)
            model.disable_step_cache()
            out["off_again"] = timed([None], n)["None"]
        assert torch.isfinite(state["x"]).all()
        print(json.dumps(out))
        return

    # chain
    def sample(cls, S):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lat, _ = cls(device).sample(unet=model, S=S, conditioning=c, batch_size=w["b"], shape=tuple(x_T.shape[1:]), x0_emb=x0_emb,
                                    verbose=False, unconditional_guidance_scale=w["scale"], unconditional_conditioning=uc, eta=0.0,
                                    x_T=x_T, is_3d=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, lat.clone()

    def setting(interval, order=1):
        model.disable_step_cache() if interval is None else model.enable_step_cache(interval, 1, order)
    for name, cls, S in (("ddim_50", DDIMSampler, 50), ("dpmpp_25", DPMSolverSampler, 25)):
        settings = [None, 2, 3, 5]
        ms = {s: [] for s in settings}
        for r in range(args.warmup + args.rounds):
            for s in settings:                             # alternated round by round
                setting(s)
                t, lat = sample(cls, S)
                assert torch.isfinite(lat).all()
                if r >= args.warmup:
                    ms[s].append(t)
        out[name] = {("off" if s is None else f"interval_{s}"): spread(v) for s, v in ms.items()}
        setting(None)
        ref = sample(cls, S)[1]
        drift = {}
        for interval in (2, 3, 5):
            for order in (0, 1, 2):
                setting(interval, order)
                lat = sample(cls, S)[1]
                drift[f"interval_{interval}_order_{order}"] = round(((lat - ref).norm() / ref.norm()).item(), 5)
        out[name + "_drift_rel_l2_synthetic_weights"] = drift
        setting(None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
