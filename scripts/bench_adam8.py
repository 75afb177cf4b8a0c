"""fp32 AdamW (seer_adamw_step) against 8-bit AdamW (seer_adamw8_step) on one MI355X, in one process:
    kernels  both launches alone on flat buffers of the trainer's full size (pu.n + pf.n of a BASELINE config 5 trainer with
             use_8bit_adam=True, about 405 M elements) and of a quarter of it: HIP events around each launch, 10 warm-up launches,
             then 50 timed ones per kernel, the two kernels alternating; the median.  Random data (gradients N(0, 1e-2), a state left
             by three steps on other gradients).  Bytes moved per element by the algorithm: 28 (p read + written, g read, m and v
             read + written, the bf16 copy written) or 18 (the moments as two 1-byte codes; the scales add 16 bytes per 256 elements).
    step     SeerTrainer.step_from_batch(use_graph=True) at config 5 in both modes (scripts/bench_train_from_batch.py's setting):
             host clock around a synchronised block, 5 warm-up + 20 timed steps; optimizer state bytes and peak memory of each.
Usage: python scripts/bench_adam8.py kernels|step|all          (one JSON line per measurement)"""
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from seervideoldm_amd import train_ops  # noqa: E402
from seervideoldm_amd.trainer import SeerTrainer, ddpm_alphas_cumprod  # noqa: E402
from scripts.bench_train import build  # noqa: E402

HP = dict(lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)


def bench_kernels(dev, n, launches=50, warmup=10):
    gen = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn((n,), device=dev, generator=gen)
    g = torch.randn((n,), device=dev, generator=gen) * 1e-2
    pb = torch.empty((n,), device=dev, dtype=torch.bfloat16)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    cm, cv = torch.full((n,), 127, device=dev, dtype=torch.uint8), torch.zeros((n,), device=dev, dtype=torch.uint8)
    am, av = torch.zeros((n // 256,), device=dev), torch.zeros((n // 256,), device=dev)
    ss = train_ops.sumsq(g)
    step = [0]

    def run32():
        train_ops.adamw_step(p, g, m, v, step=step[0], grad_sumsq=ss, max_norm=0.3, p_bf16=pb, **HP)

    def run8():
        train_ops.adamw8_step(p, g, cm, cv, am, av, step=step[0], grad_sumsq=ss, max_norm=0.3, p_bf16=pb, **HP)

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {"fp32": [], "8bit": []}
    for i in range(warmup + launches):
        step[0] += 1
        if i < 3:                                  # the state both kernels start from: three steps on other gradients
            g.normal_(generator=gen).mul_(1e-2)
        for name, fn in (("fp32", run32), ("8bit", run8)):
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[name].append(ev[0].elapsed_time(ev[1]))
    out = {"what": "optimizer launch alone", "device": torch.cuda.get_device_name(0), "n": n, "launches": launches}
    for name, bpe, state in (("fp32", 28, 8 * n), ("8bit", 18, 2 * n + 8 * (n // 256))):
        ms = statistics.median(times[name])
        out[name] = {"median_ms": ms, "min_ms": min(times[name]), "max_ms": max(times[name]), "bytes_per_element": bpe,
                     "bytes_moved": bpe * n, "gb_per_s": bpe * n / (ms * 1e-3) / 1e9, "state_bytes": state}
    out["time_8bit_over_fp32"] = out["8bit"]["median_ms"] / out["fp32"]["median_ms"]
    return out


def bench_step(dev, unet, fst, steps=20, warmup=5):
    from scripts.bench_train_from_batch import B, F1, F2, PIX, frozen, timed
    g = torch.Generator().manual_seed(1)
    video = (torch.rand((B, 3, F1 + F2, PIX, PIX), generator=g) * 2 - 1).to(dev)
    ids = torch.randint(0, 49408, (B, 77), generator=g)
    mask = torch.ones((B, 77), dtype=torch.int64)
    acp = ddpm_alphas_cumprod().to(dev)
    vae, clip = frozen(dev)
    fst.set_numframe(F1 + F2)
    out, n8 = [], None
    for mode in (False, True):
        torch.cuda.reset_peak_memory_stats()
        tr = SeerTrainer(unet, fst, lr=1e-5, max_grad_norm=0.3, use_8bit_adam=mode)
        fn = lambda: tr.step_from_batch(video, ids, mask, vae=vae, text_encoder=clip, cond_frames=F1, alphas_cumprod=acp, use_graph=True)
        ms = timed(fn, steps, warmup)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        opt = []
        for _ in range(10):                        # the optimizer part alone (clip norm + both segments), on the step's gradients
            ev[0].record()
            tr.optimizer_step()
            ev[1].record()
            torch.cuda.synchronize()
            opt.append(ev[0].elapsed_time(ev[1]))
        out.append({"what": "step_from_batch, BASELINE config 5", "use_8bit_adam": mode, "ms_per_step": ms,
                    "optimizer_step_median_ms": statistics.median(opt), "loss_last": float(fn()), "steps": steps, "warmup": warmup,
                    "hipgraph": not getattr(tr, "_graph_broken", False), "elements": tr.pu.n + tr.pf.n,
                    "optimizer_state_bytes": tr.optimizer_state_bytes(), "peak_mem_gb": torch.cuda.max_memory_allocated() / 2 ** 30,
                    "device": torch.cuda.get_device_name(0)})
        if mode:
            n8 = tr.pu.n + tr.pf.n
        del tr, fn
        torch.cuda.empty_cache()
    return out, n8


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    dev = torch.device("cuda:0")
    t0 = time.time()
    unet, fst = build(dev)
    n = None
    if mode in ("step", "all"):
        res, n = bench_step(dev, unet, fst)
        for r in res:
            print(json.dumps(r), flush=True)
    if mode in ("kernels", "all"):
        if n is None:
            fst.set_numframe(14)
            tr = SeerTrainer(unet, fst, use_8bit_adam=True)
            n = tr.pu.n + tr.pf.n
            del tr
        del unet, fst
        torch.cuda.empty_cache()
        for size in (n, n // 4 // 256 * 256):
            print(json.dumps(bench_kernels(dev, size)), flush=True)
    print(json.dumps({"wall_s": time.time() - t0}))


if __name__ == "__main__":
    main()
