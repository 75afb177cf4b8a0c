"""The exponential moving average inside the AdamW launch (seer_adamw_ema_step, seer_adamw8_ema_step) against keeping it beside the
step with torch operations, on one MI355X, in one process:
    kernels  on flat buffers of the trainer's full size (pu.n + pf.n of a BASELINE config 5 trainer with use_8bit_adam=True, about
             405 M elements) and of a small one (1 M elements: every buffer fits the memory-side cache), for both optimizer modes:
               (a) the plain step                                   28 / 18 bytes per element (scripts/bench_adam8.py's accounting)
               (b) the _ema step                                    (a) + 8: ema read, ema written
               (c) the plain step, then ema.sub_(omd * (ema - p))   (a) + 32: three passes (12 + 8 + 12 bytes per element)
             HIP events around each, 5 warm-up rounds, then 30 timed ones, the variants alternating inside a round; the median.
             "warm": a launch follows the previous one directly; "cold": 1 GiB is written before every timed launch, so nothing of the
             buffers is left in the 256 MB memory-side cache (at the full size the buffers do not fit it either way).
    step     SeerTrainer.step_from_batch(use_graph=True) at config 5 without and with use_ema (scripts/bench_adam8.py's setting):
             host clock around a synchronised block, 5 warm-up + 20 timed steps; the optimizer part alone; the bytes of the average.
    train    scripts/bench_train.py's own measurement (time_train: forward_backward(use_graph=True) + optimizer_step on synthetic
             latents at config 5, HIP events, 3 warm-up + 20 timed steps) without and with use_ema, three rounds, alternating; that
             script is not edited: its SeerTrainer is called with use_ema=True added.
Usage: python scripts/bench_ema.py kernels|step|train|all [--n ELEMENTS]          (one JSON line per measurement)"""
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from seervideoldm_amd import train_ops  # noqa: E402
from seervideoldm_amd.trainer import SeerTrainer, ddpm_alphas_cumprod, ema_one_minus_decay  # noqa: E402
from scripts.bench_train import build  # noqa: E402

HP = dict(lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
SMALL_N = 1 << 20
BYTES = {"a": 28, "b": 36, "c": 60, "a8": 18, "b8": 26, "c8": 50}


def bench_kernels(dev, n, rounds=30, warmup=5):
    gen = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn((n,), device=dev, generator=gen)
    g = torch.randn((n,), device=dev, generator=gen) * 1e-2
    pb = torch.empty((n,), device=dev, dtype=torch.bfloat16)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    cm, cv = torch.full((n,), 127, device=dev, dtype=torch.uint8), torch.zeros((n,), device=dev, dtype=torch.uint8)
    am, av = torch.zeros((n // 256,), device=dev), torch.zeros((n // 256,), device=dev)
    ema = p.clone()
    ss = train_ops.sumsq(g)
    flush = torch.empty((1 << 28,), device=dev)                    # 1 GiB
    omd = ema_one_minus_decay(0.9999, 10 ** 6, True)
    step = [0]
    kw = lambda: dict(step=step[0], grad_sumsq=ss, max_norm=0.3, p_bf16=pb, **HP)

    def torch_ema():
        ema.sub_(omd * (ema - p))

    def c32():
        train_ops.adamw_step(p, g, m, v, **kw())
        torch_ema()

    def c8():
        train_ops.adamw8_step(p, g, cm, cv, am, av, **kw())
        torch_ema()

    variants = (("a", lambda: train_ops.adamw_step(p, g, m, v, **kw())),
                ("b", lambda: train_ops.adamw_ema_step(p, g, m, v, ema, one_minus_decay=omd, **kw())),
                ("c", c32),
                ("a8", lambda: train_ops.adamw8_step(p, g, cm, cv, am, av, **kw())),
                ("b8", lambda: train_ops.adamw8_ema_step(p, g, cm, cv, am, av, ema, one_minus_decay=omd, **kw())),
                ("c8", c8))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = {"what": "optimizer launch alone, with and without the average", "device": torch.cuda.get_device_name(0), "n": n,
           "rounds": rounds, "one_minus_decay": omd}
    for cache in ("warm", "cold"):
        times = {name: [] for name, _ in variants}
        for i in range(warmup + rounds):
            step[0] += 1
            for name, fn in variants:
                if cache == "cold":
                    flush.fill_(float(i))
                ev[0].record()
                fn()
                ev[1].record()
                torch.cuda.synchronize()
                if i >= warmup:
                    times[name].append(ev[0].elapsed_time(ev[1]))
        res = {}
        for name, _ in variants:
            ms = statistics.median(times[name])
            res[name] = {"median_ms": ms, "min_ms": min(times[name]), "max_ms": max(times[name]), "bytes_per_element": BYTES[name],
                         "gb_per_s": BYTES[name] * n / (ms * 1e-3) / 1e9}
        for a, b, c in (("a", "b", "c"), ("a8", "b8", "c8")):
            per = lambda x, y: (res[x]["median_ms"] - res[y]["median_ms"]) * 1e-3 / n       # seconds per element
            bw = BYTES[a] * n / (res[a]["median_ms"] * 1e-3)                                # the plain launch's bytes per second
            res[f"{b}-{a}"] = {"ms": res[b]["median_ms"] - res[a]["median_ms"], "bytes_per_element_at_plain_rate": per(b, a) * bw}
            res[f"{c}-{a}"] = {"ms": res[c]["median_ms"] - res[a]["median_ms"], "bytes_per_element_at_plain_rate": per(c, a) * bw}
        out[cache] = res
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
    out = []
    for use_ema in (False, True, False, True):             # twice each, alternating: the spread of a repetition
        torch.cuda.reset_peak_memory_stats()
        tr = SeerTrainer(unet, fst, lr=1e-5, max_grad_norm=0.3, use_ema=use_ema)
        fn = lambda: tr.step_from_batch(video, ids, mask, vae=vae, text_encoder=clip, cond_frames=F1, alphas_cumprod=acp, use_graph=True)
        ms = timed(fn, steps, warmup)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        opt = []
        for _ in range(10):                                # the optimizer part alone (clip norm + both segments), on the step's gradients
            ev[0].record()
            tr.optimizer_step()
            ev[1].record()
            torch.cuda.synchronize()
            opt.append(ev[0].elapsed_time(ev[1]))
        out.append({"what": "step_from_batch, BASELINE config 5", "use_ema": use_ema, "ms_per_step": ms,
                    "optimizer_step_median_ms": statistics.median(opt), "loss_last": float(fn()), "steps": steps, "warmup": warmup,
                    "hipgraph": not getattr(tr, "_graph_broken", False), "elements": tr.pu.n + tr.pf.n,
                    "ema_state_bytes": tr.ema_state_bytes(), "ema_num_updates": tr.ema_num_updates,
                    "peak_mem_gb": torch.cuda.max_memory_allocated() / 2 ** 30, "device": torch.cuda.get_device_name(0)})
        del tr, fn
        torch.cuda.empty_cache()
    return out


def bench_train(dev, unet, fst, rounds=3, steps=20):
    import functools
    from scripts import bench_train as bt
    plain, out = bt.SeerTrainer, []
    try:
        for r in range(rounds):
            for use_ema in (False, True):
                bt.SeerTrainer = functools.partial(plain, use_ema=True) if use_ema else plain
                res = bt.time_train(dev, steps=steps, warmup=3, unet=unet, fst=fst)
                out.append({"what": "scripts/bench_train.py time_train, BASELINE config 5", "round": r, "use_ema": use_ema, **res})
                torch.cuda.empty_cache()
    finally:
        bt.SeerTrainer = plain
    return out


def main():
    args = sys.argv[1:]
    n = None
    if "--n" in args:
        i = args.index("--n")
        n = int(args[i + 1]) // 256 * 256
        del args[i:i + 2]
    mode = args[0] if args else "all"
    dev = torch.device("cuda:0")
    t0 = time.time()
    unet = fst = None
    if mode in ("step", "train", "all") or n is None:
        unet, fst = build(dev)
    if mode in ("train", "all"):
        for r in bench_train(dev, unet, fst):
            print(json.dumps(r), flush=True)
    if mode in ("step", "all"):
        for r in bench_step(dev, unet, fst):
            print(json.dumps(r), flush=True)
    if mode in ("kernels", "all"):
        if n is None:
            fst.set_numframe(14)
            tr = SeerTrainer(unet, fst, use_8bit_adam=True)
            n = tr.pu.n + tr.pf.n
            del tr
        del unet, fst
        torch.cuda.empty_cache()
        for size in (n, SMALL_N):
            print(json.dumps(bench_kernels(dev, size)), flush=True)
    print(json.dumps({"wall_s": time.time() - t0}))


if __name__ == "__main__":
    main()
