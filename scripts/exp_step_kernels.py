"""What one launch of a sampler-step kernel (csrc/sampler_step.hip) costs: each entry point 200 times in one captured graph (the
protocol of scripts/exp_edit_step.py's blend figure), the replay timed by device events and divided by 200, twenty replays; config
2's latent [rows, 4, 10, 32, 32] with 2 conditioning frames, b = 1 with the CFG pair and 4 slots.  Prints one JSON line: (median,
min, max) in microseconds per entry point.  The library is the one SEER_HIP_LIB names, else the tree's: run it once per library,
alternating, to compare two builds (profiles/step_refactor.md keeps such a run).  `python scripts/exp_step_kernels.py`"""
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from seervideoldm_amd import DDIMSampler, _lib, ops  # noqa: E402

dev = torch.device("cuda")
C, FP, F1, H = 4, 10, 2, 32


def timed(fn, n=200, rounds=20):
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(n):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        e.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(e) * 1e3 / n)
    return round(statistics.median(times), 3), round(min(times), 3), round(max(times), 3)


def main():
    g = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(s, generator=g).to(dev)
    out = {"lib": str(_lib.lib_path())}
    tabs = {}
    for eta in (0., 0.5):
        smp = DDIMSampler(dev)
        smp.make_schedule(30, ddim_eta=eta, verbose=False)
        tabs[eta] = (smp.ddim_coef, smp._t_table)
    n = tabs[0.][0].shape[0]
    # the batch forms, b = 1 with the CFG pair; step[1] is only read, so the index stays 15 launch after launch
    x, xp, pred, eps, x0 = rn(1, C, FP, H, H), rn(1, C, FP, H, H), rn(1, C, FP, H, H), rn(2, C, F1 + FP, H, H), rn(1, C, F1, H, H)
    step = torch.tensor([15, 15], dtype=torch.int32, device=dev)
    seeds = ops.seed_words([1234]).to(dev)
    kw = dict(cfg=True, scale=7.5, cond_f=F1, x_prev=xp, pred_x0=pred)
    out["cfg_ddim_step_dev eta 0"] = timed(lambda: ops.cfg_ddim_step_dev(eps, x, tabs[0.][0], step, **kw))
    out["cfg_ddim_step_rng_dev eta 0"] = timed(lambda: ops.cfg_ddim_step_rng_dev(eps, x, tabs[0.][0], step, seeds, temperature=1., **kw))
    out["cfg_ddim_step_rng_dev eta 0.5"] = timed(lambda: ops.cfg_ddim_step_rng_dev(eps, x, tabs[.5][0], step, seeds, temperature=1., **kw))
    # the slot forms, 4 slots; begin reads step[s][0] and writes step[s][1], the update the other way round: the index stays
    S = 4
    xs, xps, preds, epss, x0s = rn(S, C, FP, H, H), rn(S, C, FP, H, H), rn(S, C, FP, H, H), rn(2 * S, C, F1 + FP, H, H), rn(S, C, F1, H, H)
    xprov, ring = rn(S, C, FP, H, H), rn(S, 3, C, FP, H, H)
    steps = torch.tensor([[15, 15]] * S, dtype=torch.int32, device=dev)
    state = torch.zeros((S, 8), dtype=torch.int32, device=dev)
    scale = torch.full((S,), 7.5, device=dev)
    temp = torch.ones((S,), device=dev)
    seedS = ops.seed_words([1234, 5, 6, 7]).to(dev)
    sample = torch.empty((2 * S, C, F1 + FP, H, H), device=dev)
    t_out = torch.zeros((2 * S,), dtype=torch.int64, device=dev)
    coefs = {eta: tabs[eta][0][None].repeat(S, 1, 1).contiguous() for eta in tabs}
    ttab = tabs[0.][1][None].repeat(S, 1).contiguous()
    out["slot_step_begin"] = timed(lambda: ops.slot_step_begin(x0s, xs, ttab, steps, 2, sample, t_out))
    out["slot_plms_step_begin"] = timed(lambda: ops.slot_plms_step_begin(x0s, xs, xprov, ttab, steps, state, 2, sample, t_out))
    skw = dict(cond_f=F1, x_prev=xps, pred_x0=preds)
    out["slot_cfg_ddim_step"] = timed(lambda: ops.slot_cfg_ddim_step(epss, xs, scale, coefs[0.], steps, **skw))
    out["slot_cfg_ddim_step_rng eta 0.5"] = timed(lambda: ops.slot_cfg_ddim_step_rng(epss, xs, scale, coefs[.5], steps, seedS, temp, **skw))
    out["slot_cfg_plms_step phase 0"] = timed(lambda: ops.slot_cfg_plms_step(epss, xs, scale, coefs[0.], steps, state, ring, xprov, **skw))
    assert n > 15
    print(json.dumps(out))


if __name__ == "__main__":
    main()
