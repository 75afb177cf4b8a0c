"""DPMSolverSampler on a real MI355X: the fused CFG + DPM-Solver++ kernel against float64 (tests/dpm_ref.py), its refusals, its
device-counter form against the host-index form bit for bit over whole chains, the sampler on the mini UNet against the restatement
over the oracle on the CPU, the captured step against the launches, the solver on the analytic model, decode, and a frame-sharded
two-process run."""
import os
import sys

import pytest
import torch

from oracle import seer_oracle as O
from seervideoldm_amd import DDIMSampler, DPMSolverSampler, SeerUNet, _lib, ops, synth
from tests import dpm_ref as R
from tests import plms_oracle as P
from tests.test_dist_gpu import CFG_MINI, ROOT, _backend, _host_staged_gathers, _spawn
from tests.test_dpm_host import refusal_cases

pytestmark = pytest.mark.gpu

_cache = {}


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _rel(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).norm() / ref.norm()).item()


def _model(device):
    if "mini" not in _cache:
        sd = synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI))
        m = SeerUNet(**CFG_MINI)
        m.load_state_dict(sd, strict=True)
        _cache["mini"] = (CFG_MINI, sd, m.to(device).eval())
    return _cache["mini"]


def _combined(eps, b, cfg, scale, cond_f):
    e = eps.double().cpu()[:, :, cond_f:]
    return e[:b] + scale * (e[b:] - e[:b]) if cfg else e


def _fenced(shape, device, pad=64):
    """a NaN buffer with an output of `shape` in its middle -> (the output view, the whole buffer)"""
    n = 1
    for v in shape:
        n *= v
    whole = torch.full((n + 2 * pad,), float("nan"), device=device)
    return whole[pad:pad + n].view(shape), whole


def _fence_intact(whole, pad=64):
    return bool(torch.isnan(whole[:pad]).all() and torch.isnan(whole[-pad:]).all())


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("cond_f", [0, 2])
@pytest.mark.parametrize("cfg", [True, False])
@pytest.mark.parametrize("order", [1, 2])
def test_dpm_kernel_matches_float64(device, order, cfg, cond_f, b):
    """b * 4 * 3 * 96 = 1152 or 2304 elements: more than one block of 256, a ragged last one with b = 1 ... 1e-6 is PLMS's bound for
    the same kind of fp32 elementwise kernel"""
    smp = DPMSolverSampler(device)
    smp.make_schedule(10, verbose=False)
    C, Fp, h, w = 4, 3, 8, 12
    eps = _randn(((2 if cfg else 1) * b, C, Fp + cond_f, h, w), 1).to(device)
    x = _randn((b, C, Fp, h, w), 2).to(device)
    d_prev = _randn(x.shape, 3).to(device) if order == 2 else torch.full(x.shape, float("nan"), device=device)
    index, kw = 6, dict(cfg=cfg, scale=7.5, cond_f=cond_f)
    (x_prev, wx), (pred, wp) = _fenced(x.shape, device), _fenced(x.shape, device)
    rx, rp = ops.cfg_dpm_step(eps, x, smp.dpm_coef, index, order, d_prev=d_prev, x_prev=x_prev, pred_x0=pred, **kw)
    assert rx is x_prev and rp is pred and _fence_intact(wx) and _fence_intact(wp)
    want_x, want_d = R.step64(_combined(eps, b, cfg, 7.5, cond_f), x.cpu(), smp.ddim_alphas, smp.ddim_alphas_prev, index, order,
                              d_prev.cpu())
    for got, want, what in ((x_prev, want_x, "x_prev"), (pred, want_d, "pred_x0")):
        assert torch.isfinite(got).all(), what           # at order 1 the NaN in d_prev was never read
        rel = _rel(got, want)
        assert rel <= 1e-6, (what, rel)
    # x_prev aliasing x and pred_x0 aliasing d_prev: the same bits
    xa, da = x.clone(), d_prev.clone()
    x2, p2 = ops.cfg_dpm_step(eps, xa, smp.dpm_coef, index, order, d_prev=da, x_prev=xa, pred_x0=da, **kw)
    assert x2 is xa and p2 is da and torch.equal(xa, x_prev) and torch.equal(da, pred)
    # without pred_x0 the latent is the same, and a fresh pair of outputs too
    x3, p3 = ops.cfg_dpm_step(eps, x, smp.dpm_coef, index, order, d_prev=d_prev, want_pred_x0=False, **kw)
    assert p3 is None and torch.equal(x3, x_prev)
    if order == 1:                                       # first order is the eta = 0 DDIM step
        dx, dp = ops.cfg_ddim_step(eps, x, smp.ddim_coef, index, **kw)
        assert _rel(x_prev, dx) <= 1e-6 and _rel(pred, dp) <= 1e-6
        x4, _ = ops.cfg_dpm_step(eps, x, smp.dpm_coef, index, 1, **kw)               # d_prev = NULL at order 1
        assert torch.equal(x4, x_prev)


def test_dpm_entry_points_refuse_bad_arguments_and_launch_nothing(device):
    """real, aligned buffers: a refused call returns SEER_EINVAL and leaves every buffer as it was"""
    lib = _lib.load()
    buf = torch.full((4096,), float("nan"), device=device)
    words = torch.full((8,), -7, dtype=torch.int32, device=device)
    n = 0
    for fn, args, why in refusal_cases(buf.data_ptr(), words.data_ptr()):
        assert getattr(lib, fn)(*args, None) == -22, (fn, why)
        n += 1
    torch.cuda.synchronize()
    assert n >= 45 and torch.isnan(buf).all() and bool((words == -7).all())
    smp = DPMSolverSampler(device)
    smp.make_schedule(10, verbose=False)
    x, e = torch.zeros((1, 4, 3, 8, 12), device=device), torch.zeros((1, 4, 3, 8, 12), device=device)
    for args in ((10, 1), (-1, 1), (1, 0), (1, 3), (1, 2)):                          # the last: order 2 without d_prev
        with pytest.raises(ValueError):
            ops.cfg_dpm_step(e, x, smp.dpm_coef, *args, cfg=False, scale=1.0, cond_f=0)


# ---- 2. the device-counter form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lower_order_final", [True, False])
@pytest.mark.parametrize("S", [10, 20])
def test_device_counter_chain_equals_host_index_kernel(device, S, lower_order_final):
    """first order, then second, then a first- or second-order end; the index and history words read back after every step"""
    smp = DPMSolverSampler(device, lower_order_final=lower_order_final)
    smp.make_schedule(S, verbose=False)
    n = smp.dpm_coef.shape[0]
    assert n == S
    b, C, Fp, cond_f, h, w = 2, 4, 3, 1, 8, 12
    eps_seq = [_randn((2 * b, C, Fp + cond_f, h, w), 100 + k).to(device) for k in range(n)]
    x_T = _randn((b, C, Fp, h, w), 99).to(device)
    kw = dict(cfg=True, scale=7.5, cond_f=cond_f)
    x, d_prev, want, orders = x_T, None, [], []
    for k in range(n):
        index = n - 1 - k
        orders.append(smp.step_order(index, d_prev is not None))
        x, d_prev = ops.cfg_dpm_step(eps_seq[k], x, smp.dpm_coef, index, orders[-1], d_prev=d_prev, **kw)
        want.append((x, d_prev))
    final_first = lower_order_final and n < 15
    assert orders == [1] + [2] * (n - 2) + [1 if final_first else 2]
    # a table with more rows than the schedule, as the captured step's: the rows beyond are zero
    table = torch.zeros((64, ops.DPM_ROW_WORDS), device=device)
    table[:n] = smp.dpm_coef
    step = torch.tensor([n - 1, -5], dtype=torch.int32, device=device)
    state = torch.tensor([0, 0, 2, int(final_first)], dtype=torch.int32, device=device)
    xd, hist = x_T.clone(), torch.full(x_T.shape, float("nan"), device=device)       # stale history: never read while not valid
    sample, t_out = torch.empty((b, C, Fp, h, w), device=device), torch.empty((b,), dtype=torch.long, device=device)
    for k in range(n):
        index = n - 1 - k
        ops.ddim_step_begin(None, xd, smp._t_table, step, 1, sample, t_out)
        ops.cfg_dpm_step_dev(eps_seq[k], xd, table, step, state, x_prev=xd, d_hist=hist, **kw)
        assert torch.equal(xd, want[k][0]) and torch.equal(hist, want[k][1]), k
        assert step.tolist() == [index - 1, index]
        words = state.tolist()
        assert words[(index - 1) & 1] == 1 and words[2:] == [2, int(final_first)], (k, words)
        assert torch.equal(t_out, smp._t_table[index].expand(b))
    # past the end of the schedule: the words move on, no element is written
    before = (xd.clone(), hist.clone())
    step[1] = -1
    ops.cfg_dpm_step_dev(eps_seq[0], xd, table, step, state, x_prev=xd, d_hist=hist, **kw)
    assert torch.equal(xd, before[0]) and torch.equal(hist, before[1]) and step.tolist() == [-2, -1] and state.tolist()[0] == 0
    # order = 1 in the state words: the history is never read
    state1 = torch.tensor([1, 1, 1, 0], dtype=torch.int32, device=device)
    step1 = torch.tensor([0, 4], dtype=torch.int32, device=device)
    xo, ho = x_T.clone(), torch.full(x_T.shape, float("nan"), device=device)
    ops.cfg_dpm_step_dev(eps_seq[0], xo, table, step1, state1, x_prev=xo, d_hist=ho, **kw)
    fx, fd = ops.cfg_dpm_step(eps_seq[0], x_T, smp.dpm_coef, 4, 1, **kw)
    assert torch.equal(xo, fx) and torch.equal(ho, fd)


# ---- 3. the sampler on the mini UNet ---------------------------------------------------------------------------------------
def _mini_inputs(cfg, b=1, f1=1, Fp=2, H=16, seed=0):
    x0_emb = _randn((b, 4, f1, H, H), seed + 1) * 0.9
    c = _randn((b, f1 + Fp, 77, cfg["cross_attention_dim"]), seed + 2)
    uc = _randn((b, 1, 77, cfg["cross_attention_dim"]), seed + 3).expand(-1, f1 + Fp, -1, -1).contiguous()
    return x0_emb, c, uc, _randn((b, 4, Fp, H, H), seed + 4)


def test_dpm_sampler_matches_oracle(device):
    """S = 10 with guidance 7.5 against the float64 restatement driven by the oracle's UNet on the CPU.  The bound is the one
    tests/test_gpu_plms.py holds PLMSSampler to on this model, 8e-2; DDIMSampler's own distance to its restatement on the same
    model, S and inputs is measured beside it (profiles/dpm_sampler.md records both: 2.83e-2 for this sampler, 2.91e-2 for DDIM)."""
    cfg, sd, m = _model(device)
    b, Fp, H, S = 1, 2, 16, 10
    x0_emb, c, uc, noise = _mini_inputs(cfg)
    unet_fn = lambda x, t, cc, cf: O.unet_forward(sd, cfg, x, t, cc, cond_frame=cf)
    eps_fn = lambda x, t: P.model_eps(unet_fn, x.float(), c, t, x0_emb, 7.5, uc, 0).double()
    kw = dict(unet=m, S=S, conditioning=c.to(device), batch_size=b, shape=(4, Fp, H, H), x0_emb=x0_emb.to(device), verbose=False,
              unconditional_guidance_scale=7.5, unconditional_conditioning=uc.to(device), eta=0.0, x_T=noise.to(device), is_3d=True)
    sampler = DPMSolverSampler(device)
    lat, inter = sampler.sample(**kw)
    with torch.no_grad():
        ref_lat, steps = R.sampling64(eps_fn, noise, sampler.ddim_alphas, sampler.ddim_alphas_prev, sampler.ddim_timesteps)
        ref_ddim = R.ddim_sampling64(eps_fn, noise, sampler.ddim_alphas, sampler.ddim_alphas_prev, sampler.ddim_timesteps)
    ddim_lat, _ = DDIMSampler(device).sample(**kw)
    assert [k for _, _, k in steps] == [1] + [2] * 8 + [1] and len(inter["x_inter"]) == 3
    rel, rel_ddim = _rel(lat, ref_lat), _rel(ddim_lat, ref_ddim)
    print(f"[parity] latent after {S} CFG steps against the restatement over the oracle: dpm rel_l2={rel:.4g}, ddim rel_l2={rel_ddim:.4g}")
    assert rel <= 8e-2, (rel, rel_ddim)


# ---- 4. the captured step --------------------------------------------------------------------------------------------------
def test_captured_dpm_step_equals_the_launch_by_launch_step(device):
    """unet.use_graph: EVERY step is ONE hipGraph (seer_ddim_step_begin, the UNet, seer_cfg_dpm_step_dev).  Same bits as the
    launches of a fresh sampler over whole samples: another prompt, a longer and a shorter schedule, scale 1.0, a schedule longer
    than the captured table (stepped launch by launch), the RNG stream in the same state afterwards, returned tensors the caller
    keeps; then decode, and a chain whose caller jumps the index."""
    cfg, sd, m = _model(device)
    b, f1, Fp, H = 1, 1, 2, 16
    captured = DPMSolverSampler(device)

    def draw(seed):
        return tuple(t.to(device) for t in _mini_inputs(cfg, seed=seed))

    def sample(sampler, graph, S, args, scale):
        x0, c, uc, noise = args
        m.use_graph = graph
        torch.manual_seed(5)
        preds = []
        lat, inter = sampler.sample(unet=m, S=S, conditioning=c, batch_size=b, shape=(4, Fp, H, H), x0_emb=x0, verbose=False,
                                    unconditional_guidance_scale=scale, unconditional_conditioning=uc, eta=0.0, x_T=noise,
                                    is_3d=True, img_callback=lambda p, i: preds.append(p))
        return lat, inter, preds, torch.rand(3, device=device)

    def graphs():
        return [k for k in m._engine._graphs if isinstance(k, tuple) and k and k[0] == "dpm"]

    try:
        kept = []
        # S = 70 has 72 entries, more than the 64 rows of the table captured with the first sample: launch by launch.  The plain
        # step comes last: another context shape empties the engine's graph cache
        for S, seed, scale in ((10, 1, 7.5), (10, 11, 7.5), (20, 21, 7.5), (6, 31, 7.5), (70, 51, 7.5), (10, 41, 1.0)):
            args = draw(seed)
            want, wi, wp, wr = sample(DPMSolverSampler(device), False, S, args, scale)
            got, gi, gp, gr = sample(captured, True, S, args, scale)
            assert torch.equal(got, want) and torch.equal(gr, wr), (S, seed)
            assert all(torch.equal(a, b_) for a, b_ in zip(gi["x_inter"] + gi["pred_x0"], wi["x_inter"] + wi["pred_x0"]))
            assert len(gp) == len(wp) == captured.ddim_timesteps.shape[0] == {10: 10, 20: 20, 6: 7, 70: 72}[S]
            assert all(torch.equal(a, b_) for a, b_ in zip(gp, wp)), (S, seed)
            kept.append((got, got.clone(), gp, [p.clone() for p in gp]))
            keys = graphs()
            assert len(keys) == 1 and keys[0][3] == (scale != 1.0), (S, seed, keys)        # one captured step, reused
            assert m._engine._graphs[keys[0]]["dpm_coef"].shape[0] == 64                    # never re-captured for a schedule
        for got, copy, gp, gcopy in kept:      # nothing a later step or sample wrote reached what the caller kept
            assert torch.equal(got, copy) and all(torch.equal(a, b_) for a, b_ in zip(gp, gcopy))
        assert not captured._capture_refused
        # decode from t_start: captured, launch by launch, and a hand-driven chain of p_sample_dpm from the same entry
        x0, c, uc, noise = draw(61)
        outs = []
        for sampler, graph in ((captured, True), (DPMSolverSampler(device), False)):
            m.use_graph = graph
            sampler.make_schedule(10, verbose=False)
            outs.append(sampler.decode(m, noise, c, 6, unconditional_guidance_scale=7.5, unconditional_conditioning=uc, x0_emb=x0))
        fresh = sampler
        x, d_prev = noise, None
        for index in reversed(range(6)):
            x, d_prev = fresh.p_sample_dpm(m, x, c, fresh._t_table[index].expand(b), index, x0_emb=x0,
                                           unconditional_guidance_scale=7.5, unconditional_conditioning=uc, d_prev=d_prev)
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], x)
        # a caller that jumps the index: the captured chain restarts first order there
        m.use_graph = True
        captured.make_schedule(10, verbose=False)
        xg, xe, d_prev, last = noise, noise, None, None
        for index in (9, 8, 7, 4, 3):
            g = captured._dpm_graph_step(m, xg, c, uc, index, x0, 0, 7.5, restart=last is None)
            assert g is not None
            if last is not None and index != last - 1:
                d_prev = None
            xe, d_prev = fresh.p_sample_dpm(m, xe, c, fresh._t_table[index].expand(b), index, x0_emb=x0,
                                            unconditional_guidance_scale=7.5, unconditional_conditioning=uc, d_prev=d_prev)
            assert torch.equal(g[0], xe) and torch.equal(g[1], d_prev), index
            xg, last = g[0], index
    finally:
        m.use_graph = False


# ---- 5. the solver on the analytic model -----------------------------------------------------------------------------------
def test_accuracy_on_the_gaussian_probability_flow_ode(device):
    """the three conditions of tests/test_dpm_host.py on the GPU kernels (launch by launch, a Python model)"""
    x_T = R.start_codes()
    c = torch.zeros((1, 1, 1, 1), device=device)
    err = {}
    for method, grid, S in R.ACCURACY_CASES:
        smp = DPMSolverSampler(device, discretize=grid) if method == "2m" else DDIMSampler(device)
        smp.make_schedule(S, verbose=False)
        eps, _ = R.gaussian(smp.alphas_cumprod)
        model = lambda x, t, cc, cond_frame=0: eps(x.double().cpu(), t).float().to(x.device)
        lat, _ = smp.sample(model, S, 1, x_T.shape[1:], conditioning=c, x_T=x_T.float().to(device), verbose=False, is_3d=True)
        err[method, grid, S] = R.max_error(lat, smp, x_T)
    print(f"[dpm] max error against the closed form, on the kernels: {err}")
    R.assert_accuracy(err)


# ---- 6. frame-sharded ------------------------------------------------------------------------------------------------------
def _dpm_worker(rank, world, port, out_path):
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    backend, dev = _backend(rank, world)
    if backend == "nccl":
        torch.cuda.set_device(dev)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        from seervideoldm_amd import DPMSolverSampler, SeerUNet, parallel, synth
        if backend == "gloo":
            _host_staged_gathers()
        m = SeerUNet(**CFG_MINI).to(dev)
        m.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI), device=dev), strict=True)
        m.eval()
        g = torch.Generator().manual_seed(7)
        b, f1, Fp, H = 1, 1, 3, 16
        x0 = (torch.randn((b, 4, f1, H, H), generator=g) * 0.9).to(dev)
        c = torch.randn((b, f1 + Fp, 77, 256), generator=g).to(dev)
        noise = torch.randn((b, 4, Fp, H, H), generator=g).to(dev)

        # unguided, two steps, as tests/test_gpu_plms.py's counterpart (its bound is that of one evaluation); lower_order_final off,
        # so that the second step of the two-entry schedule is a 2M step
        def run():
            torch.manual_seed(5)
            return DPMSolverSampler(dev, lower_order_final=False).sample(unet=m, S=2, conditioning=c, batch_size=b, shape=(4, Fp, H, H),
                                                                         x0_emb=x0, verbose=False, eta=0.0, x_T=noise, is_3d=True)[0].cpu()
        ref = run()
        shard = parallel.attach(m, world, rank, batch_groups=1)
        got = run()
        torch.save(dict(ref=ref, got=got, desc=shard.describe()), f"{out_path}.{rank}")
    finally:
        dist.destroy_process_group()


def test_frame_sharded_dpm_sample(tmp_path):
    out = tmp_path / "res.pt"
    _spawn(_dpm_worker, 2, str(out))
    r0, r1 = torch.load(f"{out}.0"), torch.load(f"{out}.1")
    assert r0["desc"].startswith("batch_groups1xframe_shards2")
    rel = ((r0["got"] - r0["ref"]).norm() / r0["ref"].norm()).item()
    print(f"[parity] 2 DPM-Solver++ steps frame-sharded ({r0['desc']}) vs one process: rel_l2={rel:.4g}")
    assert rel < 3e-2, rel                                     # test_gpu_plms.py::test_frame_sharded_plms_sample's bound
    assert torch.equal(r0["got"], r1["got"]), "every rank runs the same update on rank 0's inputs"
