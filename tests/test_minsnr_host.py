"""Min-SNR-gamma loss weighting without a GPU, on the torch stand-ins (tests/minsnr_ref.py over tests/vpred_ref.py): the stand-in against
autograd in float64, the division-free weight forms against the paper's quotients, the trainer's wiring -- what it hands the backend,
bit for bit against a twin whose plain loss is replaced by the weighted stand-in --, the refusals and the surface.  Runs everywhere
(CPU)."""
import inspect
import math

import numpy as np
import pytest
import torch

from seervideoldm_amd.trainer import SeerTrainer, ddpm_alphas_cumprod
from tests import minsnr_ref as M
from tests import vpred_ref as V
from tests.test_vpred_host import train_models  # noqa: F401  (the fixture: the 320-wide one-layer models of test_train_batch_cpu)

f64 = torch.float64
GAMMA = 5.0
PTYPES = ("epsilon", "v_prediction")


# ---- the restatement itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [False, True])
def test_stand_in_dpred_is_the_autograd_gradient_of_its_loss_in_float64(v):
    g = torch.Generator().manual_seed(3)
    B, C, Ft, cond_f, H, W = 3, 2, 4, 1, 3, 5
    pred = torch.randn((B, C, Ft, H, W), generator=g, dtype=f64)
    target = torch.randn((B, C, Ft - cond_f, H, W), generator=g, dtype=f64)
    t, table = torch.tensor([3, 999, 100]), ddpm_alphas_cumprod()
    loss, dpred, sample, w = M.snr_mse_loss_grad(pred, target, t, table, cond_f, GAMMA, v)
    assert loss.shape == (1,) and dpred.shape == pred.shape and sample.shape == w.shape == (B,) and dpred.dtype == f64
    p = pred.clone().requires_grad_(True)
    auto, sample2 = M.weighted_loss(p, target, w, cond_f)
    auto.backward()
    assert torch.allclose(loss[0], auto.detach(), rtol=1e-14, atol=0) and torch.equal(sample, sample2.detach())
    assert (p.grad[:, :, :cond_f] == 0).all() and (dpred[:, :, :cond_f] == 0).all()
    assert float((dpred - p.grad).abs().max()) <= 1e-15 * float(p.grad.abs().max())
    assert len(set(w.tolist())) == B                     # three different weights: a swapped pair would show
    # and the float64 definition agrees with it on fp32 inputs
    p32, t32 = pred.float(), target.float()
    l64, s64, d64 = M.snr_mse64(p32, t32, t, table, cond_f, GAMMA, v)
    l, d, s, _ = M.snr_mse_loss_grad(p32.double(), t32.double(), t, table, cond_f, GAMMA, v)
    assert torch.allclose(l[0], l64, rtol=1e-6) and torch.allclose(s, s64, rtol=1e-6) and torch.allclose(d, d64, rtol=1e-6, atol=1e-12)
    # caller-owned outputs
    sl, ww = torch.full((B,), math.nan), torch.full((B,), math.nan)
    out = M.snr_mse_loss_grad(p32, t32, t, table, cond_f, GAMMA, v, sample_loss=sl, weights=ww)
    assert out[2] is sl and out[3] is ww and torch.isfinite(sl).all() and torch.equal(ww, M.weights32(t, table, GAMMA, v))


@pytest.mark.parametrize("gamma", [1.0, 5.0, 20.0])
@pytest.mark.parametrize("v", [False, True])
def test_division_free_forms_equal_the_papers_quotients_on_the_ddpm_table(v, gamma):
    table = ddpm_alphas_cumprod()
    t = torch.arange(table.numel())
    got, want = M.weights64(t, table, gamma, v), M.textbook64(t, table, gamma, v)
    rel = np.abs(got - want) / want
    print(f"[minsnr] v={v} gamma={gamma}: worst relative difference {rel.max():.3g}")
    assert rel.max() <= 1e-12 and (got > 0).all() and (got <= 1).all()
    if not v:                                            # clamped where SNR > gamma, 1 elsewhere: both branches occur on this table
        assert (got == 1.0).any() and (got < 1.0).any()


def test_weights_at_the_ends_of_a_table_and_outside_it():
    table = torch.tensor([0.0, 1.0, 0.5, 0.25, 0.8125])
    t = torch.tensor([0, 1])
    assert M.weights64(t, table, GAMMA, False).tolist() == [1.0, 0.0]        # eps: a = 0 -> 1, a = 1 -> 0
    assert M.weights64(t, table, GAMMA, True).tolist() == [0.0, 0.0]         # v:   0 and 0
    assert M.weights64(torch.tensor([2, 3]), table, 0.5, False).tolist() == [0.5, 1.0]
    assert M.weights64(torch.tensor([2, 3, 4]), table, 5.0, True).tolist() == [0.5, 0.25, 0.8125]
    assert M.weights64(torch.tensor([4]), table, 1.0, True).tolist() == [0.1875]
    assert M.weights64(torch.tensor([-7, 99, 2 ** 40]), table, 5.0, True).tolist() == [0.0, 0.8125, 0.8125]     # clamped into the table


# ---- the trainer --------------------------------------------------------------------------------------------------------------------------
def _trainer(train_models, Fr, prediction_type, tops, **kw):
    """gradient_accumulation_steps = 2: the call under test back-propagates and does not step, so two trainers stay comparable"""
    from tests import torch_ops_backend as tob
    from tests.test_train_batch_cpu import HP
    unet, fst = train_models
    fst.set_numframe(Fr)
    return SeerTrainer(unet, fst, ops=tob, tops=tops, gradient_accumulation_steps=2, prediction_type=prediction_type, **HP, **kw)


def _twin_ops(t, table, gamma, v):
    """a backend WITHOUT snr_mse_loss_grad whose mse_loss_grad is the weighted stand-in at (t, table, gamma, v)"""
    base = V.train_ops()

    class Twin(type(base)):
        def mse_loss_grad(self, pred, target, cond_f):
            return M.snr_mse_loss_grad(pred, target, t, table, cond_f, gamma, v)[:2]
    return Twin()


def _same_step(a, b, loss_a, loss_b):
    assert torch.equal(loss_a, loss_b) and torch.isfinite(loss_a).all()
    assert torch.equal(a.pu.g, b.pu.g) and torch.equal(a.pf.g, b.pf.g) and bool(a.pu.g.abs().sum() > 0)


@pytest.mark.parametrize("ptype", PTYPES)
def test_trainer_with_snr_gamma_is_a_twin_whose_loss_is_the_weighted_stand_in(train_models, ptype):
    """forward_backward, train_step and step_from_batch, each against a trainer WITHOUT snr_gamma whose backend's mse_loss_grad is the
    weighted stand-in on the same inputs: loss and both gradient segments bit for bit; the recorded call shows the trainer's own
    timesteps, the table it holds, cond_frames, gamma and the v flag; and the flat loss on the same inputs differs"""
    from tests.test_train_batch_cpu import _Text, _Vae, _batch
    b, Fr, cond = 2, 3, 1
    v = ptype == "v_prediction"
    acp = ddpm_alphas_cumprod()
    g = torch.Generator().manual_seed(11)
    lat_x0, lat, nz = (torch.randn((b, 4, n, 8, 8), generator=g) for n in (cond, Fr - cond, Fr - cond))
    text = torch.randn((b, 77, 192), generator=g)
    t = torch.tensor([40, 950])                           # SNR above and below gamma: eps weights (< 1, 1), two different v weights
    w = M.weights32(t, acp, GAMMA, v)
    assert w[0] != w[1] and (v or (w[0] < 1 and w[1] == 1))

    def check_call(tops, tr, t_want, n_calls=1):
        assert len(tops.snr_calls) == n_calls
        pred, target, t_got, table, cond_f, gamma, vflag = tops.snr_calls[-1]
        assert pred is tr.last_pred and torch.equal(t_got, t_want) and t_got.dtype == torch.int64
        assert table is tr._snr_acp and torch.equal(table, acp) and table.dtype == torch.float32
        assert (cond_f, gamma, bool(vflag)) == (cond, GAMMA, v)
        assert torch.equal(tr.last_loss_weights, M.weights32(t_want, acp, GAMMA, v)) and tr.last_sample_loss.shape == (b,)

    # forward_backward
    x = torch.cat([lat_x0, lat + nz], 2)
    tops = M.train_ops()
    tr = _trainer(train_models, Fr, ptype, tops, snr_gamma=GAMMA)
    loss = tr.forward_backward(x, nz, t, text, cond)
    twin = _trainer(train_models, Fr, ptype, _twin_ops(t, acp, GAMMA, v))
    _same_step(tr, twin, loss, twin.forward_backward(x, nz, t, text, cond))
    check_call(tops, tr, t)
    flat = _trainer(train_models, Fr, ptype, V.train_ops())
    assert not torch.equal(flat.forward_backward(x, nz, t, text, cond), loss) and not torch.equal(flat.pu.g, tr.pu.g)
    assert flat.last_sample_loss is None and flat.last_loss_weights is None
    # the loss is the weighted mean of the per-sample losses it reports
    assert torch.allclose(loss[0], (tr.last_loss_weights * tr.last_sample_loss).mean(), rtol=1e-6)

    # train_step (its own table argument: the same values in another tensor object pass the comparison)
    tops = M.train_ops()
    tr = _trainer(train_models, Fr, ptype, tops, snr_gamma=GAMMA)
    loss = tr.train_step(lat_x0, lat, nz, t, text, acp.clone())
    twin = _trainer(train_models, Fr, ptype, _twin_ops(t, acp, GAMMA, v))
    _same_step(tr, twin, loss, twin.train_step(lat_x0, lat, nz, t, text, acp))
    check_call(tops, tr, t)
    assert len(tops.velocity_calls) == (1 if v else 0) and tr.step_count == 0

    # step_from_batch, the random tensors injected so that both trainers see the same ones
    video, ids, mask = _batch(b, Fr, 5)
    table = torch.randn((8, 77, 192), generator=torch.Generator().manual_seed(4))
    inj = dict(noise=torch.randn((b, 4, Fr - cond, 8, 8), generator=g), timesteps=torch.tensor([999, 0]),
               posterior_noise=torch.randn((b * Fr, 4, 8, 8), generator=g))
    kw = dict(vae=_Vae([]), text_encoder=_Text([], table), cond_frames=cond, alphas_cumprod=acp, **inj)
    tops = M.train_ops()
    tr = _trainer(train_models, Fr, ptype, tops, snr_gamma=GAMMA)
    loss = tr.step_from_batch(video, ids, mask, **kw)
    twin = _trainer(train_models, Fr, ptype, _twin_ops(inj["timesteps"], acp, GAMMA, v))
    _same_step(tr, twin, loss, twin.step_from_batch(video, ids, mask, **kw))
    check_call(tops, tr, inj["timesteps"])
    # a second call on the same table object compares nothing again (the object was seen) and records a second call
    seen = tr._snr_acp_seen
    tr.step_from_batch(video, ids, mask, **kw)
    assert tr._snr_acp_seen is seen and seen[0] is acp
    check_call(tops, tr, inj["timesteps"], n_calls=2)


@pytest.mark.parametrize("ptype", PTYPES)
def test_without_snr_gamma_nothing_changes(train_models, ptype):
    """snr_gamma=None on a backend that HAS snr_mse_loss_grad: no such call, and the bits of a backend that lacks it (the flat loss, as before)"""
    b, Fr, cond = 1, 3, 1
    acp = ddpm_alphas_cumprod()
    g = torch.Generator().manual_seed(12)
    lat_x0, lat, nz = (torch.randn((b, 4, n, 8, 8), generator=g) for n in (cond, Fr - cond, Fr - cond))
    text, t = torch.randn((b, 77, 192), generator=g), torch.tensor([612])
    tops = M.train_ops()
    tr = _trainer(train_models, Fr, ptype, tops)
    assert tr.snr_gamma is None and not hasattr(tr, "_snr_acp")
    loss = tr.train_step(lat_x0, lat, nz, t, text, acp)
    parent = _trainer(train_models, Fr, ptype, V.train_ops())
    _same_step(tr, parent, loss, parent.train_step(lat_x0, lat, nz, t, text, acp))
    assert tops.snr_calls == [] and tr.last_sample_loss is None and tr.last_loss_weights is None
    tr.train_step(lat_x0, lat, nz, t, text, acp[:700])    # no table is held: nothing to compare a table with


def test_constructor_refusals(train_models):
    from tests.train_inputs_ref import TrainOpsWithInputs
    for bad in (0.0, -5.0, math.inf, -math.inf, math.nan):
        with pytest.raises(ValueError, match="snr_gamma"):
            _trainer(train_models, 3, "epsilon", M.train_ops(), snr_gamma=bad)
    # a backend without snr_mse_loss_grad: refused only when gamma is set, for eps and v alike (the rule of velocity_target)
    for ptype, tops in (("epsilon", TrainOpsWithInputs), ("epsilon", V.train_ops), ("v_prediction", V.train_ops)):
        assert _trainer(train_models, 3, ptype, tops()).snr_gamma is None
        with pytest.raises(ValueError, match="snr_mse_loss_grad"):
            _trainer(train_models, 3, ptype, tops(), snr_gamma=GAMMA)
    with pytest.raises(ValueError, match="alphas_cumprod"):
        _trainer(train_models, 3, "epsilon", M.train_ops(), snr_gamma=GAMMA, alphas_cumprod=torch.ones((2, 5)))
    tr = _trainer(train_models, 3, "epsilon", M.train_ops(), snr_gamma=7)
    assert tr.snr_gamma == 7.0 and isinstance(tr.snr_gamma, float) and torch.equal(tr._snr_acp, ddpm_alphas_cumprod())
    own = torch.linspace(0.99, 0.01, 50, dtype=f64)
    tr = _trainer(train_models, 3, "epsilon", M.train_ops(), snr_gamma=GAMMA, alphas_cumprod=own)
    assert tr._snr_acp.dtype == torch.float32 and torch.equal(tr._snr_acp, own.float()) and tr._snr_acp.data_ptr() != own.data_ptr()


def test_a_table_other_than_the_held_one_is_refused(train_models):
    from tests.test_train_batch_cpu import _Text, _Vae, _batch
    b, Fr, cond = 1, 3, 1
    acp = ddpm_alphas_cumprod()
    g = torch.Generator().manual_seed(13)
    lat_x0, lat, nz = (torch.randn((b, 4, n, 8, 8), generator=g) for n in (cond, Fr - cond, Fr - cond))
    text, t = torch.randn((b, 77, 192), generator=g), torch.tensor([100])
    tops = M.train_ops()
    tr = _trainer(train_models, Fr, "epsilon", tops, snr_gamma=GAMMA)
    other = acp.clone()
    other[100] *= 0.5
    video, ids, mask = _batch(b, Fr, 5)
    kw = dict(vae=_Vae([]), text_encoder=_Text([], torch.zeros((8, 77, 192))), cond_frames=cond)
    for bad, what in ((acp[:500], "entries"), (ddpm_alphas_cumprod(500), "entries"), (other, "differs"), (acp.view(10, 100), "entries")):
        with pytest.raises(ValueError, match=what):
            tr.train_step(lat_x0, lat, nz, t, text, bad)
        with pytest.raises(ValueError, match=what):
            tr.step_from_batch(video, ids, mask, alphas_cumprod=bad, **kw)
    assert tops.snr_calls == [] and tops.calls == [] and tr._micro == 0           # refused before anything ran
    # a table that passed and is then written to is compared again
    mine = acp.clone()
    tr.train_step(lat_x0, lat, nz, t, text, mine)
    assert len(tops.snr_calls) == 1
    mine[3] = 0.5
    with pytest.raises(ValueError, match="differs"):
        tr.train_step(lat_x0, lat, nz, t, text, mine)
    # a trainer built on its own table takes that table and refuses the default one
    short = ddpm_alphas_cumprod(500)
    tr2 = _trainer(train_models, Fr, "epsilon", M.train_ops(), snr_gamma=GAMMA, alphas_cumprod=short)
    tr2.train_step(lat_x0, lat, nz, t, text, short)
    with pytest.raises(ValueError, match="entries"):
        tr2.train_step(lat_x0, lat, nz, t, text, acp)


# ---- the surface --------------------------------------------------------------------------------------------------------------------------
def test_surface():
    from seervideoldm_amd import _lib, train_ops
    assert "seer_snr_mse_loss_grad" in _lib.SIGNATURES and "seer_mse_loss_grad" in _lib.SIGNATURES
    argtypes, restype = _lib.SIGNATURES["seer_snr_mse_loss_grad"]
    assert len(argtypes) == 18 and restype is _lib.C.c_int
    assert _lib.ABI_VERSION == 27                        # a declaration only: no struct changed
    assert callable(train_ops.snr_mse_loss_grad) and train_ops.SNR_MSE_BLOCKS == 64
    ours = inspect.signature(M.snr_mse_loss_grad).parameters
    theirs = inspect.signature(train_ops.snr_mse_loss_grad).parameters
    assert list(ours) == list(theirs) and all(ours[k].kind == theirs[k].kind and ours[k].default == theirs[k].default for k in ours)
    init = inspect.signature(SeerTrainer.__init__).parameters
    assert init["snr_gamma"].default is None and init["alphas_cumprod"].default is None
    assert all(init[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("snr_gamma", "alphas_cumprod"))
    header = (__import__("pathlib").Path(__file__).resolve().parents[1] / "include" / "seer_hip.h").read_text()
    assert "#define SEER_SNR_MSE_BLOCKS 64" in header and "int seer_snr_mse_loss_grad(" in header


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """every refusal returns SEER_EINVAL on the host (the pointers are aligned non-NULL integers that are no memory; no call here would
    pass its checks, so nothing is launched)"""
    from seervideoldm_amd import _lib
    from seervideoldm_amd.build import build_library
    build_library()
    lib = _lib.load()
    n = 0
    for args, why in M.refusal_cases(1 << 20, 1 << 30, 1 << 31):
        assert lib.seer_snr_mse_loss_grad(*args, None) == -22, why
        n += 1
    assert n >= 50
