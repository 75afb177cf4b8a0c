"""FreeU without a GPU (tests/freeu_ref.py): the closed form the kernel evaluates against diffusers' FFT form, the exact
construction the GPU test relies on, the engine's schedule with FreeU on through the plain-torch stand-in against the patched oracle,
the identity setting and the launch count, the public surface and its refusals, the library's argument validation, the three graph
keys, and one frame-sharded gloo case."""
import ctypes
import os
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist

from oracle import seer_oracle as O
from seervideoldm_amd import DDIMSampler, SeerUNet, SlotSampler, compat, ops, synth
from seervideoldm_amd import ddim as ddim_module
from seervideoldm_amd import slots as slots_module
from tests import freeu_ref as R
from tests import slot_ref
from tests.test_dist_gloo import _spawn
from tests.test_engine_cpu import CFG_MINI

ROOT = Path(__file__).resolve().parents[1]
PARAMS = (0.9, 0.2, 1.2, 1.4)       # s1, s2, b1, b2: the values of the paper's SD-1.x recipe
CASES = [(1, 2, 16, 0), (2, 3, 8, 1)]


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ---- 1. closed form == FFT form -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (1, 4), (4, 1), (2, 2), (2, 4), (3, 5), (4, 4), (5, 8), (7, 7), (8, 8), (16, 16)])
@pytest.mark.parametrize("s", [0.0, 0.2, 0.9, 1.0, 1.5])
def test_closed_form_equals_fft_form(H, W, s):
    x = _randn((3, 5, H, W), 100 * H + W).double()
    err = (R.freeu_closed_form(x, s) - R.fourier_filter_fft(x, s)).abs().max().item()
    assert err <= 1e-13, err


def test_residue_sets():
    assert R.residues(1) == [0] and R.residues(2) == [0, 1] and R.residues(7) == [0, 6]
    # the product's table is the reference's, bit for bit, and exact at the quarter turns
    for H, W in ((1, 1), (2, 4), (3, 5), (8, 8), (12, 16)):
        (cH, sH), (cW, sW) = R.twiddles(H), R.twiddles(W)
        assert torch.equal(ops.freeu_twiddles(H, W), torch.cat([cH, sH, cW, sW]))
    c, s = R.twiddles(8)
    assert c[2] == 0 and s[4] == 0 and c[6] == 0 and c[4] == -1 and s[6] == -1


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_rnd64_is_the_storage_rounding(dtype):
    """the GPU test's per-element check rounds float64 values itself: on fp32-valued inputs (torch's conversion then rounds once) it
    must agree with torch, subnormal fp16 values and ties included"""
    x = torch.cat([_randn((20000,), 9) * 3, _randn((2000,), 10) * 1e-5, torch.tensor([0.0, 1.0, -2.5, 1.00390625, 1.01171875, 6.0e-8])])
    assert torch.equal(R.rnd64(x.double(), dtype), x.to(dtype).double())
    # just above a tie: one rounding goes up, the two roundings of a conversion through fp32 land on the tie and go to even
    assert R.rnd64(torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64), torch.bfloat16).item() == 1.0078125


# ---- 2. the exact construction of the GPU test --------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(2, 2), (2, 4), (4, 2), (4, 4)])
def test_exact_construction(H, W):
    x = torch.randint(-3, 4, (6, 16, H, W), generator=torch.Generator().manual_seed(H * 10 + W)).double()
    r64 = R.freeu_closed_form(x, 0.5, torch.float64)
    r32 = R.freeu_closed_form(x, 0.5, torch.float32)
    assert r32.dtype == torch.float32 and torch.equal(r32.double(), r64)
    assert torch.equal(r64.to(torch.bfloat16).double(), r64) and torch.equal(r64.to(torch.float16).double(), r64)
    assert not torch.equal(r64, x)
    # with cos(pi / 2) = 6e-17 left in the table the same plane is no longer exact: this pins the snapping
    if (H, W) != (2, 2):
        raw = R.freeu_closed_form(x, 0.5, torch.float64, snap=False)
        assert not torch.equal(raw, r64)


# ---- 3. / 4. the engine's schedule through the stand-in ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mini():
    sd = synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI))
    m = SeerUNet(**CFG_MINI)
    m.load_state_dict(sd, strict=True)
    return sd, m


def _engine(m, backend, params):
    """the model's engine over `backend` with FreeU at `params` (None: off), through the public surface"""
    m._ops_backend = backend
    m.disable_freeu() if params is None else m.enable_freeu(*params)
    m.prepare(torch.bfloat16)
    return m._engine


def _inputs(B, Fr, H):
    return _randn((B, 4, Fr, H, H), 1), _randn((B, Fr, 77, 256), 2), torch.tensor([501] * B)


@pytest.mark.parametrize("B,Fr,H,cond_frame", CASES)
def test_engine_with_freeu_matches_the_patched_oracle(mini, B, Fr, H, cond_frame):
    """FAILS WITHOUT THE FEATURE: the patched oracle sits 0.46 / 0.49 rel-L2 away from the unpatched one at these two cases"""
    sd, m = mini
    x, ctx, t = _inputs(B, Fr, H)
    try:
        eng = _engine(m, R.TorchOpsWithFreeu(), PARAMS)
        with torch.no_grad():
            got = eng.run(x, t, ctx, cond_frame)
            plain = O.unet_forward(sd, CFG_MINI, x, t, ctx, cond_frame=cond_frame)
            with R.patched_oracle(PARAMS, CFG_MINI):
                ref = O.unet_forward(sd, CFG_MINI, x, t, ctx, cond_frame=cond_frame)
    finally:
        m.disable_freeu()
    apart = ((ref - plain).norm() / plain.norm()).item()
    assert apart > 0.3, apart                   # the guard: the two references differ by far more than the bound below
    rel = ((got - ref).norm() / ref.norm()).item()
    assert rel < 3e-2, rel


@pytest.mark.parametrize("B,Fr,H,cond_frame", CASES)
def test_identity_values_and_launch_count(mini, B, Fr, H, cond_frame):
    sd, m = mini
    x, ctx, t = _inputs(B, Fr, H)
    lpb = CFG_MINI["layers_per_block"]
    try:
        rec = R.RecordingFreeu()
        eng = _engine(m, rec, (1.0, 1.0, 1.0, 1.0))
        with torch.no_grad():
            on = eng.run(x, t, ctx, cond_frame)
        h0, h1 = H // 8, H // 4                 # the planes of up_blocks.0 and up_blocks.1
        assert rec.calls == [(h0, h0, 320, 320, (1.0, 1.0))] * (lpb + 1) + [(h1, h1, 320, 320, (1.0, 1.0))] * (lpb + 1)
        n_on = eng.gn_from_colsums
        m.disable_freeu()
        del rec.calls[:]
        with torch.no_grad():
            off = eng.run(x, t, ctx, cond_frame)
        assert rec.calls == [] and eng.gn_from_colsums == n_on + 2 * (lpb + 1)      # the norm1s are back on their producers' sums
        with torch.no_grad():
            never = _engine(m, R.TorchOpsWithFreeu(), None).run(x, t, ctx, cond_frame)
        assert torch.equal(off, never)
    finally:
        m.disable_freeu()
    rel = ((on - off).norm() / off.norm()).item()
    assert rel < 3e-2, rel
    # other values reach the same engine's buffer in place, in (b1, s1, b2, s2) order
    eng = _engine(m, R.TorchOpsWithFreeu(), (1.0, 1.0, 1.0, 1.0))
    buf = eng._freeu_buf
    m.enable_freeu(*PARAMS)
    assert eng._freeu_buf is buf and buf.tolist() == pytest.approx([1.2, 0.9, 1.4, 0.2]) and eng.freeu_on
    m.disable_freeu()
    assert not eng.freeu_on


# ---- 5. surface and refusals ---------------------------------------------------------------------------------------------------
def test_surface():
    m = SeerUNet(**CFG_MINI)
    assert m._freeu is None and m.enable_freeu(0.9, 0.2, 1.2, 1.4) is m and m._freeu == (0.9, 0.2, 1.2, 1.4)
    assert m.enable_freeu(s1=1, s2=2, b1=3, b2=4)._freeu == (1.0, 2.0, 3.0, 4.0)       # diffusers' names and order
    for bad in (float("nan"), float("inf"), -float("inf")):
        for i in range(4):
            with pytest.raises(ValueError, match="finite"):
                m.enable_freeu(*[bad if j == i else 1.0 for j in range(4)])
    assert m._freeu == (1.0, 2.0, 3.0, 4.0)
    assert m.disable_freeu() is m and m._freeu is None
    # an engine built later starts with the model's setting
    m.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI)), strict=True)
    m._ops_backend = R.TorchOpsWithFreeu()
    m.enable_freeu(*PARAMS)
    assert m._engine is None
    m.prepare(torch.bfloat16)
    assert m._engine.freeu_on and m._engine.freeu_key == ("freeu",)
    m.disable_freeu()
    assert not m._engine.freeu_on and m._engine.freeu_key == ()


def test_compat_switch(monkeypatch):
    try:
        monkeypatch.setenv("SEER_COMPAT_FREEU", "0.9,0.2,1.2,1.4")
        compat.install()
        from seer.models.unet_3d_condition import SeerUNet as Aliased
        u = Aliased(**CFG_MINI)
        assert isinstance(u, SeerUNet) and Aliased.__name__ == "SeerUNet" and u._freeu == (0.9, 0.2, 1.2, 1.4)
        compat.uninstall()
        monkeypatch.setenv("SEER_COMPAT_FREEU", "")
        compat.install()
        from seer.models.unet_3d_condition import SeerUNet as Plain
        assert Plain is SeerUNet
        compat.uninstall()
        compat.install(freeu=(1.0, 0.5, 1.1, 1.2))           # the argument goes before the environment
        from seer.models.unet_3d_condition import SeerUNet as Aliased2
        assert Aliased2(**CFG_MINI)._freeu == (1.0, 0.5, 1.1, 1.2)
        compat.uninstall()
        for bad in ("0.9,0.2,1.2", "a,b,c,d", "0.9,0.2,1.2,nan", "0.9;0.2;1.2;1.4", "1,2,3,4,5"):
            monkeypatch.setenv("SEER_COMPAT_FREEU", bad)
            with pytest.raises(ValueError, match="SEER_COMPAT_FREEU"):
                compat.install()
    finally:
        compat.uninstall()
        monkeypatch.delenv("SEER_COMPAT_FREEU", raising=False)
        compat.install()
        compat.uninstall()


def test_trainer_refuses_freeu():
    from seervideoldm_amd.trainer import SeerTrainer
    from tests import torch_ops_backend as tob
    from tests import torch_train_ops_backend as ttob
    from tests.test_dist_gloo import _train_models
    unet, fst = _train_models()
    unet.enable_freeu(*PARAMS)
    with pytest.raises(ValueError, match="FreeU"):
        SeerTrainer(unet, fst, ops=tob, tops=ttob)
    unet.disable_freeu()
    SeerTrainer(unet, fst, ops=tob, tops=ttob)


def test_library_refusals_without_gpu():
    """every refusal of the header, before the device is touched (with good arguments these calls would launch: only bad ones here)"""
    from seervideoldm_amd import _lib
    f = _lib.load().seer_freeu
    A, B, C_, D, P, T = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000      # aligned, 64 KiB apart; rows 24 x 64 ch = 3 KiB
    ok = dict(x=A, xo=B, Cx=64, s=C_, so=D, Cs=64, rows=24, images=6, H=2, W=2, p=P, t=T, dt=0)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["x"], a["xo"], a["Cx"], a["s"], a["so"], a["Cs"], a["rows"], a["images"], a["H"], a["W"], a["p"], a["t"], a["dt"], None)
    bad = [dict(x=None, xo=None, s=None, so=None), dict(xo=None), dict(x=None), dict(so=None), dict(s=None),
           dict(xo=C_), dict(so=A), dict(xo=D), dict(xo=C_ + 1024), dict(so=A + 2048), dict(xo=A + 16), dict(so=C_), dict(so=C_ + 64),
           dict(H=0), dict(W=0), dict(H=-2), dict(images=0), dict(rows=25), dict(rows=23), dict(images=5),
           dict(Cx=60), dict(Cs=12), dict(Cx=0), dict(Cs=-8), dict(x=A + 8), dict(xo=B + 2), dict(s=C_ + 4), dict(so=D + 8),
           dict(p=None), dict(t=None), dict(p=P + 2), dict(t=T + 1), dict(dt=2), dict(dt=-1)]
    for kw in bad:
        assert call(**kw) == -22, kw
    assert call(x=None, xo=None, Cx=0, s=None, so=None, Cs=0) == -22


# ---- the three graph keys ---------------------------------------------------------------------------------------------------------
class _Seen(Exception):
    pass


def _key_of(eng, monkeypatch, fn):
    """the key `fn` hands to the engine's graph cache (the lookup is where this stops: nothing is captured on a CPU)"""
    def graph_get(key):
        raise _Seen(key)
    monkeypatch.setattr(eng, "graph_get", graph_get)
    try:
        with pytest.raises(_Seen) as e:
            fn()
    finally:
        monkeypatch.undo()
    return e.value.args[0]


def test_graph_keys(mini, monkeypatch):
    _, m = mini
    eng = _engine(m, R.TorchOpsWithFreeu(), None)
    cpu = torch.device("cpu")
    x, ctx, t = _inputs(1, 3, 8)
    smp = DDIMSampler("cpu")
    smp.make_schedule(4, verbose=False)
    xs, x0e, c = _randn((1, 4, 2, 8, 8), 3), _randn((1, 4, 1, 8, 8), 4), _randn((1, 3, 77, 256), 5)
    slot = SlotSampler(m, 2, shape=(4, 2, 8, 8), cond_frames=1, context_shape=(77, 256), device="cpu", ops=slot_ref, model_cond_frame=1)

    def keys():
        c16, L = eng._context(ctx)
        k_unet = _key_of(eng, monkeypatch, lambda: eng._run_graph(x, t, c16, L, 1))
        monkeypatch.setattr(ddim_module, "capture_engine", lambda *a: eng)
        k_ddim = _key_of(eng, monkeypatch, lambda: smp._step_graph(m, xs, c, None, x0e, 1, 1.0, "step"))
        monkeypatch.setattr(slots_module, "capture_engine", lambda *a: eng)
        monkeypatch.setattr(slots_module, "engine_on", lambda *a: eng)
        k_slot = _key_of(eng, monkeypatch, slot._run_step)
        return k_unet, k_ddim, k_slot
    try:
        off = keys()
        # off: the tuples of the parent commit, word for word
        assert off[0] == ((1, 4, 3, 8, 8), 77, 1, (231, 256), False)
        assert off[1] == ("step", (1, 4, 2, 8, 8), 1, False, 1, None, 77, (231, 256), False)
        assert off[2] == ("slots", 2, (4, 2, 8, 8), 1, 1, 77, (4 * 3 * 77, 256), False)
        m.enable_freeu(*PARAMS)
        on = keys()
        m.enable_freeu(1.0, 0.5, 1.1, 1.3)
        other = keys()
    finally:
        m.disable_freeu()
    for a, b, c_ in zip(off, on, other):
        assert b == a + ("freeu",) and c_ == b          # on: one more word; other values: the same graph
    assert keys() == off


# ---- 6. frame shards over gloo ------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, out_path):
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from seervideoldm_amd import parallel
        from tests import torch_ops_backend as tob
        m = SeerUNet(**CFG_MINI)
        m.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI)), strict=True)
        m._ops_backend = R.TorchOpsWithFreeu()
        tob.EXACT = True
        m.ln_fold = False           # (as tests/test_dist_gloo.py: one arithmetic for row subsets and whole rows)
        m.ff_fold = False
        m.enable_freeu(*PARAMS)
        g = torch.Generator().manual_seed(7)
        x, ctx, t = torch.randn((1, 4, 3, 8, 8), generator=g), torch.randn((1, 3, 77, 256), generator=g), torch.tensor([501])
        ref1 = off1 = None
        if rank == 0:
            parallel.attach(m, 1, 0).force_exact_stats = True
            ref1 = m(x, t, ctx, cond_frame=1)
            m.disable_freeu()
            off1 = m(x, t, ctx, cond_frame=1)
            m.enable_freeu(*PARAMS)
        parallel.attach(m, world, rank, batch_groups=1)
        got = m(x, t, ctx, cond_frame=1)
        if rank == 0:
            torch.save(dict(ref1=ref1, off1=off1, got=got, on=m._engine.freeu_on), out_path)
    finally:
        dist.destroy_process_group()


def test_frame_sharded_engine_with_freeu_is_bit_identical_to_one_rank(tmp_path):
    out = tmp_path / "res.pt"
    _spawn(_worker, 2, str(out))
    r = torch.load(out)
    assert r["on"] and torch.equal(r["got"], r["ref1"]), (r["got"] - r["ref1"]).abs().max().item()
    assert not torch.equal(r["ref1"], r["off1"])         # FreeU did run
