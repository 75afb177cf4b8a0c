"""Min-SNR-gamma loss weighting on a real MI355X: seer_snr_mse_loss_grad exact on small integers, against float64 on normals at its
edges (scalar path, tail, 16-byte path, a base that is only 4-byte aligned, blocks that make more than one trip), at weight 1 against
seer_mse_loss_grad, every refusal; then SeerTrainer(snr_gamma=5.0) on the mini config of tests/test_gpu_train_batch.py: against a
twin whose backward is fed the kernel's dpred, and replayed from a captured step with new timesteps.

Every kernel call here goes through `_call`, which hands the entry point views into NaN-filled allocations: each output has NaN
words in front of it and behind it, and they are still NaN afterwards."""
import pytest
import torch

from seervideoldm_amd import _lib, train_ops
from seervideoldm_amd.trainer import SeerTrainer, ddpm_alphas_cumprod
from tests import minsnr_ref as M

pytestmark = pytest.mark.gpu

NAN = float("nan")
U = M.U
PAD = 8                                                  # NaN words on either side of every array (a multiple of 4: 16-byte bases)
CAP = train_ops.SNR_MSE_BLOCKS
EXACT_TABLE = [0.0, 1.0, 0.5, 0.25, 0.8125]              # dyadic weights: eps at gamma 0.5 -> 1, 0, 0.5, 1, .; v at gamma 5 -> 0, 0, 0.5, 0.25, 0.8125


def _bits(a, b):
    """bit for bit, NaN and the sign of zero included"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _held(shape, device, shift=0, dtype=torch.float32):
    """a view of `shape` inside a NaN-filled allocation, PAD + shift words behind its start -> (view, allocation)"""
    n = 1
    for s in shape:
        n *= s
    hold = torch.full((n + 2 * PAD + 4,), NAN, device=device, dtype=dtype)
    return hold[PAD + shift:PAD + shift + n].view(shape), hold


def _intact(view, hold, shift=0):
    n = view.numel()
    return bool(torch.isnan(hold[:PAD + shift]).all()) and bool(torch.isnan(hold[PAD + shift + n:]).all())


def _call(pred, target, t, table, cond_f, gamma, v, shift=0):
    """seer_snr_mse_loss_grad on fenced copies of the inputs and fenced outputs; shift = 1: pred, target and dpred start 4 bytes
    behind a 16-byte boundary.  -> (loss [1], dpred, sample_loss [B], weights [B]) after the fences were checked"""
    dev = pred.device
    B, C, Ft, H, W = pred.shape
    (p, hp), (g, hg), (dp, hdp) = (_held(x, dev, shift) for x in (pred.shape, target.shape, pred.shape))
    p.copy_(pred), g.copy_(target)
    (loss, hl), (sl, hsl), (w, hw) = (_held(s, dev) for s in ((1,), (B,), (B,)))
    ws, hws = _held((B * CAP,), dev, dtype=torch.float64)
    assert (dp.data_ptr() % 16 == 0) == (shift == 0) and p.data_ptr() % 4 == 0 and ws.data_ptr() % 8 == 0
    rc = _lib.load().seer_snr_mse_loss_grad(p.data_ptr(), g.data_ptr(), t.data_ptr(), table.data_ptr(), table.numel(), float(gamma),
                                            int(v), B, C, Ft, cond_f, H * W, loss.data_ptr(), sl.data_ptr(), w.data_ptr(),
                                            dp.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert torch.equal(p, pred) and torch.equal(g, target)                                      # the inputs are only read
    for view, hold, s in ((p, hp, shift), (g, hg, shift), (dp, hdp, shift), (loss, hl, 0), (sl, hsl, 0), (w, hw, 0), (ws, hws, 0)):
        assert _intact(view, hold, s)
    assert not torch.isnan(dp).any() and not torch.isnan(loss).any() and not torch.isnan(sl).any() and not torch.isnan(w).any()
    return loss, dp, sl, w


def _ints(shape, seed, device, lo=-8, hi=9):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)).float().to(device)


def _randn(shape, seed, device):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(device)


# ---- 1. exact ---------------------------------------------------------------------------------------------------------------------------
# (v, gamma, timesteps): entries 0 and 1, out-of-range values (clamped to entries 0 and 4), weights that differ between the samples
# and per-sample data of very different size (below) -- two samples' weights or partial rows swapped would change the outputs
EXACT = [(0, 0.5, [2, -3, 3, 1]), (1, 5.0, [2, 3, 2 ** 40, 0]), (1, 1.0, [4, 1, 7, 2]), (0, 5.0, [1, 0, 1, 3])]


@pytest.mark.parametrize("cond_f", [0, 1])
@pytest.mark.parametrize("B", [2, 4])
@pytest.mark.parametrize("v,gamma,ts", EXACT, ids=lambda x: str(x).replace(" ", ""))
def test_exact_on_small_integers(device, v, gamma, ts, B, cond_f):
    """C = 4, F_total = 3, HW = 16; small integers, sample b scaled by b + 1: every square, every partial sum and every weighted term is
    exact, so loss, sample_loss and weights are the float64 definition's bits whatever the order.  dpred is the header's three fp32
    products ((2 d) inv_n) w_b to the bit (tests/minsnr_ref.stated32); with cond_f = 1, B n_s is a power of two, inv_n is exact and that
    IS the float64 definition rounded once (asserted); with cond_f = 0 (n_s = 192) inv_n = (float)(1 / (B 192)) carries a rounding and
    the definition is met within 3 * 2^-24 relative -- inv_n, and the two inexact products."""
    C, Ft, HW = 4, 3, 16
    table = torch.tensor(EXACT_TABLE, device=device)
    t = torch.tensor(ts[:B], device=device)
    scale = torch.arange(1, B + 1, device=device).float().view(B, 1, 1, 1, 1)
    pred = _ints((B, C, Ft, HW, 1), 5, device) * scale
    target = _ints((B, C, Ft - cond_f, HW, 1), 6, device) * scale
    loss, dpred, sl, w = _call(pred, target, t, table, cond_f, gamma, v)
    w64 = M.weights64(t, table, gamma, bool(v))
    assert _bits(w, M.weights32(t, table, gamma, bool(v))) and set(w64.tolist()) <= {0.0, 0.1875, 0.25, 0.5, 0.8125, 1.0}
    l64, s64, d64 = M.snr_mse64(pred, target, t, table, cond_f, gamma, bool(v))
    assert _bits(sl, s64.float()) and _bits(loss, l64.float().reshape(1))
    l32, s32, d32 = M.stated32(pred, target, t, table, cond_f, gamma, bool(v))
    assert _bits(loss, l32) and _bits(sl, s32) and _bits(dpred, d32)
    if cond_f:
        assert _bits(dpred, d64.float())
        assert torch.equal(dpred[:, :, :cond_f].cpu().view(torch.int32), torch.zeros((B, C, cond_f, HW, 1), dtype=torch.int32))   # +0.0
    else:
        assert ((dpred.double().cpu() - d64).abs() <= 3 * U * d64.abs()).all()
    assert len(set(sl.tolist())) == B and float(loss) > 0    # no two samples alike
    # the wrapper: same bits, caller-owned buffers honoured
    mine_s, mine_w = torch.full((B,), NAN, device=device), torch.full((B,), NAN, device=device)
    out = train_ops.snr_mse_loss_grad(pred, target, t, table, cond_f, gamma, bool(v), sample_loss=mine_s, weights=mine_w)
    assert out[2] is mine_s and out[3] is mine_w
    assert _bits(out[0], loss) and _bits(out[1], dpred) and _bits(mine_s, sl) and _bits(mine_w, w)


# ---- 2. edges ---------------------------------------------------------------------------------------------------------------------------
# (C, F_total, cond_f, HW, shift).  HW = 1 and 15: the scalar path (15: a tail behind the last full block trip); 1030 = 4 * 257 + 2 is no
# multiple of 4 either: scalar, 8240 elements per sample in 33 blocks; 1028: the 16-byte path, and from a base 4 bytes behind a 16-byte
# boundary the scalar path on the same shape; (4, 5, 1, 1030): 20600 > CAP * 256 elements per sample, every block of the scalar path
# makes two trips; (4, 5, 2, 3280): 65600 > 4 * CAP * 256, the same for the 16-byte path
EDGES = [(4, 3, 1, 1, 0), (4, 3, 1, 15, 0), (2, 4, 1, 1030, 0), (4, 3, 1, 1028, 0), (4, 3, 1, 1028, 1), (4, 3, 0, 1028, 0),
         (4, 5, 1, 1030, 0), (4, 5, 2, 3280, 0)]


@pytest.mark.parametrize("v", [0, 1])
@pytest.mark.parametrize("case", EDGES, ids=lambda c: "x".join(map(str, c)))
def test_edges_against_float64(device, case, v):
    """B = 3, normal data, the DDPM table, gamma = 5, timesteps inside and (second vector) outside the table.  Against the float64
    definition on the fp32 difference d (tests/minsnr_ref.snr_mse64), relative, every term of a sum being >= 0:
      weights      the bits of the numpy float64 expression cast to fp32
      sample_loss  2 * 2^-24 + 2^-30: the fp32 rounding of d * d, the rounding of the result; the double sums and the product with
                   1 / n_s stay below n_s * 2^-53 + 2^-52 < 2^-30 together
      loss         the same: its terms carry the rounding of d * d, the result is rounded once, double arithmetic between
      dpred        3 * 2^-24 (+ 2^-149): 2.0f * d is exact, inv_n = (float)(1 / (B n_s)) is rounded, and so are the products with
                   inv_n and with w_b -- and, stricter, the bits of those three fp32 products (tests/minsnr_ref.stated32)
    all under 8 * 2^-24, beyond which the arithmetic would not be what the header says; +0.0 on the conditioning frames by bit pattern"""
    C, Ft, cond_f, HW, shift = case
    B, gamma = 3, 5.0
    table = ddpm_alphas_cumprod().to(device)
    T = table.numel()
    pred, target = _randn((B, C, Ft, HW, 1), 7, device), _randn((B, C, Ft - cond_f, HW, 1), 8, device)
    target[1] *= 3.0                                         # three samples of three sizes
    target[2] *= 0.25
    for ts in ([30, 100, T - 1], [-5, T + 3, 80]):
        t = torch.tensor(ts, device=device)
        loss, dpred, sl, w = _call(pred, target, t, table, cond_f, gamma, v, shift)
        assert _bits(w, M.weights32(t, table, gamma, bool(v))) and len(set(w.tolist())) == 3
        l64, s64, d64 = M.snr_mse64(pred, target, t, table, cond_f, gamma, bool(v))
        rel = 2 * U + 2.0 ** -30
        e_s = ((sl.double().cpu() - s64).abs() / s64).max()
        e_l = (loss.double().cpu()[0] - l64).abs() / l64
        e_d = (dpred.double().cpu() - d64).abs()
        print(f"[minsnr] {case} v={v} t={ts}: sample_loss {float(e_s) / U:.3f}, loss {float(e_l) / U:.3f} (allowed {rel / U:.3f}), dpred "
              f"{float((e_d / (d64.abs() + 2.0 ** -126)).max()) / U:.3f} (allowed 3) x 2^-24")
        assert e_s <= rel and e_l <= rel and (e_d <= 3 * U * d64.abs() + 2.0 ** -149).all()
        assert _bits(dpred, M.stated32(pred, target, t, table, cond_f, gamma, bool(v))[2])
        if cond_f:
            assert int(dpred[:, :, :cond_f].contiguous().view(torch.int32).abs().max()) == 0


# ---- 3. neutral weight -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(4, 3, 1, 1028, 0), (4, 3, 1, 15, 0), (4, 5, 2, 3280, 0)], ids=lambda c: "x".join(map(str, c)))
def test_weight_one_gives_the_dpred_of_the_plain_loss(device, case):
    """eps-model, gamma = 5, timesteps whose SNR is at most gamma: every weight is exactly 1, dpred is seer_mse_loss_grad's bit for bit
    (one more product, by 1.0f), and the loss is the plain mean within the bound of test_edges_against_float64"""
    C, Ft, cond_f, HW, shift = case
    B, gamma = 3, 5.0
    table = ddpm_alphas_cumprod().to(device)
    t = torch.tensor([999, 600, 300], device=device)
    a = table[t].double().cpu()
    assert (gamma * (1 - a) / a >= 1).all()
    pred, target = _randn((B, C, Ft, HW, 1), 9, device), _randn((B, C, Ft - cond_f, HW, 1), 10, device)
    loss, dpred, sl, w = _call(pred, target, t, table, cond_f, gamma, 0, shift)
    assert _bits(w, torch.ones(B))
    plain_loss, plain_dpred = train_ops.mse_loss_grad(pred, target, cond_f)
    assert _bits(dpred, plain_dpred)
    mean64 = ((pred[:, :, cond_f:] - target).double() ** 2).mean().cpu()
    assert (loss.double().cpu()[0] - mean64).abs() <= (2 * U + 2.0 ** -30) * mean64
    assert (plain_loss.double().cpu()[0] - mean64).abs() <= 1e-4 * mean64          # (the plain loss adds in fp32: only loosely the same)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_einval_and_touch_nothing(device):
    lib = _lib.load()
    buf = torch.full((8192,), NAN, device=device)
    ts = torch.full((4,), 3, dtype=torch.int64, device=device)
    ws = torch.full((2 * CAP + 2,), NAN, device=device, dtype=torch.float64)
    assert buf.data_ptr() % 16 == 0 and ts.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0
    n = 0
    for args, why in M.refusal_cases(buf.data_ptr(), ts.data_ptr(), ws.data_ptr()):
        assert lib.seer_snr_mse_loss_grad(*args, torch.cuda.current_stream().cuda_stream) == -22, why
        n += 1
    torch.cuda.synchronize()
    assert n >= 50 and torch.isnan(buf).all() and torch.isnan(ws).all() and bool((ts == 3).all())
    # and the good call of that list is one: it returns 0 and writes exactly its outputs
    args = next(iter(M.refusal_cases(buf.data_ptr(), ts.data_ptr(), ws.data_ptr())))[0]
    good = (buf.data_ptr(),) + args[1:]                  # (the first case is pred = NULL)
    buf[:768] = 1.0                                      # pred, target
    buf[1024:1034] = 0.5                                 # the table
    assert lib.seer_snr_mse_loss_grad(*good, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    written = ~torch.isnan(buf)
    want = torch.zeros(8192, dtype=torch.bool, device=device)
    for lo, hi in ((0, 768), (1024, 1034), (2048, 2049), (2052, 2054), (2056, 2058), (4096, 4096 + 384)):
        want[lo:hi] = True
    assert torch.equal(written, want) and float(buf[2048]) == 0.0 and buf[2056:2058].tolist() == [1.0, 1.0]
    # the wrapper's own refusals
    p, g = torch.zeros((2, 4, 3, 4, 4), device=device), torch.zeros((2, 4, 2, 4, 4), device=device)
    t, table = torch.zeros((2,), dtype=torch.int64, device=device), torch.full((10,), 0.5, device=device)
    for bad in (dict(target=g[:, :, :1].contiguous()), dict(timesteps=t[:1]), dict(timesteps=t.int()), dict(alphas_cumprod=table.double()),
                dict(alphas_cumprod=table.cpu()), dict(sample_loss=torch.zeros(3, device=device)), dict(weights=torch.zeros(2, device=device).double())):
        kw = {**dict(pred=p, target=g, timesteps=t, alphas_cumprod=table, cond_f=1, snr_gamma=5.0), **bad}
        with pytest.raises((AssertionError, TypeError, _lib.SeerHipError)):
            train_ops.snr_mse_loss_grad(**kw)
    with pytest.raises(_lib.SeerHipError):
        train_ops.snr_mse_loss_grad(p, g, t, table, 1, float("inf"))


# ---- 5. the trainer ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(device):
    """the models of tests/test_gpu_train_batch.py, this module's own instances"""
    from seervideoldm_amd import AutoencoderKL, FSTextTransformer, SeerUNet, synth
    from seervideoldm_amd.vae import ldm_to_diffusers_vae
    from tests.test_gpu_train_batch import CFG_MINI, FR, FS, StubTextEncoder, T
    unet = SeerUNet(**CFG_MINI).to(device)
    unet.load_state_dict(synth.synth_state_dict(synth.unet_param_shapes(CFG_MINI), device=device), strict=True)
    fst = FSTextTransformer(num_frames=FS["num_frames"], in_channels=192, out_channels=192, n_heads=2, num_layers=1,
                            cross_attention_dim=192).to(device)
    fst.load_state_dict(synth.synth_state_dict(synth.fstext_param_shapes(**FS), device=device), strict=True)
    fst.set_numframe(FR)
    vae = AutoencoderKL(block_out_channels=(128, 128, 256, 256), layers_per_block=1)
    vae.load_state_dict(ldm_to_diffusers_vae(synth.synth_state_dict(synth.vae_encoder_param_shapes(
        ch=128, ch_mult=(1, 1, 2, 2), num_res_blocks=1, z_channels=4)), 4), strict=True)
    return dict(unet=unet, fst=fst, vae=vae.to(device), text=StubTextEncoder(device), acp=ddpm_alphas_cumprod(T))


class _FedBackend:
    """train_ops, except that mse_loss_grad hands back what it was given to hand back -- after checking that it was asked about the
    same prediction"""

    def __init__(self, pred, loss, dpred):
        self.fed, self.asked = (pred, loss, dpred), 0

    def __getattr__(self, name):
        return getattr(train_ops, name)

    def mse_loss_grad(self, pred, target, cond_f):
        assert torch.equal(pred, self.fed[0])
        self.asked += 1
        return self.fed[1], self.fed[2]


@pytest.mark.parametrize("ptype", ["epsilon", "v_prediction"])
def test_step_from_batch_is_a_twin_fed_the_kernels_dpred(device, world, ptype):
    """snr_gamma = 5, timesteps [0, T - 1] (the two ends of the table).  The step equals, bit for bit in loss and both gradient segments,
    the forward_backward of a twin WITHOUT snr_gamma whose loss entry returns train_ops.snr_mse_loss_grad's (loss, dpred) computed from
    the first trainer's last_pred; last_sample_loss / last_loss_weights are that direct call's; the unweighted step differs"""
    from tests.test_gpu_train_batch import B, FR, HP, PIX, T, _batch
    cond, gamma, v = 2, 5.0, ptype == "v_prediction"
    acp = world["acp"]
    batch, inj = _batch(71, cond, device, [0, T - 1])
    kw = dict(vae=world["vae"], text_encoder=world["text"], cond_frames=cond, alphas_cumprod=acp, **inj)
    make = lambda **k: SeerTrainer(world["unet"], world["fst"], gradient_accumulation_steps=2, prediction_type=ptype, **HP, **k)
    tr = make(snr_gamma=gamma)
    loss = tr.step_from_batch(*batch, **kw)
    model_input, noise, t, text = tr.last_inputs
    assert t.tolist() == [0, T - 1] and tr._snr_acp.is_cuda and torch.equal(tr._snr_acp.cpu(), acp)
    target = noise
    if v:
        frames = batch[0].to(device).permute(0, 2, 1, 3, 4).reshape(B * FR, 3, PIX, PIX)
        latents = torch.empty_like(noise)
        train_ops.train_inputs(world["vae"].encode(frames).latent_dist.parameters.contiguous(), inj["posterior_noise"], noise, t,
                               acp.to(device), cond, latents=latents)
        target = train_ops.velocity_target(latents, noise, t, acp.to(device))
    l2, dpred, sl, w = train_ops.snr_mse_loss_grad(tr.last_pred, target, t, acp.to(device), cond, gamma, v)
    assert _bits(loss, l2) and _bits(tr.last_sample_loss, sl) and _bits(tr.last_loss_weights, w) and torch.isfinite(loss).all()
    assert _bits(w, M.weights32(t, acp, gamma, v)) and w[0] != w[1]
    fed = _FedBackend(tr.last_pred, l2, dpred)
    twin = make(tops=fed)
    loss2 = twin.forward_backward(model_input, target, t, text, cond)
    assert fed.asked == 1 and torch.equal(loss, loss2)
    assert torch.equal(tr.pu.g, twin.pu.g) and torch.equal(tr.pf.g, twin.pf.g) and bool(tr.pu.g.abs().sum() > 0)
    flat = make()
    assert not torch.equal(flat.step_from_batch(*batch, **kw), loss) and not torch.equal(flat.pu.g, tr.pu.g)
    assert flat.last_sample_loss is None and tr.step_count == 0
    # the weighted loss is the weighted mean of what it reports
    want = (w.double() * sl.double()).mean()
    assert abs(float(loss) - float(want)) <= 4 * U * float(want)


def test_captured_step_replays_with_new_timesteps(device, world):
    """use_graph=True, a v-model: three calls with three batches and three timestep vectors, each a replay of the graphs the first call
    captured (one key, the same graph objects, the same static outputs), each equal to the eager trainer's call bit for bit -- loss,
    last_sample_loss, last_loss_weights, both gradient segments and the parameters after the optimizer step.  The weights differ from
    call to call: the kernel read the timesteps from device memory."""
    from tests.test_gpu_train_batch import HP, T, _batch
    cond, gamma = 2, 5.0
    steps = [[417, 93], [5, 800], [T - 1, 0]]
    batches = [_batch(81 + i, cond, device, ts) for i, ts in enumerate(steps)]
    runs = []
    for use_graph in (False, True):
        tr = SeerTrainer(world["unet"], world["fst"], prediction_type="v_prediction", snr_gamma=gamma, **HP)
        out, captured = [], None
        for batch, inj in batches:
            loss = tr.step_from_batch(*batch, vae=world["vae"], text_encoder=world["text"], cond_frames=cond, alphas_cumprod=world["acp"],
                                      use_graph=use_graph, **inj)
            out.append([x.clone() for x in (loss, tr.last_sample_loss, tr.last_loss_weights, tr.pu.g, tr.pf.g, tr.pu.p, tr.pf.p)])
            if use_graph:
                assert not tr._graph_broken and len(tr._graphs) == 1
                g = next(iter(tr._graphs.values()))
                mine = (g[0], g[1], tr.last_sample_loss.data_ptr(), tr.last_loss_weights.data_ptr(), loss.data_ptr())
                captured = captured or mine
                assert all(a is b if not isinstance(a, int) else a == b for a, b in zip(mine, captured))     # nothing re-captured
            else:
                assert tr._graphs == {}
        runs.append(out)
    for k, (eager, graph) in enumerate(zip(*runs)):
        assert all(torch.equal(a, b) for a, b in zip(eager, graph)), k
        assert _bits(eager[2], M.weights32(torch.tensor(steps[k]), world["acp"], gamma, True))
    assert len({tuple(o[2].tolist()) for o in runs[1]}) == 3
