"""Min-SNR-gamma loss weighting restated (include/seer_hip.h: seer_snr_mse_loss_grad): the weights in numpy float64 -- the expressions
the kernel evaluates, operation for operation, so their cast to fp32 is the kernel's `weights` to the bit --, the loss, the per-sample
losses and dpred in float64 from the definition, and a torch stand-in with the signature of train_ops.snr_mse_loss_grad behind a
`tops=` backend that records its calls.  Nothing here comes from a kernel.

  * weights64(t, table, gamma, v): fmin(1, gamma (1 - a) / a) for an eps-model, fmin(a, gamma (1 - a)) for a v-model, a the fp32 table
    entry of the clamped timestep, gamma the fp32 value, both widened to float64;
  * textbook64: min(SNR, gamma) / SNR and min(SNR, gamma) / (SNR + 1) with SNR = a / (1 - a), what the forms above stand for;
  * snr_mse64: (loss, sample_loss [B], dpred) in float64; d is first taken as the fp32 difference pred - target (correctly rounded: it
    is what the kernel computes), everything behind it is float64;
  * snr_mse_loss_grad: the stand-in (any float dtype: the host tests check its dpred against autograd in float64);
  * train_ops(): tests/vpred_ref.train_ops() + the stand-in; `snr_calls` lists the arguments of every snr_mse_loss_grad call."""
import numpy as np
import torch

from tests import vpred_ref as V

f64 = torch.float64
U = V.U                                                  # 2^-24: the relative rounding error of one fp32 operation


def _a64(t, table):
    tab = table.detach().cpu().to(torch.float32).numpy().astype(np.float64)
    idx = np.clip(torch.as_tensor(t).detach().cpu().to(torch.int64).numpy(), 0, tab.shape[0] - 1)
    return tab[idx]


def weights64(t, table, gamma, v):
    """-> numpy float64 [B]; `.astype(numpy.float32)` of it is the kernel's `weights`, bit for bit"""
    a, g = _a64(t, table), np.float64(np.float32(gamma))
    with np.errstate(divide="ignore"):                  # a = 0: gamma / 0 = inf, and fmin(1, inf) = 1
        return np.minimum(a, g * (1.0 - a)) if v else np.minimum(1.0, g * (1.0 - a) / a)


def textbook64(t, table, gamma, v):
    """min(SNR, gamma) / SNR, or / (SNR + 1) for a v-model, as the paper writes them (0 < a < 1)"""
    a, g = _a64(t, table), np.float64(np.float32(gamma))
    snr = a / (1.0 - a)
    return np.minimum(snr, g) / (snr + 1.0 if v else snr)


def weights32(t, table, gamma, v):
    return torch.from_numpy(weights64(t, table, gamma, v).astype(np.float32))


def snr_mse64(pred, target, t, table, cond_f, gamma, v):
    """-> (loss [], sample_loss [B], dpred like pred) in float64 on the CPU, with the fp32-rounded weights the kernel applies:
    sample_loss_b = mean_e d^2 (unweighted), loss = mean_b w_b sample_loss_b, dpred = 2 d w_b / (B n_s), 0 on the conditioning frames"""
    pred, target = pred.detach().cpu().float(), target.detach().cpu().float()
    d = (pred[:, :, cond_f:] - target).double()          # the fp32 difference, widened
    B, n_s = d.shape[0], d[0].numel()
    w = weights32(t, table, gamma, v).double()
    sample = (d * d).reshape(B, -1).sum(1) / n_s
    dpred = torch.zeros(pred.shape, dtype=f64)
    dpred[:, :, cond_f:] = 2.0 * d / (B * n_s) * w.view(B, 1, 1, 1, 1)
    return (w * sample).sum() / B, sample, dpred


def stated32(pred, target, t, table, cond_f, gamma, v):
    """The header's arithmetic, operation for operation, in numpy -> (loss [1], sample_loss [B], dpred) as fp32 tensors.
    dpred = ((2.0f d) inv_n) w_b in fp32 products (numpy rounds each correctly, as the GPU does), inv_n = (float)(1.0 / (B n_s)): the
    kernel's bits for ANY input.  The sums are float64 sums of the rounded fp32 squares: sum_b is taken here in numpy's order, which is
    the kernel's result only where every partial sum is exact (small integers) -- elsewhere compare sample_loss and loss under a bound."""
    p, g = pred.detach().cpu().float().numpy(), target.detach().cpu().float().numpy()
    d = p[:, :, cond_f:] - g                             # fp32
    B, n_s = d.shape[0], d[0].size
    w = weights64(t, table, gamma, v).astype(np.float32)
    s = (d * d).astype(np.float64).reshape(B, -1).sum(1)
    sample = (s * (1.0 / np.float64(n_s))).astype(np.float32)
    total = np.float64(0.0)
    for b in range(B):                                   # in order; the quotient, the product and the sum each rounded once
        total = total + np.float64(w[b]) * (s[b] / np.float64(n_s))
    loss = np.float32(total / np.float64(B))
    inv_n = np.float32(1.0 / (np.float64(B) * np.float64(n_s)))
    dp = np.zeros(p.shape, dtype=np.float32)             # +0.0 on the conditioning frames
    dp[:, :, cond_f:] = ((np.float32(2.0) * d) * inv_n) * w.reshape(B, 1, 1, 1, 1)
    return torch.from_numpy(np.array([loss])), torch.from_numpy(sample), torch.from_numpy(dp)


def weighted_loss(pred, target, w, cond_f):
    """the definition as one differentiable torch expression in pred's dtype -> (loss [], sample_loss [B])"""
    sample = ((pred[:, :, cond_f:] - target) ** 2).mean([1, 2, 3, 4])
    return (w * sample).mean(), sample


def snr_mse_loss_grad(pred, target, timesteps, alphas_cumprod, cond_f, snr_gamma, v_prediction=False, *, sample_loss=None,
                      weights=None):
    """train_ops.snr_mse_loss_grad in plain torch, in pred's dtype -> (loss [1], dpred, sample_loss [B], weights [B])"""
    B = pred.shape[0]
    assert target.shape == (B, pred.shape[1], pred.shape[2] - cond_f, *pred.shape[3:]) and tuple(timesteps.shape) == (B,)
    w = weights32(timesteps, alphas_cumprod, snr_gamma, bool(v_prediction)).to(pred.dtype)
    loss, sample = weighted_loss(pred.detach(), target, w, cond_f)
    d = pred.detach()[:, :, cond_f:] - target
    dpred = torch.zeros_like(pred)
    dpred[:, :, cond_f:] = 2.0 * d / (B * d[0].numel()) * w.view(B, 1, 1, 1, 1)
    outs = []
    for buf, val in ((sample_loss, sample), (weights, w)):
        if buf is None:
            outs.append(val)
        else:
            assert tuple(buf.shape) == (B,)
            buf.copy_(val)
            outs.append(buf)
    return loss.reshape(1), dpred, outs[0], outs[1]


def train_ops():
    """a `tops=` backend: tests/vpred_ref.train_ops() + snr_mse_loss_grad; `snr_calls` lists (pred, target, timesteps, alphas_cumprod,
    cond_f, snr_gamma, v_prediction) of every call"""
    base = V.train_ops()

    class TrainOps(type(base)):
        def __init__(self):
            super().__init__()
            self.snr_calls = []

        def snr_mse_loss_grad(self, pred, target, timesteps, alphas_cumprod, cond_f, snr_gamma, v_prediction=False, *,
                              sample_loss=None, weights=None):
            self.snr_calls.append((pred, target, timesteps, alphas_cumprod, cond_f, snr_gamma, v_prediction))
            return snr_mse_loss_grad(pred, target, timesteps, alphas_cumprod, cond_f, snr_gamma, v_prediction,
                                     sample_loss=sample_loss, weights=weights)
    return TrainOps()


def refusal_cases(P, T8, W8):
    """(arguments of seer_snr_mse_loss_grad without the stream, what is wrong) for every refusal the header lists.  P: a fp32 buffer of at
    least 8192 floats, T8: the int64 timesteps, W8: the float64 workspace (at least 2 * 64 doubles); all 16-byte aligned.  The good call
    (B = 2, C = 4, F_total = 3, cond_f = 1, HW = 16: 384 floats of pred) keeps its arrays apart inside P:
    pred at 0, target at 512, the table at 1024, loss at 2048, sample_loss at 2052, weights at 2056, dpred at 4096"""
    f = lambda n: P + 4 * n
    inf, nan = float("inf"), float("nan")
    good = dict(pred=f(0), target=f(512), timesteps=T8, alphas_cumprod=f(1024), T=10, snr_gamma=5.0, v_prediction=0, B=2, C=4, F_total=3,
                cond_f=1, HW=16, loss=f(2048), sample_loss=f(2052), weights=f(2056), dpred=f(4096), workspace=W8)
    cases = [dict(pred=None), dict(target=None), dict(timesteps=None), dict(alphas_cumprod=None), dict(loss=None),
             dict(sample_loss=None), dict(weights=None), dict(dpred=None), dict(workspace=None),
             dict(T=0), dict(T=-1), dict(B=0), dict(B=-2), dict(C=0), dict(C=-4), dict(F_total=0, cond_f=0), dict(F_total=-3), dict(HW=0),
             dict(HW=-16), dict(cond_f=-1), dict(cond_f=3), dict(cond_f=4), dict(B=65536),
             dict(snr_gamma=0.0), dict(snr_gamma=-5.0), dict(snr_gamma=inf), dict(snr_gamma=-inf), dict(snr_gamma=nan),
             dict(v_prediction=2), dict(v_prediction=-1),
             dict(pred=f(0) + 2), dict(target=f(512) + 1), dict(alphas_cumprod=f(1024) + 2), dict(loss=f(2048) + 3),
             dict(sample_loss=f(2052) + 1), dict(weights=f(2056) + 2), dict(dpred=f(4096) + 2), dict(timesteps=T8 + 4),
             dict(workspace=W8 + 4),
             dict(dpred=f(0)), dict(dpred=f(512)), dict(dpred=f(128)), dict(dpred=f(512 + 64)),        # dpred on / inside pred, target
             dict(loss=f(2052)), dict(loss=f(2057)), dict(sample_loss=f(2056)), dict(sample_loss=f(2055)), dict(loss=f(4096)),
             dict(weights=f(4096 + 383)), dict(sample_loss=f(4096 + 100)), dict(workspace=P + 4 * 4096), dict(workspace=P + 4 * 2048),
             dict(workspace=P + 4 * 2056)]
    for kw in cases:
        yield tuple({**good, **kw}.values()), kw
