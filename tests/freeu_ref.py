"""TEST INFRASTRUCTURE ONLY -- FreeU (Si et al., CVPR 2024) restated for the tests of seer_freeu / SeerUNet.enable_freeu.

    fourier_filter_fft(x, s)             diffusers' fourier_filter (threshold 1) with torch.fft, float64, last two dimensions
    twiddles(N)                          cos / sin of 2 pi k / N in float64, exact at the multiples of a quarter turn
    freeu_closed_form(x, s, dtype)       the residue-set form the kernel evaluates, in `dtype` arithmetic (float64 or float32)
    rnd64(x, dtype)                      float64 -> bf16 / fp16 in one rounding, as float64
    backbone_scale(x, b)                 the first half of the channels (dimension 1) times b
    patched_oracle(params, cfg)          context manager: oracle.seer_oracle.resnet_block with FreeU in front of the resnets of
                                         up_blocks.0 / up_blocks.1 (the oracle's file is not edited)
    TorchOpsWithFreeu / RecordingFreeu   tests/torch_ops_backend.py plus `freeu` (that file is not edited), and a recorder of its calls
"""
import contextlib
import math

import torch

from oracle import seer_oracle as O
from tests import torch_ops_backend as tob


def fourier_filter_fft(x, s):
    """Re ifft2(mask * fft2(x)) over the last two dimensions in float64: the mask is s on the fft-shifted index block
    [H//2 - 1 : H//2 + 1, W//2 - 1 : W//2 + 1] and 1 elsewhere (diffusers.utils.torch_utils.fourier_filter, threshold = 1)."""
    H, W = x.shape[-2:]
    xf = torch.fft.fftshift(torch.fft.fftn(x.double(), dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(xf.shape, dtype=torch.float64)
    mask[..., max(H // 2 - 1, 0):H // 2 + 1, max(W // 2 - 1, 0):W // 2 + 1] = s
    xf = torch.fft.ifftshift(xf * mask, dim=(-2, -1))
    return torch.fft.ifftn(xf, dim=(-2, -1)).real


def twiddles(N, snap=True):
    """(cos, sin) of 2 pi k / N, k = 0 .. N - 1, float64; snap: the index is reduced first, so a multiple of a quarter turn gives
    exactly 0 or +-1"""
    c, s = [], []
    for k in range(N):
        if snap and (4 * k) % N == 0:
            q = 4 * k // N
            c.append((1.0, 0.0, -1.0, 0.0)[q]); s.append((0.0, 1.0, 0.0, -1.0)[q])
        else:
            c.append(math.cos(2.0 * math.pi * k / N)); s.append(math.sin(2.0 * math.pi * k / N))
    return torch.tensor(c, dtype=torch.float64), torch.tensor(s, dtype=torch.float64)


def residues(N):
    """K_N: the distinct values of {0, -1 mod N}"""
    return sorted({0, (-1) % N})


def freeu_closed_form(x, s, dtype=torch.float64, snap=True):
    """x + (s - 1) / (H W) * sum_{kh in K_H, kw in K_W} Re(X[kh, kw] e^{+2 pi i (kh h / H + kw w / W)}) over the last two dimensions,
    every operation in `dtype` (the table is made in float64 and cast, as the product's is); complex numbers as (re, im) pairs"""
    H, W = x.shape[-2:]
    x = x.to(dtype)
    (cH, sH), (cW, sW) = twiddles(H, snap), twiddles(W, snap)
    cH, sH, cW, sW = (t.to(dtype) for t in (cH, sH, cW, sW))
    hh, ww = torch.arange(H), torch.arange(W)
    P = torch.zeros_like(x)
    for kh in residues(H):
        for kw in residues(W):
            # e^{-2 pi i kh h / H} = (cos, -sin) of the table at index kh h mod H
            ch, sh = cH[(kh * hh) % H][:, None], sH[(kh * hh) % H][:, None]
            cw, sw = cW[(kw * ww) % W][None, :], sW[(kw * ww) % W][None, :]
            cr, ci = ch * cw - sh * sw, sh * cw + ch * sw          # cos, sin of the summed angle
            Xr = (x * cr).sum(dim=(-2, -1), keepdim=True)
            Xi = -(x * ci).sum(dim=(-2, -1), keepdim=True)
            P = P + (Xr * cr - Xi * ci)                             # Re((Xr + i Xi)(cr + i ci))
    g = (torch.tensor(s, dtype=dtype) - 1) / (H * W)
    return x + g * P


def rnd64(x, dtype):
    """float64 -> the nearest value of the 16-bit storage type (ties to even), returned in float64, in ONE rounding (torch's
    conversion goes through fp32: two roundings).  Finite inputs inside the type's range."""
    p, emin = (8, -125) if dtype == torch.bfloat16 else (11, -13)      # significand bits; frexp exponent of the least normal number
    _, e = torch.frexp(x)
    e = e.clamp_min(emin).to(torch.int32)
    return torch.ldexp(torch.round(torch.ldexp(x, p - e)), e - p)


def backbone_scale(x, b):
    y = x.clone()
    half = x.shape[1] // 2
    y[:, :half] = x[:, :half] * b
    return y


def backbone_channels(cfg, p):
    """channels of the backbone input of resnet `p` = up_blocks.<i>.resnets.<j>: the previous stage's width for j = 0 (the mid block's
    for i = 0), else the stage's own"""
    parts = p.split(".")
    i, j = int(parts[1]), int(parts[3])
    rev = tuple(cfg["block_out_channels"])[::-1]
    return rev[max(i - 1, 0)] if j == 0 else rev[i]


@contextlib.contextmanager
def patched_oracle(params, cfg):
    """oracle.seer_oracle.resnet_block with FreeU (params = (s1, s2, b1, b2)) applied to the concatenated 5-D input [B, C, F, H, W] of
    every resnet under up_blocks.0. / up_blocks.1.: split at the backbone channel count, the definition per frame, the original"""
    s1, s2, b1, b2 = params
    real = O.resnet_block

    def resnet_block(sd, p, x, temb, groups, eps):
        stage = {"up_blocks.0.": (b1, s1), "up_blocks.1.": (b2, s2)}
        for prefix, (b, s) in stage.items():
            if p.startswith(prefix):
                Cx = backbone_channels(cfg, p)
                back, skip = x[:, :Cx], x[:, Cx:]
                back = backbone_scale(back, b)
                skip = fourier_filter_fft(skip, s).to(x.dtype)          # the last two dimensions: per (batch, channel, frame) plane
                x = torch.cat([back, skip], dim=1)
        return real(sd, p, x, temb, groups, eps)
    O.resnet_block = resnet_block
    try:
        yield
    finally:
        O.resnet_block = real


def freeu_rows(x, skip, params, H, W):
    """the stand-in of ops.freeu on token-major [images * H * W, C] tensors: fp32 closed form, rounded to the storage type"""
    b, s = (float(v) for v in params.tolist())
    xo = so = None
    if x is not None:
        xo = x.clone()
        half = x.shape[1] // 2
        xo[:, :half] = (x[:, :half].float() * b).to(x.dtype)
    if skip is not None:
        C = skip.shape[1]
        planes = skip.float().reshape(-1, H, W, C).permute(0, 3, 1, 2).contiguous()   # (a plane's sums do not see the other planes)
        f = freeu_closed_form(planes, s, torch.float64 if tob.EXACT else torch.float32)
        so = f.permute(0, 2, 3, 1).reshape(-1, C).to(skip.dtype)
    return xo, so


class TorchOpsWithFreeu:
    """tests/torch_ops_backend.py with `freeu` added"""

    def __getattr__(self, name):
        return getattr(tob, name)

    def freeu(self, x, skip, params, H, W):
        return freeu_rows(x, skip, params, H, W)


class RecordingFreeu(TorchOpsWithFreeu):
    """... and every freeu call written down as (H, W, Cx, Cs, (b, s))"""

    def __init__(self):
        self.calls = []

    def freeu(self, x, skip, params, H, W):
        self.calls.append((H, W, x.shape[1], skip.shape[1], tuple(round(float(v), 6) for v in params.tolist())))
        return freeu_rows(x, skip, params, H, W)
