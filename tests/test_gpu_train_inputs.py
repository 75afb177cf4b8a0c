"""seer_train_inputs alone, on synthetic encoder moments: every output element against the float64 evaluation of the formula from
the same fp32 inputs (tests/train_inputs_ref.py), the posterior sample against seer_gaussian_sample bit for bit, and the layout
(nothing outside the outputs written, everything inside written).

The bound per element is 2^-20 * (sqrt(a) * scale * (|mean| + |std * eps|) + sqrt(1 - a) * |noise|): each term passes through at
most eight fp32 operations of at most 1 ulp each (expf taken at 2), and 2^-20 is sixteen half-ulps.  It is derived, not tuned.  Where the
budget goes at the clamp edges: the kernel's exponential is exp2(x * log2 e) with x * log2 e rounded to fp32; at logvar = -30
(x = -15, |x log2 e| = 21.6, half an ulp of that times ln 2) that rounding alone is 5.1 * 2^-23 of std = 3.1e-7, at logvar = 20
(x = 10) 0.3 * 2^-23 -- the std * eps term is then inside its own sixteen half-ulps unless |mean| < 2e-8 * |eps|, and the means here
are standard normal."""
import functools

import pytest
import torch

from seervideoldm_amd import ops, train_ops
from seervideoldm_amd.trainer import ddpm_alphas_cumprod
from tests.train_inputs_ref import reference, worst_ratio

pytestmark = pytest.mark.gpu

SCALE = 0.18215
T = 1000
# (b, f1, f2, C, h, w): HW = 64 -> the 16-byte path (twice: two and one conditioning frame), HW = 25 -> the scalar path, b = 1, HW = 4
# = one 16-byte access per row and three videos
SHAPES = [(2, 2, 2, 4, 8, 8), (2, 1, 3, 4, 8, 8), (1, 2, 1, 4, 5, 5), (3, 1, 1, 4, 2, 2)]
TIMESTEPS = {2: [0, T - 1], 1: [T - 1], 3: [T - 1, 0, 417]}
TIMESTEPS_B = {(2, 1, 3, 4, 8, 8): [T - 1, 417], (1, 2, 1, 4, 5, 5): [0]}
EDGES = [-40.0, -30.0, 0.0, 20.0, 25.0]                 # below / at the lower clamp, the middle, at / above the upper clamp


@functools.lru_cache(maxsize=None)
def _case(shape):
    """seeded CPU inputs of one shape and their float64 reference (shared by the tests, never modified)"""
    b, f1, f2, C, h, w = shape
    F = f1 + f2
    g = torch.Generator().manual_seed(1000 + sum(shape))
    mom = torch.randn((b * F, 2 * C, h, w), generator=g)
    lv = mom[:, C:].reshape(-1)                          # (a copy: the slice is not contiguous)
    for k, v in enumerate(EDGES):                        # every seventh logvar is a clamp-edge value, all five in every case
        lv[k * 7::35] = v
    mom[:, C:] = lv.view(b * F, C, h, w)
    eps = torch.randn((b * F, C, h, w), generator=g)
    noise = torch.randn((b, C, f2, h, w), generator=g)
    t = torch.tensor(TIMESTEPS_B.get(shape, TIMESTEPS[b]), dtype=torch.int64)
    acp = ddpm_alphas_cumprod(T)
    assert all(bool((mom[:, C:] == v).any()) for v in EDGES) and (b == 1 or len(set(t.tolist())) > 1)
    return dict(mom=mom, eps=eps, noise=noise, t=t, acp=acp, ref=reference(mom, eps, noise, t, acp, f1, SCALE),
                ref_mean=reference(mom, None, noise, t, acp, f1, SCALE))


def _framed(shape, device, pad):
    """a tensor of `shape` inside a larger NaN-filled buffer, `pad` floats from its start"""
    n = 1
    for s in shape:
        n *= s
    big = torch.full((n + 2 * pad,), float("nan"), device=device)
    return big, big[pad:pad + n].view(shape)


def _run(case, shape, device, *, eps=True, want_latents=True, pad=64, scale=SCALE):
    b, f1, f2, C, h, w = shape
    d = lambda k: case[k].to(device)
    bx, x = _framed((b, C, f1 + f2, h, w), device, pad)
    bl, lat = _framed((b, C, f2, h, w), device, pad)
    out = train_ops.train_inputs(d("mom"), d("eps") if eps else None, d("noise"), d("t"), d("acp"), f1, scale, out=x,
                                 latents=lat if want_latents else None)
    assert out.data_ptr() == x.data_ptr()
    torch.cuda.synchronize()
    for big, inner, written in ((bx, x, True), (bl, lat, want_latents)):
        assert bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[pad + inner.numel():]).all()), "wrote outside the output"
        assert bool(torch.isfinite(inner).all()) if written else bool(torch.isnan(inner).all())
    return x, lat


@pytest.mark.parametrize("shape", SHAPES)
def test_every_element_meets_the_float64_formula(device, shape):
    case = _case(shape)
    f1 = shape[1]
    x, lat = _run(case, shape, device)
    rx, rl, bound, lbound = case["ref"]
    r_all, r_cond = worst_ratio(x, rx, bound), worst_ratio(x[:, :, :f1], rx[:, :, :f1], bound[:, :, :f1])
    r_lat = worst_ratio(lat, rl, lbound)
    print(f"{shape}: worst |err| / bound: model_input {r_all:.3f}, its conditioning frames {r_cond:.3f}, clean latents {r_lat:.3f}")
    assert r_all <= 1.0 and r_cond <= 1.0 and r_lat <= 1.0


@pytest.mark.parametrize("shape", SHAPES[:1] + SHAPES[2:3])
def test_posterior_mean_when_no_noise_is_given(device, shape):
    case = _case(shape)
    x, lat = _run(case, shape, device, eps=False)
    rx, rl, bound, lbound = case["ref_mean"]
    r, r_lat = worst_ratio(x, rx, bound), worst_ratio(lat, rl, lbound)
    print(f"{shape}: eps_post = None: worst |err| / bound: model_input {r:.3f}, clean latents {r_lat:.3f}")
    assert r <= 1.0 and r_lat <= 1.0


@pytest.mark.parametrize("shape", SHAPES)
def test_sample_is_gaussian_sample_bit_for_bit(device, shape):
    """at latent_scale = 1 the clean latents and the conditioning frames ARE z: the bits of ops.gaussian_sample on the same inputs"""
    case = _case(shape)
    b, f1, f2, C, h, w = shape
    x, lat = _run(case, shape, device, scale=1.0)
    z = ops.gaussian_sample(case["mom"].to(device), case["eps"].to(device)).view(b, f1 + f2, C, h, w).permute(0, 2, 1, 3, 4)
    assert torch.equal(x[:, :, :f1], z[:, :, :f1]) and torch.equal(lat, z[:, :, f1:])


@pytest.mark.parametrize("shape", SHAPES)
def test_latents_are_optional_and_paths_agree(device, shape):
    """latents = None leaves model_input identical; outputs 12 bytes off a 16-byte boundary take the scalar path and give the same bits
    as the 16-byte path"""
    case = _case(shape)
    x, lat = _run(case, shape, device)
    x2, _ = _run(case, shape, device, want_latents=False)
    x3, lat3 = _run(case, shape, device, pad=3)
    assert torch.equal(x, x2) and torch.equal(x, x3) and torch.equal(lat, lat3)


def _offset(t, floats):
    """a copy of `t` whose first element lies `floats` floats behind a 16-byte boundary (allocations start on one)"""
    big = torch.empty((t.numel() + floats,), device=t.device, dtype=t.dtype)
    assert big.data_ptr() % 16 == 0
    v = big[floats:].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("which,floats", [("mom", 1), ("eps", 3), ("noise", 1)])
def test_an_input_off_the_16_byte_boundary_takes_the_scalar_path(device, which, floats):
    """HW = 64 with ONE input base 4 or 12 bytes off a 16-byte boundary (outputs aligned): the scalar path, and the bits of the
    16-byte path"""
    shape = SHAPES[0]
    case = _case(shape)
    x, lat = _run(case, shape, device)
    moved = dict(case)
    moved[which] = _offset(case[which].to(device), floats)
    assert moved[which].data_ptr() % 16 == 4 * floats and moved[which].is_contiguous()
    x2, lat2 = _run(moved, shape, device)
    assert torch.equal(x, x2) and torch.equal(lat, lat2)


def test_timesteps_outside_the_table_are_rejected_before_launch(device):
    shape = SHAPES[0]
    case = _case(shape)
    d = lambda k: case[k].to(device)
    for bad in ([0, T], [-1, 5]):
        with pytest.raises(ValueError):
            train_ops.train_inputs(d("mom"), d("eps"), d("noise"), torch.tensor(bad, device=device), d("acp"), shape[1], SCALE)
