"""The seeded noise of the sampler step, restated on the CPU (include/seer_hip.h, "seeded noise"; DESIGN.md, "Seeded noise").

  * philox4x32_10 / words: Philox4x32-10 in numpy integer arithmetic -- exact, checked against the Random123 known-answer vectors
    (KAT) in tests/test_stoch_host.py and, bit for bit, against seer_philox_u32 in tests/test_gpu_stoch.py;
  * normals64: the normals in float64 from the same uniforms -- what the device's fp32 Box-Muller is measured against;
  * philox_normal, cfg_ddim_step_rng, slot_cfg_ddim_step_rng (and slot_step_begin from tests/slot_ref.py): a torch stand-in with the
    signatures of seervideoldm_amd.ops, on tensors of any device, so that `SlotSampler(stochastic=True, ops=tests.stoch_ref)` runs the
    host logic on the CPU.  The normals are normals64 rounded to fp32 and the update is fp32 torch arithmetic in the kernel's
    expression order: equal to the kernels to rounding, not to the bit."""
import numpy as np
import torch

from tests.slot_ref import slot_step_begin  # noqa: F401  (the first kernel of the step is unchanged)

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
STREAM_START, STREAM_STEP = 0, 1
MAX_ABS_NORMAL = 5.7682                 # sqrt(-2 ln 2^-24) = 5.76813...: the largest |n| the map can give

# Random123's kat_vectors for philox4x32 with 10 rounds: (counter, key, output)
KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints -> uint32 [..., 4]"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)          # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def words(seed, stream, index, first_block, n_blocks):
    """what seer_philox_u32 writes: uint32 [n_blocks, 4]; key (seed lo, seed hi), counter (block, index, stream lo, stream hi)"""
    seed, stream = int(seed), int(stream)
    blocks = np.arange(int(first_block), int(first_block) + int(n_blocks), dtype=np.uint64)
    assert blocks[-1] <= MASK
    z = np.zeros_like(blocks)
    return philox4x32_10((blocks, z + np.uint64(int(index) & MASK), z + np.uint64(stream & MASK), z + np.uint64(stream >> 32)),
                         (seed & MASK, seed >> 32))


def uniforms(w):
    """u = (2 (w >> 9) + 1) 2^-24: a 24-bit odd numerator, exact in fp32 and in float64"""
    return (2.0 * (np.asarray(w, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -24


def normals64(seed, stream, index, n):
    """the first n normals of (seed, stream, index) in float64: Box-Muller on (w0, w1) and (w2, w3) of every block"""
    u = uniforms(words(seed, stream, index, 0, (int(n) + 3) // 4))
    out = np.empty(u.shape, dtype=np.float64)
    for a in (0, 2):
        r, ang = np.sqrt(-2.0 * np.log(u[:, a])), 2.0 * np.pi * u[:, a + 1]
        out[:, a], out[:, a + 1] = r * np.cos(ang), r * np.sin(ang)
    return out.reshape(-1)[:int(n)]


def seed_of(words32) -> int:
    """(lo, hi) int32 words (ops.seed_words) -> the uint64 seed"""
    lo, hi = (int(v) & MASK for v in words32)
    return lo | (hi << 32)


# ---- the stand-in for seervideoldm_amd.ops --------------------------------------------------------------------------------------
def philox_normal(seed, stream, index, n, device=None, out=None):
    vals = torch.from_numpy(normals64(seed, stream, index, n)).to(torch.float32)
    if out is None:
        return vals.to(device) if device is not None else vals
    out.view(-1)[:n] = vals.to(out.device)
    return out


def _update(e, x, coef_row, noise):
    a_t, a_prev, sigma, s1m = coef_row
    x0 = (x - s1m * e) / torch.sqrt(a_t)
    dirx = torch.sqrt(1.0 - a_prev - sigma * sigma) * e
    return torch.sqrt(a_prev) * x0 + dirx + (sigma * noise if noise is not None else 0.0), x0


def _noise(seed_words32, index, temperature, like):
    n = philox_normal(seed_of(seed_words32), STREAM_STEP, index, like.numel()).reshape(like.shape).to(like.device)
    return torch.tensor(temperature, dtype=torch.float32) * n


def cfg_ddim_step_rng(eps, x, coef, index, seeds, *, cfg, scale, cond_f, temperature=1., x_prev=None, want_pred_x0=True):
    b = x.shape[0]
    e = eps[:, :, cond_f:]
    e = e[:b] + scale * (e[b:] - e[:b]) if cfg else e
    new, pred = torch.empty_like(x), torch.empty_like(x)
    for bi in range(b):
        noise = _noise(seeds[bi], index, temperature, x[bi]) if float(coef[index, 2]) != 0 else None
        new[bi], pred[bi] = _update(e[bi], x[bi], coef[index], noise)
    if x_prev is not None:
        x_prev.copy_(new)
        new = x_prev
    return new, (pred if want_pred_x0 else None)


def slot_cfg_ddim_step_rng(eps, x, scale, coef, step, seeds, temperature, *, cond_f, x_prev, pred_x0):
    slots = x.shape[0]
    assert eps.shape[0] == 2 * slots and eps.shape[2] == x.shape[2] + cond_f and tuple(coef.shape[::2]) == (slots, 4)
    assert tuple(seeds.shape) == (slots, 2) and seeds.dtype == torch.int32 and tuple(temperature.shape) == (slots,)
    for s in range(slots):
        index = int(step[s, 1])
        if index < 0 or index >= coef.shape[1]:
            continue                                # idle: nothing of the slot is written
        eu, ec = eps[s, :, cond_f:], eps[slots + s, :, cond_f:]
        e = eu + scale[s] * (ec - eu)
        noise = _noise(seeds[s], index, float(temperature[s]), x[s]) if float(coef[s, index, 2]) != 0 else None
        new, x0 = _update(e, x[s], coef[s, index], noise)
        x_prev[s] = new
        if pred_x0 is not None:
            pred_x0[s] = x0
        step[s, 0] = index - 1
