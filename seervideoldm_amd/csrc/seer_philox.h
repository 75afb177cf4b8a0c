// Counter-based noise for the sampler step ("Seeded noise"): Philox4x32-10 (Salmon et al., "Parallel random numbers: as
// easy as 1, 2, 3", SC'11; the Random123 known-answer vectors are in tests/stoch_ref.py) and the map from its words to normals.
// Shared by rng.hip (seer_philox_u32, seer_philox_normal) and elementwise.hip (the *_rng forms of the DDIM step), so that the start
// code, the diagnostic and the step noise are one piece of device code.
//
//   key      (seed & 0xffffffff, seed >> 32): one 64-bit seed per clip
//   counter  (block, index, stream, 0); block = e >> 2 for element e of the clip's own [C, F_pred, HW] latent; element e takes normal
//            e & 3 of its block.  stream 0 = the start code (index 0), stream 1 = the step noise (index = schedule index), stream 2 = the
//            noise that re-noises GIVEN latents to the level of schedule index `index` (seer_q_sample, seer_known_blend), >= 3 reserved
//   uniform  u = float(2 * (w >> 9) + 1) * 2^-24: exact in fp32, strictly inside (0, 1)
//   normals  Box-Muller on (w0, w1) and (w2, w3): r = sqrtf(-2 logf(u_a)), (s, c) = sincospif(2 u_b) -- the argument is exact, no
//            2 pi rounding -- n_even = r c, n_odd = r s.  |n| <= 5.7682 (u_a = 2^-24).
// A normal is a rounded fp32 product that only ever feeds another multiply, so no later add can be contracted into it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace seer_philox {

constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;      // round multipliers
constexpr uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;      // key increments
enum : uint32_t { STREAM_START = 0, STREAM_STEP = 1, STREAM_KNOWN = 2 };

// ten rounds of (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key bumped between rounds
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&w)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

__device__ __forceinline__ float uniform(uint32_t w) { return (float)(2u * (w >> 9) + 1u) * 0x1p-24f; }

__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float& n_even, float& n_odd) {
    const float r = sqrtf(-2.f * logf(uniform(wa)));
    float s, c;
    sincospif(2.f * uniform(wb), &s, &c);
    n_even = r * c;
    n_odd = r * s;
}

// normal number e of the (seed, stream, index) sequence: the one path every kernel takes to a single element
__device__ __forceinline__ float normal_at(uint32_t seed_lo, uint32_t seed_hi, uint32_t stream, uint32_t index, uint32_t e) {
    uint32_t w[4];
    philox4x32_10(e >> 2, index, stream, 0u, seed_lo, seed_hi, w);
    float n_even, n_odd;
    const bool second = (e & 2u) != 0u;
    box_muller(second ? w[2] : w[0], second ? w[3] : w[1], n_even, n_odd);
    return (e & 1u) ? n_odd : n_even;
}

}  // namespace seer_philox
