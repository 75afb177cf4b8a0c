// The counter-based generator on its own (seer_philox.h has the definitions): the raw words as a diagnostic, and the first n
// normals of a clip's stream -- the start code of a seeded clip, and the noise tensor the two-stage comparison of the tests feeds to
// seer_cfg_ddim_step.  One thread per Philox block of four; the step kernels in sampler_step.hip draw per element through
// seer_philox::normal_at and get the same values.
#include "seer_common.h"
#include "seer_philox.h"
#include <cstdint>

namespace {

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

__global__ void philox_u32_kernel(uint32_t k0, uint32_t k1, uint32_t c2, uint32_t c3, uint32_t index, uint32_t first_block,
                                  int64_t n_blocks, uint32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_blocks) return;
    uint32_t w[4];
    seer_philox::philox4x32_10(first_block + (uint32_t)i, index, c2, c3, k0, k1, w);
    for (int j = 0; j < 4; ++j) out[4 * i + j] = w[j];
}

__global__ void philox_normal_kernel(uint32_t k0, uint32_t k1, uint32_t stream, uint32_t index, int64_t n, float* __restrict__ out) {
    const int64_t blk = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (4 * blk >= n) return;
    uint32_t w[4];
    seer_philox::philox4x32_10((uint32_t)blk, index, stream, 0u, k0, k1, w);
    float v[4];
    seer_philox::box_muller(w[0], w[1], v[0], v[1]);
    seer_philox::box_muller(w[2], w[3], v[2], v[3]);
    for (int j = 0; j < 4; ++j)
        if (4 * blk + j < n) out[4 * blk + j] = v[j];    // nothing past out[n - 1]
}

}  // namespace

extern "C" int seer_philox_u32(uint64_t seed, uint64_t stream, uint32_t index, uint64_t first_block, int64_t n_blocks, uint32_t* out,
                               void* stream_) {
    if (!out || (reinterpret_cast<uintptr_t>(out) & 3) || n_blocks <= 0 || first_block > 0xffffffffull ||
        (uint64_t)n_blocks > 0x100000000ull - first_block)
        return SEER_EINVAL;
    hipLaunchKernelGGL(philox_u32_kernel, dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, S(stream_), (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint32_t)stream, (uint32_t)(stream >> 32), index, (uint32_t)first_block, n_blocks, out);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_philox_normal(uint64_t seed, uint32_t stream, uint32_t index, int64_t n, float* out, void* stream_) {
    if (!out || (reinterpret_cast<uintptr_t>(out) & 3) || n <= 0 || n >= ((int64_t)1 << 31)) return SEER_EINVAL;
    const int64_t blocks = (n + 3) / 4;
    hipLaunchKernelGGL(philox_normal_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, S(stream_), (uint32_t)seed,
                       (uint32_t)(seed >> 32), stream, index, n, out);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}
