// Step caching (SeerUNet.enable_step_cache; DeepCache, Ma et al., CVPR 2024, and TaylorSeer, Liu et al., 2025): the feature that enters
// the shallowest decoder layers is kept over the last three full evaluations in a ring of three slots, slot 0 the newest, and a cached
// evaluation starts from a weighted combination of the slots (seer_cache_push, seer_cache_forecast; include/seer_hip.h).
//
// Both kernels are flat and memory bound: a thread owns ONE 16-byte vector (8 elements) of every slot, the thread behind the last whole
// vector owns the n % 8 elements of the tail, one 16-bit access each.  No LDS, no atomics, no cross-thread traffic: an element's bits
// depend on that element of the sources and, for the forecast, on the three weights.
#include "seer_common.h"

#define SC_THREADS 256

// slot2 <- slot1, slot1 <- slot0, slot0 <- x.  Every thread reads its elements of the three sources before its first store, and no
// other thread touches them.  Values move as bits: one kernel serves both storage types.
__global__ __launch_bounds__(SC_THREADS) void cache_push_kernel(const char* __restrict__ x, char* ring, int64_t n, int64_t slot_bytes) {
    const int64_t i = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x, vecs = n >> 3;
    char *s0 = ring, *s1 = ring + slot_bytes, *s2 = ring + 2 * slot_bytes;
    if (i < vecs) {
        const int64_t off = i * 16;
        const u32x4 vx = *reinterpret_cast<const u32x4*>(x + off);
        const u32x4 v0 = *reinterpret_cast<const u32x4*>(s0 + off);
        const u32x4 v1 = *reinterpret_cast<const u32x4*>(s1 + off);
        store16_out(s2 + off, v1);
        store16_out(s1 + off, v0);
        store16_out(s0 + off, vx);
    } else if (i == vecs) {
        for (int64_t e = vecs * 8; e < n; ++e) {
            const unsigned short ex = reinterpret_cast<const unsigned short*>(x)[e];
            const unsigned short e0 = reinterpret_cast<const unsigned short*>(s0)[e];
            const unsigned short e1 = reinterpret_cast<const unsigned short*>(s1)[e];
            reinterpret_cast<unsigned short*>(s2)[e] = e1;
            reinterpret_cast<unsigned short*>(s1)[e] = e0;
            reinterpret_cast<unsigned short*>(s0)[e] = ex;
        }
    }
}

// out = rnd(fma(w2, f2, fma(w1, f1, w0 * f0))) in fp32, one rounding to the storage type.  The weights are wave-uniform: a slot whose
// weight is exactly 0 is not loaded at all (it may hold NaN, or never have been written) and leaves the accumulator as it is -- +0 in
// place of the first product.
template <bool F16>
__global__ __launch_bounds__(SC_THREADS) void cache_forecast_kernel(const char* __restrict__ ring, int64_t n, int64_t slot_bytes,
                                                                    const float* __restrict__ w, char* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x, vecs = n >> 3;
    const float w0 = w[0], w1 = w[1], w2 = w[2];
    const bool on0 = w0 != 0.0f, on1 = w1 != 0.0f, on2 = w2 != 0.0f;
    const char *s0 = ring, *s1 = ring + slot_bytes, *s2 = ring + 2 * slot_bytes;
    if (i < vecs) {
        const int64_t off = i * 16;
        u32x4 v0 = {0u, 0u, 0u, 0u}, v1 = v0, v2 = v0;
        if (on0) v0 = *reinterpret_cast<const u32x4*>(s0 + off);
        if (on1) v1 = *reinterpret_cast<const u32x4*>(s1 + off);
        if (on2) v2 = *reinterpret_cast<const u32x4*>(s2 + off);
        float acc[8], f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
        if (on0) {
            unpack8t<F16>(v0, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = w0 * f[e];
        }
        if (on1) {
            unpack8t<F16>(v1, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(w1, f[e], acc[e]);
        }
        if (on2) {
            unpack8t<F16>(v2, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(w2, f[e], acc[e]);
        }
        store16_out(out + off, pack8t<F16>(acc));
    } else if (i == vecs) {
        for (int64_t e = vecs * 8; e < n; ++e) {
            float acc = 0.0f;
            if (on0) acc = w0 * unpack2t<F16>(reinterpret_cast<const unsigned short*>(s0)[e])[0];
            if (on1) acc = fmaf(w1, unpack2t<F16>(reinterpret_cast<const unsigned short*>(s1)[e])[0], acc);
            if (on2) acc = fmaf(w2, unpack2t<F16>(reinterpret_cast<const unsigned short*>(s2)[e])[0], acc);
            reinterpret_cast<unsigned short*>(out)[e] = (unsigned short)(pack2t<F16>(acc, 0.0f) & 0xffffu);
        }
    }
}

// the checks both entry points share: `other` is x (push) or out (forecast), n elements; the ring spans 2 * slot_stride + n elements
static bool cache_args_ok(const void* other, const void* ring, int64_t n, int64_t slot_stride) {
    if (!other || !ring || n < 1 || slot_stride < n || slot_stride % 8) return false;
    if (n > (INT64_MAX / 8) || slot_stride > (INT64_MAX / 8)) return false;
    if (((uintptr_t)other | (uintptr_t)ring) % 16) return false;
    const uintptr_t po = (uintptr_t)other, pr = (uintptr_t)ring;
    const uintptr_t bo = (uintptr_t)n * 2, br = (uintptr_t)(2 * slot_stride + n) * 2;
    return !(po < pr + br && pr < po + bo);
}

static unsigned cache_blocks(int64_t n) { return (unsigned)(((n >> 3) + ((n & 7) ? 1 : 0) + SC_THREADS - 1) / SC_THREADS); }

extern "C" int seer_cache_push(const void* x, void* ring, int64_t n, int64_t slot_stride, int32_t dtype, void* stream) {
    if (dtype != SEER_DT_BF16 && dtype != SEER_DT_F16) return SEER_EINVAL;
    if (!cache_args_ok(x, ring, n, slot_stride) || (n >> 3) / SC_THREADS >= INT32_MAX) return SEER_EINVAL;
    hipLaunchKernelGGL(cache_push_kernel, dim3(cache_blocks(n)), dim3(SC_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const char*>(x), reinterpret_cast<char*>(ring), n, slot_stride * 2);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_cache_forecast(const void* ring, int64_t n, int64_t slot_stride, const float* w, void* out, int32_t dtype,
                                   void* stream) {
    return seer_dispatch_dtype(dtype, [&](auto f16) {
        constexpr bool F16 = decltype(f16)::value;
        if (!w || (uintptr_t)w % 4) return SEER_EINVAL;
        if (!cache_args_ok(out, ring, n, slot_stride) || (n >> 3) / SC_THREADS >= INT32_MAX) return SEER_EINVAL;
        hipLaunchKernelGGL(cache_forecast_kernel<F16>, dim3(cache_blocks(n)), dim3(SC_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                           reinterpret_cast<const char*>(ring), n, slot_stride * 2, w, reinterpret_cast<char*>(out));
        SEER_LAUNCH_CHECK();
        return SEER_OK;
    });
}
