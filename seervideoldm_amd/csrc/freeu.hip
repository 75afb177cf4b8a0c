// FreeU (Si et al., CVPR 2024; diffusers' apply_freeu / fourier_filter, threshold 1) on the engine's token-major activations,
// ONE launch per decoder resnet of the two coarsest stages (seer_freeu, include/seer_hip.h):
//   backbone  x_out[r][c] = rnd(x[r][c] * b) for c < Cx / 2, the bits of x[r][c] for the other channels;
//   skip      skip_out = rnd(skip + (s - 1) / (H W) * P), P = the image's lowest frequencies -- the residue set K_H x K_W,
//             K_N = distinct values of {0, -1 mod N} -- put back per (image, channel) plane.  With a_h = e^{+2 pi i h / H} and
//             b_w = e^{+2 pi i w / W} (the twiddle table; conj = the forward transform's sign at residue -1):
//                 X00 = sum skip,  X10 = sum skip a_h,  X01 = sum skip b_w,  X11 = sum skip a_h b_w
//                 P[h][w] = X00 + Re(X10 conj a_h) + Re(X01 conj b_w) + Re(X11 conj(a_h b_w))
//             and the X10 / X11 terms dropped where H = 1, the X01 / X11 terms where W = 1 (K_1 = {0}).
// No sin / cos is evaluated here: the table is the host's (float64, snapped at the quarter turns, stored as fp32 hi and lo parts).
//
// A workgroup owns one image and a slice of FREEU_SLICE channels; a thread owns 8 consecutive channels (16-byte accesses).  Wave v
// of the FREEU_WAVES waves walks the rows h = v, v + FREEU_WAVES, ... in that order.  ORDER OF SUMMATION of a coefficient, per
// channel: inside a row the pixels w = 0 .. W - 1 in order (row sums R0 = sum skip, R1 = sum skip b_w, each kept as the running
// fp32 sum and the sum of its rounding errors; all of the skip half is two-float arithmetic, see below); the
// wave's rows in ascending h (X00 += R0, X01 += R1, X10 += R0 a_h, X11 += R1 a_h); then the waves' partials 0 .. FREEU_WAVES - 1
// in order, read back from LDS by every thread.  No atomics: an element's bits depend on its own (image, channel) plane, on H, W,
// the table and s -- not on the other images, the other channels or the launch's size.  The second pass re-reads the plane (from
// L2: a workgroup's share is FREEU_SLICE * H * W * 2 bytes) and writes each element once.
#include "seer_common.h"

#define FREEU_WAVES 4
#define FREEU_SLICE (SEER_WAVE * 8)
#define FREEU_COEFS 7       // X00, X10 (re, im), X01 (re, im), X11 (re, im)

template <bool F16>
__device__ __forceinline__ void freeu_backbone(const char* x, char* x_out, int Cx, int slice, int64_t img, int HW, float b) {
    const int lane = threadIdx.x & (SEER_WAVE - 1), wave = threadIdx.x / SEER_WAVE;
    const int c0 = slice * FREEU_SLICE + lane * 8;
    if (c0 >= Cx) return;                       // the tail of the last slice
    const int half = Cx / 2;
    // per 16-bit element of the four dwords: scaled (all ones) or passed through as it is (bits, NaN payloads included)
    unsigned int mask[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        mask[i] = (c0 + 2 * i < half ? 0x0000ffffu : 0u) | (c0 + 2 * i + 1 < half ? 0xffff0000u : 0u);
    const int64_t base = (img * HW * Cx + c0) * 2;
    for (int p = wave; p < HW; p += FREEU_WAVES) {
        const int64_t off = base + (int64_t)p * Cx * 2;
        u32x4 v = *reinterpret_cast<const u32x4*>(x + off);
        if (c0 < half) {
            float f[8];
            unpack8t<F16>(v, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] *= b;
            const u32x4 sc = pack8t<F16>(f);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = (sc[i] & mask[i]) | (v[i] & ~mask[i]);
        }
        store16_out(x_out + off, v);
    }
}

// ---- two-float arithmetic: a value is hi + lo, two fp32 numbers (about 48 significand bits).  Why it is here: where skip and
// correction cancel, an error of 2^-25 of the CORRECTION is a visible part of the small result's fp16 spacing, and a correction kept
// in one fp32 number then moves more than 2e-4 of a small plane's elements off the rounded exact value (tests/test_gpu_freeu.py).
// The building blocks are the error-free transformations (Knuth's TwoSum, Dekker's FastTwoSum, the fma TwoProduct); they are exact
// only if the compiler neither fuses nor reorders them: contraction is off from here on, every fma below is written out.
#pragma clang fp contract(off)
struct df {
    float h, l;
};
__device__ __forceinline__ df two_sum(float a, float b) {
    const float s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ df fast_two_sum(float a, float b) {      // |a| >= |b|, or a == 0
    const float s = a + b;
    return {s, b - (s - a)};
}
__device__ __forceinline__ df two_prod(float a, float b) {
    const float p = a * b;
    return {p, fmaf(a, b, -p)};
}
__device__ __forceinline__ df df_add(df a, df b) {
    const df s = two_sum(a.h, b.h);
    return fast_two_sum(s.h, s.l + (a.l + b.l));
}
__device__ __forceinline__ df df_mul(df a, df b) {
    const df p = two_prod(a.h, b.h);
    return fast_two_sum(p.h, fmaf(a.h, b.l, fmaf(a.l, b.h, p.l)));
}
__device__ __forceinline__ df df_neg(df a) { return {-a.h, -a.l}; }

#define FREEU_PHASE 3       // coefficients whose partials share the LDS buffer at a time

template <bool F16>
__device__ __forceinline__ void freeu_skip(const char* skip, char* skip_out, int Cs, int slice, int64_t img, int H, int W, float s,
                                           const float* __restrict__ tw, float (*part)[FREEU_PHASE][2][8][SEER_WAVE]) {
    const int lane = threadIdx.x & (SEER_WAVE - 1), wave = threadIdx.x / SEER_WAVE;
    const int c0 = slice * FREEU_SLICE + lane * 8;
    const bool on = c0 < Cs;                    // (off: the tail of the last slice -- no access, but the barriers are everybody's)
    // the table: hi parts, then lo parts, each cos_H[H] sin_H[H] cos_W[W] sin_W[W]
    const int n_tw = 2 * H + 2 * W;
    const float *cH = tw, *sH = tw + H, *cW = tw + 2 * H, *sW = tw + 2 * H + W;
    const int64_t base = (img * H * W * Cs + c0) * 2;
    const int64_t pitch = (int64_t)Cs * 2;
    df acc[FREEU_COEFS][8];
#pragma unroll
    for (int k = 0; k < FREEU_COEFS; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] = {0.f, 0.f};
    if (on) {
        for (int h = wave; h < H; h += FREEU_WAVES) {
            // row sums R0 = sum skip, R1 = sum skip b_w as (running sum, sum of its rounding errors)
            float s0[8], e0[8], s1[8], e1[8], s2[8], e2[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) s0[e] = e0[e] = s1[e] = e1[e] = s2[e] = e2[e] = 0.f;
            const char* row = skip + base + (int64_t)h * W * pitch;
            for (int w = 0; w < W; ++w) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(row + w * pitch);
                float f[8];
                unpack8t<F16>(v, f);
                const float ch = cW[w], cl = cW[w + n_tw], sh = sW[w], sl = sW[w + n_tw];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    df t = two_sum(s0[e], f[e]);
                    s0[e] = t.h;
                    e0[e] += t.l;
                    df p = two_prod(f[e], ch);          // exact: a 16-bit value times an fp32 one
                    t = two_sum(s1[e], p.h);
                    s1[e] = t.h;
                    e1[e] += t.l + fmaf(f[e], cl, p.l);
                    p = two_prod(f[e], sh);
                    t = two_sum(s2[e], p.h);
                    s2[e] = t.h;
                    e2[e] += t.l + fmaf(f[e], sl, p.l);
                }
            }
            const df c = {cH[h], cH[h + n_tw]}, sn = {sH[h], sH[h + n_tw]};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const df r0 = two_sum(s0[e], e0[e]), r1r = two_sum(s1[e], e1[e]), r1i = two_sum(s2[e], e2[e]);
                acc[0][e] = df_add(acc[0][e], r0);
                acc[1][e] = df_add(acc[1][e], df_mul(r0, c));
                acc[2][e] = df_add(acc[2][e], df_mul(r0, sn));
                acc[3][e] = df_add(acc[3][e], r1r);
                acc[4][e] = df_add(acc[4][e], r1i);
                acc[5][e] = df_add(acc[5][e], df_add(df_mul(r1r, c), df_neg(df_mul(r1i, sn))));      // (R1r + i R1i)(c + i sn)
                acc[6][e] = df_add(acc[6][e], df_add(df_mul(r1r, sn), df_mul(r1i, c)));
            }
        }
    }
    // the waves' partials in wave order, FREEU_PHASE coefficients at a time; K_1 = {0}: the coefficients at residue -1 of a length-1
    // axis do not exist
#pragma unroll
    for (int k0 = 0; k0 < FREEU_COEFS; k0 += FREEU_PHASE) {
        if (k0) __syncthreads();
#pragma unroll
        for (int k = k0; k < k0 + FREEU_PHASE && k < FREEU_COEFS; ++k)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                part[wave][k - k0][0][e][lane] = acc[k][e].h;
                part[wave][k - k0][1][e][lane] = acc[k][e].l;
            }
        __syncthreads();
#pragma unroll
        for (int k = k0; k < k0 + FREEU_PHASE && k < FREEU_COEFS; ++k) {
            const bool use = k == 0 || (k < 3 ? H > 1 : k < 5 ? W > 1 : (H > 1 && W > 1));
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                df t = {part[0][k - k0][0][e][lane], part[0][k - k0][1][e][lane]};
#pragma unroll
                for (int v = 1; v < FREEU_WAVES; ++v) t = df_add(t, df{part[v][k - k0][0][e][lane], part[v][k - k0][1][e][lane]});
                acc[k][e] = use ? t : df{0.f, 0.f};
            }
        }
    }
    if (!on) return;
    // g = (s - 1) / (H W) in two floats
    const float n = (float)((int64_t)H * W);
    const df d = two_sum(s, -1.0f);
    const float q1 = d.h / n;
    const df g = fast_two_sum(q1, (fmaf(-q1, n, d.h) + d.l) / n);
    for (int h = wave; h < H; h += FREEU_WAVES) {
        const df c = {cH[h], cH[h + n_tw]}, sn = {sH[h], sH[h + n_tw]};
        // g P[h][w] = A + Br cos_w + Bi sin_w
        df A[8], Br[8], Bi[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            A[e] = df_mul(g, df_add(acc[0][e], df_add(df_mul(acc[1][e], c), df_mul(acc[2][e], sn))));
            Br[e] = df_mul(g, df_add(acc[3][e], df_add(df_mul(acc[5][e], c), df_mul(acc[6][e], sn))));
            Bi[e] = df_mul(g, df_add(acc[4][e], df_add(df_mul(acc[6][e], c), df_neg(df_mul(acc[5][e], sn)))));
        }
        const int64_t roff = base + (int64_t)h * W * pitch;
        for (int w = 0; w < W; ++w) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(skip + roff + w * pitch);
            float f[8];
            unpack8t<F16>(v, f);
            const float ch = cW[w], cl = cW[w + n_tw], sh = sW[w], sl = sW[w + n_tw];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                // skip + A + Br cos_w + Bi sin_w: the four leading terms added without error, every error term into one fp32 tail
                const df p1 = two_prod(Br[e].h, ch), p2 = two_prod(Bi[e].h, sh);
                const float low = (A[e].l + (p1.l + p2.l)) + (fmaf(Br[e].h, cl, Br[e].l * ch) + fmaf(Bi[e].h, sl, Bi[e].l * sh));
                const df t1 = two_sum(p1.h, p2.h), t2 = two_sum(t1.h, A[e].h), t3 = two_sum(t2.h, f[e]);
                f[e] = t3.h + (t3.l + (t2.l + (t1.l + low)));
            }
            store16_out(skip_out + roff + w * pitch, pack8t<F16>(f));
        }
    }
}

// grid (images, skip slices + backbone slices): blockIdx.y < slices_s is a slice of the skip, the others of the backbone
template <bool F16>
__global__ __launch_bounds__(FREEU_WAVES* SEER_WAVE) void freeu_kernel(const char* x, char* x_out, int Cx, const char* skip,
                                                                        char* skip_out, int Cs, int slices_s, int H, int W,
                                                                        const float* __restrict__ params,
                                                                        const float* __restrict__ tw) {
    __shared__ float part[FREEU_WAVES][FREEU_PHASE][2][8][SEER_WAVE];
    const int64_t img = blockIdx.x;
    const int y = blockIdx.y;
    if (y < slices_s)
        freeu_skip<F16>(skip, skip_out, Cs, y, img, H, W, params[1], tw, part);
    else
        freeu_backbone<F16>(x, x_out, Cx, y - slices_s, img, H * W, params[0]);
}

static bool freeu_overlap(const void* a, const void* b, int64_t bytes_a, int64_t bytes_b) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)bytes_b && pb < pa + (uintptr_t)bytes_a;
}

extern "C" int seer_freeu(const void* x, void* x_out, int32_t Cx, const void* skip, void* skip_out, int32_t Cs, int64_t rows,
                          int32_t images, int32_t H, int32_t W, const float* params, const float* twiddles, int32_t dtype,
                          void* stream) {
    return seer_dispatch_dtype(dtype, [&](auto f16) {
        constexpr bool F16 = decltype(f16)::value;
        const bool has_x = x || x_out, has_s = skip || skip_out;
        if (!has_x && !has_s) return SEER_EINVAL;
        if ((has_x && (!x || !x_out)) || (has_s && (!skip || !skip_out))) return SEER_EINVAL;
        if (!params || !twiddles || ((uintptr_t)params | (uintptr_t)twiddles) % 4) return SEER_EINVAL;
        if (images < 1 || H < 1 || W < 1 || (int64_t)H * W > INT32_MAX || rows != (int64_t)images * H * W) return SEER_EINVAL;
        if ((has_x && (Cx < 8 || Cx % 8)) || (has_s && (Cs < 8 || Cs % 8))) return SEER_EINVAL;
        if (((uintptr_t)x | (uintptr_t)x_out | (uintptr_t)skip | (uintptr_t)skip_out) % 16) return SEER_EINVAL;
        const int64_t bx = has_x ? rows * Cx * 2 : 0, bs = has_s ? rows * Cs * 2 : 0;
        if (has_x && x_out != x && freeu_overlap(x_out, x, bx, bx)) return SEER_EINVAL;        // in place, or apart
        if (has_s && freeu_overlap(skip_out, skip, bs, bs)) return SEER_EINVAL;                // the skip is read twice: never in place
        if (has_x && has_s &&
            (freeu_overlap(x_out, skip, bx, bs) || freeu_overlap(skip_out, x, bs, bx) || freeu_overlap(x_out, skip_out, bx, bs)))
            return SEER_EINVAL;
        const int64_t slices_s = has_s ? (Cs + FREEU_SLICE - 1) / FREEU_SLICE : 0;
        const int64_t slices_x = has_x ? (Cx + FREEU_SLICE - 1) / FREEU_SLICE : 0;
        if (slices_s + slices_x > 65535) return SEER_EINVAL;
        dim3 grid((unsigned)images, (unsigned)(slices_s + slices_x));
        hipLaunchKernelGGL(freeu_kernel<F16>, grid, dim3(FREEU_WAVES * SEER_WAVE), 0, reinterpret_cast<hipStream_t>(stream),
                           reinterpret_cast<const char*>(x), reinterpret_cast<char*>(x_out), has_x ? Cx : 0,
                           reinterpret_cast<const char*>(skip), reinterpret_cast<char*>(skip_out), has_s ? Cs : 0, (int)slices_s, H, W,
                           params, twiddles);
        SEER_LAUNCH_CHECK();
        return SEER_OK;
    });
}
