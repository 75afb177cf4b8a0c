// Small / boundary kernels of the Seer hot path on gfx950: rotary embedding, timestep embedding, small-M linear,
// conv_in / conv_out (layout change fused), casts, CFG + DDIM / PLMS update.
#include "seer_common.h"
#include "seer_philox.h"
#include <atomic>
#include <cstdint>
#include <initializer_list>

namespace {

// ---- rotary ------------------------------------------------------------------------------------------------
// table[pos][j] = (cos, sin)(pos * freqs[j]) in fp32, angle rounded once like the reference's einsum
// (rotary-embedding-torch 0.1.5: freqs = einsum('..., f -> ... f', t.float(), freqs)).
__global__ void rotary_table_kernel(const float* __restrict__ freqs, int T, int half, float* __restrict__ cs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * half) return;
    const int pos = i / half, j = i - pos * half;
    const float ang = (float)pos * freqs[j];
    float s, c;
    sincosf(ang, &s, &c);
    cs[2 * i] = c;
    cs[2 * i + 1] = s;
}

// one wave per token row: lane -> (which of q/k, head, 8-element chunk of the rotated prefix)
__global__ void __launch_bounds__(256) rotary_kernel(bf16* __restrict__ x, int64_t rows, int ld, int col0_q, int col0_k,
                                                     int heads, int head_dim, int rot_dim, int tokens_per_batch,
                                                     int pos_offset, const float* __restrict__ cs) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int cpr = rot_dim / 8;                 // chunks per head
    const int per_which = heads * cpr;
    const int half = rot_dim / 2;
    const int pos = (int)(row % tokens_per_batch) + pos_offset;
    for (int item = lane; item < 2 * per_which; item += 64) {
        const int which = item / per_which;
        const int rem = item - which * per_which;
        const int head = rem / cpr, ch = rem - head * cpr;
        bf16* ptr = x + row * ld + (which ? col0_k : col0_q) + head * head_dim + ch * 8;
        u32x4 v = *reinterpret_cast<u32x4*>(ptr);
        float f[8];
        unpack8(v, f);
        const float* t = cs + ((int64_t)pos * half + ch * 4) * 2;
#pragma unroll
        for (int pi = 0; pi < 4; ++pi) {
            // t*cos + rotate_half(t)*sin, rotate_half: (x0, x1) -> (-x1, x0); rot_pair (seer_common.h) says why it is not written out
            const f32x2 r = rot_pair(f32x2{f[2 * pi], f[2 * pi + 1]}, t[2 * pi], t[2 * pi + 1]);
            f[2 * pi] = r[0];
            f[2 * pi + 1] = r[1];
        }
        *reinterpret_cast<u32x4*>(ptr) = pack8(f);
    }
}

// ---- timestep embedding ---------------------------------------------------------------------------------------
__global__ void timestep_embedding_kernel(const int64_t* __restrict__ t, int B, int dim, int flip, float shift,
                                          float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int half = dim / 2;
    if (i >= B * half) return;
    const int b = i / half, j = i - b * half;
    // diffusers 0.10.2 get_timestep_embedding: exponent = -ln(10000) * j / (half - shift); emb = t * exp(exponent)
    const float expo = -9.210340371976184f * (float)j / ((float)half - shift);
    const float arg = (float)t[b] * expf(expo);
    float s, c;
    sincosf(arg, &s, &c);
    float* o = out + (int64_t)b * dim;
    if (flip) { o[j] = c; o[half + j] = s; }
    else { o[j] = s; o[half + j] = c; }
}

// ---- small-M linear (time-embedding MLP, B <= 8 rows): act(x) staged once per block in LDS, each wave owns ROWS
// consecutive output features so ROWS independent 16-B weight loads per lane are in flight per K pass (the 51 MB
// time_emb_proj stack is a pure HBM stream) -----------------------------------------------------------------------
template <int MAXB, int ROWS, bool F16 = false>
__global__ void __launch_bounds__(256) linear_smallm_kernel(const float* __restrict__ x, int B, int K,
                                                            const bf16* __restrict__ W, const float* __restrict__ bias,
                                                            int N, int silu_in, int silu_out, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float xs[];     // [B][K]
    for (int i = threadIdx.x; i < B * K; i += 256) {
        float v = x[i];
        if (silu_in) v = silu_f(v);
        xs[i] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * ROWS;
    if (n0 >= N) return;
    float acc[ROWS][MAXB];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
        for (int b = 0; b < MAXB; ++b) acc[r][b] = 0.f;
    for (int k0 = lane * 8; k0 < K; k0 += 64 * 8) {
        u32x4 wv[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int n = n0 + r < N ? n0 + r : N - 1;
            wv[r] = *reinterpret_cast<const u32x4*>(W + (int64_t)n * K + k0);
        }
        float xv[MAXB][8];
#pragma unroll
        for (int b = 0; b < MAXB; ++b) {
            const int bb = b < B ? b : 0;
            const f32x4 lo = *reinterpret_cast<const f32x4*>(xs + bb * K + k0);
            const f32x4 hi = *reinterpret_cast<const f32x4*>(xs + bb * K + k0 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { xv[b][e] = lo[e]; xv[b][4 + e] = hi[e]; }
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            float w[8];
            unpack8t<F16>(wv[r], w);
#pragma unroll
            for (int b = 0; b < MAXB; ++b)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[r][b] += xv[b][e] * w[e];
        }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
#pragma unroll
        for (int b = 0; b < MAXB; ++b) {
            const float v0 = wave_sum(acc[r][b]);
            if (lane == 0 && b < B && n0 + r < N) {
                float v = v0;
                if (bias) v += bias[n0 + r];
                if (silu_out) v = silu_f(v);
                y[(int64_t)b * N + n0 + r] = v;
            }
        }
    }
}

// ---- conv_in: [B, Cin, F, H, W] fp32 -> channels-last bf16 [B*F*H*W, Cout]; weights fp32 [3][3][Cin][Cout] ----
// per block: the 9*Cin*Cout weights and the 3x3xCin input patches of its `ppb` pixels are staged in LDS once (every
// output-channel group needs the same 9*Cin inputs); a thread owns 8 output channels of one pixel lane
template <bool F16>
__global__ void __launch_bounds__(256) conv_in_kernel(const float* __restrict__ x, int B, int Cin, int F, int H, int Wd,
                                                      const float* __restrict__ Wt, const float* __restrict__ bias,
                                                      int Cout, bf16* __restrict__ y, int ppb) {
    extern __shared__ __attribute__((aligned(16))) float wsm[];     // [9*Cin][Cout] then patches [ppb][9*Cin]
    const int nw = 9 * Cin * Cout;
    const int kk = 9 * Cin;
    float* patch = wsm + nw;
    for (int i = threadIdx.x * 4; i < nw; i += 1024) *reinterpret_cast<f32x4*>(wsm + i) = *reinterpret_cast<const f32x4*>(Wt + i);
    const int64_t npix = (int64_t)B * F * H * Wd;
    const int64_t p0 = (int64_t)blockIdx.x * ppb;
    const int np = (int)(p0 + ppb < npix ? ppb : npix - p0);
    const int64_t cstride = (int64_t)F * H * Wd;   // channel stride of the NCFHW input
    for (int i = threadIdx.x; i < np * kk; i += 256) {
        const int pp = i / kk, k = i - pp * kk;
        const int tap = k / Cin, ci = k - tap * Cin;
        const int64_t pix = p0 + pp;
        const int ox = (int)(pix % Wd);
        const int oy = (int)((pix / Wd) % H);
        const int f = (int)((pix / ((int64_t)Wd * H)) % F);
        const int b = (int)(pix / ((int64_t)Wd * H * F));
        const int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
        float v = 0.f;
        if (iy >= 0 && iy < H && ix >= 0 && ix < Wd)
            v = x[(((int64_t)b * Cin + ci) * F + f) * H * Wd + (int64_t)iy * Wd + ix];
        patch[i] = v;
    }
    __syncthreads();
    const int cgroups = Cout / 8;
    const int npl = 256 / cgroups;                // pixel lanes per block
    const int pl = threadIdx.x / cgroups;
    const int cg = threadIdx.x - pl * cgroups;
    if (pl >= npl) return;
    float bv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bv[e] = bias ? bias[cg * 8 + e] : 0.f;
    for (int pp = pl; pp < np; pp += npl) {
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = bv[e];
        const float* xp = patch + pp * kk;
        const float* wp = wsm + cg * 8;
#pragma unroll 4
        for (int k = 0; k < kk; ++k) {
            const float xv = xp[k];
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp + k * Cout);
            const f32x4 w1 = *reinterpret_cast<const f32x4*>(wp + k * Cout + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc[e] += xv * w0[e]; acc[4 + e] += xv * w1[e]; }
        }
        *reinterpret_cast<u32x4*>(y + (p0 + pp) * Cout + cg * 8) = pack8t<F16>(acc);
    }
}

// ---- conv_out: channels-last bf16 [B*F*H*W, C0] -> [B, Cout, F, H, W] fp32; weights fp32 [Cout][3][3][C0] -------
// weights in LDS once per block; one wave per pixel (lanes over the 9 * C0/8 input chunks), `ppb` pixels per block
template <int COUT, bool F16 = false>
__global__ void __launch_bounds__(256) conv_out_kernel(const bf16* __restrict__ x, int B, int C0, int F, int H, int Wd,
                                                       const float* __restrict__ Wt, const float* __restrict__ bias,
                                                       float* __restrict__ y, int ppb) {
    extern __shared__ __attribute__((aligned(16))) float wsm[];     // [COUT][9][C0]
    const int nw = COUT * 9 * C0;
    for (int i = threadIdx.x * 4; i < nw; i += 1024) *reinterpret_cast<f32x4*>(wsm + i) = *reinterpret_cast<const f32x4*>(Wt + i);
    __syncthreads();
    const int64_t npix = (int64_t)B * F * H * Wd;
    const int64_t p0 = (int64_t)blockIdx.x * ppb;
    const int64_t p1 = p0 + ppb < npix ? p0 + ppb : npix;
    const int lane = threadIdx.x & 63;
    const int nch = C0 / 8;
    for (int64_t pix = p0 + (threadIdx.x >> 6); pix < p1; pix += 4) {
        const int ox = (int)(pix % Wd);
        const int oy = (int)((pix / Wd) % H);
        const int64_t img = pix / ((int64_t)Wd * H);       // b*F + f
        // (even, odd) element pairs accumulated as whole packed operations: with scalar accumulators the SLP vectoriser builds
        // packed multiplies that read the high half of their second source (op_sel[1] = 1), the form asm_check.py refuses
        f32x2 acc[COUT];
#pragma unroll
        for (int o = 0; o < COUT; ++o) acc[o] = f32x2{0.f, 0.f};
        for (int item = lane; item < 9 * nch; item += 64) {
            const int tap = item / nch, ch = item - tap * nch;
            const int ky = tap / 3, kx = tap - 3 * ky;
            const int iy = oy + ky - 1, ix = ox + kx - 1;
            if (iy < 0 || iy >= H || ix < 0 || ix >= Wd) continue;
            const u32x4 v = *reinterpret_cast<const u32x4*>(x + ((img * H + iy) * Wd + ix) * C0 + ch * 8);
            float f[8];
            unpack8t<F16>(v, f);
#pragma unroll
            for (int o = 0; o < COUT; ++o) {
                const float* w = wsm + (o * 9 + tap) * C0 + ch * 8;
                const f32x4 w0 = *reinterpret_cast<const f32x4*>(w);
                const f32x4 w1 = *reinterpret_cast<const f32x4*>(w + 4);
                acc[o] = __builtin_elementwise_fma(f32x2{f[0], f[1]}, f32x2{w0[0], w0[1]}, acc[o]);
                acc[o] = __builtin_elementwise_fma(f32x2{f[2], f[3]}, f32x2{w0[2], w0[3]}, acc[o]);
                acc[o] = __builtin_elementwise_fma(f32x2{f[4], f[5]}, f32x2{w1[0], w1[1]}, acc[o]);
                acc[o] = __builtin_elementwise_fma(f32x2{f[6], f[7]}, f32x2{w1[2], w1[3]}, acc[o]);
            }
        }
        const int f_ = (int)(img % F);
        const int b = (int)(img / F);
#pragma unroll
        for (int o = 0; o < COUT; ++o) {
            const float v = wave_sum(acc[o][0] + acc[o][1]);
            if (lane == 0) y[((((int64_t)b * COUT + o) * F + f_) * H + oy) * Wd + ox] = v + (bias ? bias[o] : 0.f);
        }
    }
}

template <bool F16>
__global__ void cast_f32_bf16_kernel(const float* __restrict__ x, int64_t n, bf16* __restrict__ y) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < n) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + i);
        u32x2 o;
        if constexpr (F16) {
            o[0] = pack2h(v[0], v[1]);
            o[1] = pack2h(v[2], v[3]);
        } else {
            o[0] = pack2(v[0], v[1]);
            o[1] = pack2(v[2], v[3]);
        }
        *reinterpret_cast<u32x2*>(y + i) = o;
    } else {
        for (int64_t j = i; j < n; ++j) {
            if constexpr (F16) reinterpret_cast<_Float16*>(y)[j] = (_Float16)x[j];
            else y[j] = (bf16)x[j];
        }
    }
}

// [N, C, HW] fp32 <-> [N, HW, C] bf16 through a 32x32 LDS tile
__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const float* __restrict__ x, int C, int HW, bf16* __restrict__ y) {
    __shared__ float tile[32][33];
    const int n = blockIdx.z;
    const int c0 = blockIdx.y * 32, p0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, p = p0 + tx;
        tile[i][tx] = (c < C && p < HW) ? x[((int64_t)n * C + c) * HW + p] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int p = p0 + i, c = c0 + tx;
        if (c < C && p < HW) y[((int64_t)n * HW + p) * C + c] = (bf16)tile[tx][i];
    }
}
__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const bf16* __restrict__ x, int C, int HW, float* __restrict__ y) {
    __shared__ float tile[32][33];
    const int n = blockIdx.z;
    const int c0 = blockIdx.y * 32, p0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int p = p0 + i, c = c0 + tx;
        tile[i][tx] = (c < C && p < HW) ? (float)x[((int64_t)n * HW + p) * C + c] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, p = p0 + tx;
        if (c < C && p < HW) y[((int64_t)n * C + c) * HW + p] = tile[tx][i];
    }
}

// ---- CFG + DDIM update (fp32, one thread per latent element) ------------------------------------------------------
// the update of element i from its CFG-combined eps e and row `index` of coef; one body for every form of the step, so an element
// gets the same bits from each.  x may alias x_prev: the element is read before it is written.
__device__ __forceinline__ void ddim_update(float e, const float* __restrict__ coef, int index, const float* x,
                                            const float* __restrict__ noise, float* x_prev, float* __restrict__ pred_x0, int64_t i) {
    const float a_t = coef[4 * index], a_prev = coef[4 * index + 1], sigma = coef[4 * index + 2], s1m = coef[4 * index + 3];
    const float xv = x[i];
    const float x0 = (xv - s1m * e) / sqrtf(a_t);
    const float dir = sqrtf(1.f - a_prev - sigma * sigma) * e;
    float nz = 0.f;
    if (noise) nz = sigma * noise[i];
    x_prev[i] = sqrtf(a_prev) * x0 + dir + nz;
    if (pred_x0) pred_x0[i] = x0;
}

__global__ void cfg_ddim_kernel(const float* __restrict__ eps, int cfg, int b, int C, int Ft, int cond_f, int HW,
                                float scale, const float* __restrict__ coef, int index, const float* __restrict__ x,
                                const float* __restrict__ noise, float* __restrict__ x_prev,
                                float* __restrict__ pred_x0) {
    const int Fp = Ft - cond_f;
    const int64_t n = (int64_t)b * C * Fp * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int hw = (int)(i % HW);
    const int f = (int)((i / HW) % Fp);
    const int c = (int)((i / ((int64_t)HW * Fp)) % C);
    const int bi = (int)(i / ((int64_t)HW * Fp * C));
    const int64_t eoff = (((int64_t)bi * C + c) * Ft + (f + cond_f)) * HW + hw;
    float e;
    if (cfg) {
        const float eu = eps[eoff];
        const float ec = eps[eoff + (int64_t)b * C * Ft * HW];
        e = eu + scale * (ec - eu);
    } else {
        e = eps[eoff];
    }
    ddim_update(e, coef, index, x, noise, x_prev, pred_x0, i);
}

// ---- the same step with its schedule index in DEVICE memory (a whole p_sample_ddim captured in one hipGraph: the kernel
// arguments of a replay are frozen, the step counter is not).  step[0] = index of the NEXT step to run, step[1] = index of the
// step in flight.  seer_ddim_step_begin (first kernel of a step) reads step[0] everywhere and one thread copies it to step[1];
// seer_cfg_ddim_step_dev (last kernel) reads step[1] everywhere and one thread writes step[0] = index - 1: no kernel both reads
// and writes a word, so a chain of replays walks the schedule downwards without the host touching device memory.
// Input assembly of ddim_video.py:189,201-203: the UNet input [reps*b, C, F, HW] = cat([x0_emb, x], frames), repeated for the CFG
// pair, and t[reps*b] = timesteps[index].
__global__ void ddim_assemble_kernel(const float* __restrict__ x0_emb, const float* __restrict__ x, int b, int reps, int C, int f1,
                                     int Fp, int HW, const int64_t* __restrict__ t_table, int* __restrict__ step,
                                     float* __restrict__ sample, int64_t* __restrict__ t_out) {
    const int F = f1 + Fp;
    const int64_t per = (int64_t)b * C * F * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int index = step[0];
    if (i == 0) step[1] = index;
    if (i < reps * b) t_out[i] = t_table[index];
    if (i >= per) return;
    const int hw = (int)(i % HW);
    const int f = (int)((i / HW) % F);
    const int64_t bc = i / ((int64_t)HW * F);            // bi * C + c
    const float v = f < f1 ? x0_emb[(bc * f1 + f) * HW + hw] : x[(bc * Fp + (f - f1)) * HW + hw];
    for (int r = 0; r < reps; ++r) sample[i + r * per] = v;
}

// x may alias x_prev (the captured step updates its latent in place): every thread reads its element before it writes it
__global__ void cfg_ddim_dev_kernel(const float* __restrict__ eps, int cfg, int b, int C, int Ft, int cond_f, int HW, float scale,
                                    const float* __restrict__ coef, int* __restrict__ step, const float* x,
                                    const float* __restrict__ noise, float* x_prev, float* __restrict__ pred_x0) {
    const int Fp = Ft - cond_f;
    const int64_t n = (int64_t)b * C * Fp * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int index = step[1];
    if (i == 0) step[0] = index - 1;
    if (i >= n) return;
    const int hw = (int)(i % HW);
    const int f = (int)((i / HW) % Fp);
    const int c = (int)((i / ((int64_t)HW * Fp)) % C);
    const int bi = (int)(i / ((int64_t)HW * Fp * C));
    const int64_t eoff = (((int64_t)bi * C + c) * Ft + (f + cond_f)) * HW + hw;
    float e;
    if (cfg) {
        const float eu = eps[eoff];
        const float ec = eps[eoff + (int64_t)b * C * Ft * HW];
        e = eu + scale * (ec - eu);
    } else {
        e = eps[eoff];
    }
    ddim_update(e, coef, index, x, noise, x_prev, pred_x0, i);
}

// ---- CFG + PLMS update (ldm/models/diffusion/plms.py:199-236, eta = 0; fp32, one thread per latent element) -----------------
// e = the CFG-combined eps of this evaluation; h1, h2, h3 = earlier e, newest first.  e' by order:
//   0: e (the first step's provisional DDIM update)   1: (h1 + e)/2 (the first step's final update: h1 = first evaluation, e = second)
//   2: (3e - h1)/2   3: (23e - 16h1 + 5h2)/12   4: (55e - 59h1 + 37h2 - 9h3)/24
// then the DDIM update with e' from coefficient row `index`.  A history term the order does not use is never read (stale slots may
// hold NaN, and 0 * NaN is NaN).  e_out (may alias a history slot: every thread reads its element before it writes it) receives e,
// not e' (plms.py:160), for every order but 1, whose e is the second evaluation that plms.py does not keep.
__device__ __forceinline__ float cfg_eps_at(const float* __restrict__ eps, int cfg, int b, int C, int Ft, int cond_f, int HW,
                                            float scale, int64_t i) {
    const int Fp = Ft - cond_f;
    const int hw = (int)(i % HW);
    const int f = (int)((i / HW) % Fp);
    const int c = (int)((i / ((int64_t)HW * Fp)) % C);
    const int bi = (int)(i / ((int64_t)HW * Fp * C));
    const int64_t eoff = (((int64_t)bi * C + c) * Ft + (f + cond_f)) * HW + hw;
    if (!cfg) return eps[eoff];
    const float eu = eps[eoff];
    const float ec = eps[eoff + (int64_t)b * C * Ft * HW];
    return eu + scale * (ec - eu);
}

__device__ __forceinline__ void plms_update(float e, int order, const float* h1, const float* h2, const float* h3, int64_t i,
                                            const float* __restrict__ coef, int index, const float* x, float* x_prev,
                                            float* __restrict__ pred_x0, float* e_out) {
    float ep;
    switch (order) {
        case 0: ep = e; break;
        case 1: ep = (h1[i] + e) / 2.f; break;
        case 2: ep = (3.f * e - h1[i]) / 2.f; break;
        case 3: ep = (23.f * e - 16.f * h1[i] + 5.f * h2[i]) / 12.f; break;
        default: ep = (55.f * e - 59.f * h1[i] + 37.f * h2[i] - 9.f * h3[i]) / 24.f; break;
    }
    const float a_t = coef[4 * index], a_prev = coef[4 * index + 1], sigma = coef[4 * index + 2], s1m = coef[4 * index + 3];
    const float xv = x[i];
    const float x0 = (xv - s1m * ep) / sqrtf(a_t);
    const float dir = sqrtf(1.f - a_prev - sigma * sigma) * ep;
    x_prev[i] = sqrtf(a_prev) * x0 + dir;
    if (pred_x0) pred_x0[i] = x0;
    if (e_out && order != 1) e_out[i] = e;
}

__global__ void cfg_plms_kernel(const float* __restrict__ eps, int cfg, int b, int C, int Ft, int cond_f, int HW, float scale,
                                const float* __restrict__ coef, int index, int order, const float* x, const float* h1,
                                const float* h2, const float* h3, float* x_prev, float* __restrict__ pred_x0, float* e_out) {
    const int64_t n = (int64_t)b * C * (Ft - cond_f) * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    plms_update(cfg_eps_at(eps, cfg, b, C, Ft, cond_f, HW, scale, i), order, h1, h2, h3, i, coef, index, x, x_prev, pred_x0,
                e_out);
}

// The captured form: the index is step[1] (seer_ddim_step_begin copied it there) and the history is a 3-slot ring of [n] fp32
// slots.  ring_state int32[4] holds (valid, newest) twice, by parity of the index: a step reads pair (index & 1) and one thread
// writes pair ((index - 1) & 1) = (min(valid + 1, 3), slot) with slot = (newest + 1) % 3, the slot this step stores e into (the
// oldest one once all three are valid); it also writes step[0] = index - 1.  No kernel reads and writes the same word.
// valid = 0 is a plain DDIM step (order 0), valid = k > 0 is order k + 1.
__global__ void cfg_plms_dev_kernel(const float* __restrict__ eps, int cfg, int b, int C, int Ft, int cond_f, int HW, float scale,
                                    const float* __restrict__ coef, int* __restrict__ step, float* ring,
                                    int* __restrict__ ring_state, const float* x, float* x_prev, float* __restrict__ pred_x0) {
    const int64_t n = (int64_t)b * C * (Ft - cond_f) * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int index = step[1];
    const int* rs = ring_state + 2 * (index & 1);
    int valid = rs[0], newest = rs[1];
    if (valid < 0 || valid > 3 || newest < 0 || newest > 2) valid = 0, newest = 2;     // never index outside the ring
    const int slot = newest == 2 ? 0 : newest + 1;
    if (i == 0) {
        step[0] = index - 1;
        int* ws = ring_state + 2 * ((index - 1) & 1);
        ws[0] = valid < 3 ? valid + 1 : 3;
        ws[1] = slot;
    }
    if (i >= n) return;
    const float* h1 = ring + (int64_t)newest * n;
    const float* h2 = ring + (int64_t)(newest == 0 ? 2 : newest - 1) * n;
    const float* h3 = ring + (int64_t)slot * n;
    plms_update(cfg_eps_at(eps, cfg, b, C, Ft, cond_f, HW, scale, i), valid == 0 ? 0 : valid + 1, h1, h2, h3, i, coef, index,
                x, x_prev, pred_x0, ring + (int64_t)slot * n);
}

// ---- the captured step over SLOTS (continuous batching, seervideoldm_amd/slots.py): per-slot forms of ddim_assemble_kernel and
// cfg_ddim_dev_kernel.  Slot s owns rows s and slots + s of the [uc | c] pair, its own schedule tables t_table[s][nsched] and
// coef[s][nsched][4], its own guidance scale scale[s] and its own counter pair step[s][0..1].  An idle slot (index < 0) still gets
// finite input rows (the host zeroed its latents; its t is row 0 of its table) and its update writes nothing.  As above, no kernel
// reads and writes the same word.  The int64 tables move as int32 pairs: no pointer is relied on beyond 4-byte alignment.
__global__ void slot_assemble_kernel(const float* __restrict__ x0_emb, const float* __restrict__ x, int slots, int reps, int C, int f1,
                                     int Fp, int HW, const int* __restrict__ t_table, int nsched, int* __restrict__ step,
                                     float* __restrict__ sample, int* __restrict__ t_out) {
    const int F = f1 + Fp;
    const int64_t per_slot = (int64_t)C * F * HW;
    const int64_t per = (int64_t)slots * per_slot;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per) return;
    const int s = (int)(i / per_slot);
    if (i == (int64_t)s * per_slot) {                    // the slot's first element: its counter and its timesteps
        const int index = step[2 * s];
        step[2 * s + 1] = index;
        const int row = index < 0 ? 0 : (index < nsched ? index : nsched - 1);      // never outside the table
        const int* t = t_table + 2 * ((int64_t)s * nsched + row);
        for (int r = 0; r < reps; ++r) {
            t_out[2 * (r * slots + s)] = t[0];
            t_out[2 * (r * slots + s) + 1] = t[1];
        }
    }
    const int hw = (int)(i % HW);
    const int f = (int)((i / HW) % F);
    const int64_t bc = i / ((int64_t)HW * F);            // s * C + c
    const float v = f < f1 ? x0_emb[(bc * f1 + f) * HW + hw] : x[(bc * Fp + (f - f1)) * HW + hw];
    for (int r = 0; r < reps; ++r) sample[i + r * per] = v;
}

// CFG always on, eta = 0 (no noise term): cfg_eps_at with scale[s], ddim_update with row step[s][1] of coef[s].  x may alias x_prev.
__global__ void slot_cfg_ddim_kernel(const float* __restrict__ eps, int slots, int C, int Ft, int cond_f, int HW,
                                     const float* __restrict__ scale, const float* __restrict__ coef, int nsched,
                                     int* __restrict__ step, const float* x, float* x_prev, float* __restrict__ pred_x0) {
    const int64_t per_slot = (int64_t)C * (Ft - cond_f) * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)slots * per_slot) return;
    const int s = (int)(i / per_slot);
    const int index = step[2 * s + 1];
    if (index < 0 || index >= nsched) return;            // idle (or a counter outside the table): nothing of this slot is written
    if (i == (int64_t)s * per_slot) step[2 * s] = index - 1;
    ddim_update(cfg_eps_at(eps, 1, slots, C, Ft, cond_f, HW, scale[s], i), coef + (int64_t)s * nsched * 4, index, x, nullptr, x_prev,
                pred_x0, i);
}

// ---- the three forms of the DDIM step above with SEEDED noise (eta > 0): the noise of element el of a clip at schedule index
// `index` is normal number el of Philox stream 1 of the clip's seed (seer_philox.h), drawn here instead of read from a tensor, so a
// captured step has nothing to draw between its launches and a clip's noise does not depend on its batch row or slot.  The update
// is ddim_update's expression with n in the place of noise[i]: sigma * (temperature * n), two rounded fp32 products, then the add.
// sigma == 0 (uniform over a clip's threads) draws nothing and gives ddim_update's bits with noise == nullptr.
__device__ __forceinline__ void ddim_update_rng(float e, const float* __restrict__ coef, int index, const float* x,
                                                const uint32_t* __restrict__ seed, float temperature, uint32_t el, float* x_prev,
                                                float* __restrict__ pred_x0, int64_t i) {
    const float a_t = coef[4 * index], a_prev = coef[4 * index + 1], sigma = coef[4 * index + 2], s1m = coef[4 * index + 3];
    const float xv = x[i];
    const float x0 = (xv - s1m * e) / sqrtf(a_t);
    const float dir = sqrtf(1.f - a_prev - sigma * sigma) * e;
    float nz = 0.f;
    if (sigma != 0.f) {
        const float tn = temperature * seer_philox::normal_at(seed[0], seed[1], seer_philox::STREAM_STEP, (uint32_t)index, el);
        nz = sigma * tn;
    }
    x_prev[i] = sqrtf(a_prev) * x0 + dir + nz;
    if (pred_x0) pred_x0[i] = x0;
}

// seeds uint32 [b][2] (lo, hi): one pair per batch row.  step == nullptr: the host's `index`; else index = step[1] and one thread
// writes step[0] = index - 1, as cfg_ddim_dev_kernel.  x may alias x_prev.
__global__ void cfg_ddim_rng_kernel(const float* __restrict__ eps, int cfg, int b, int C, int Ft, int cond_f, int HW, float scale,
                                    const float* __restrict__ coef, int index, int* __restrict__ step, const float* x,
                                    const uint32_t* __restrict__ seeds, float temperature, float* x_prev,
                                    float* __restrict__ pred_x0) {
    const int64_t per_clip = (int64_t)C * (Ft - cond_f) * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (step) {
        index = step[1];
        if (i == 0) step[0] = index - 1;
    }
    if (index < 0 || i >= (int64_t)b * per_clip) return;     // (a counter that ran past the schedule's end reads no coefficient row)
    const int64_t bi = i / per_clip;
    ddim_update_rng(cfg_eps_at(eps, cfg, b, C, Ft, cond_f, HW, scale, i), coef, index, x, seeds + 2 * bi, temperature,
                    (uint32_t)(i - bi * per_clip), x_prev, pred_x0, i);
}

// slot_cfg_ddim_kernel with a seed pair and a temperature per slot; sigma is column 2 of the slot's own coef rows
__global__ void slot_cfg_ddim_rng_kernel(const float* __restrict__ eps, int slots, int C, int Ft, int cond_f, int HW,
                                         const float* __restrict__ scale, const float* __restrict__ coef, int nsched,
                                         int* __restrict__ step, const float* x, const uint32_t* __restrict__ seeds,
                                         const float* __restrict__ temperature, float* x_prev, float* __restrict__ pred_x0) {
    const int64_t per_slot = (int64_t)C * (Ft - cond_f) * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)slots * per_slot) return;
    const int s = (int)(i / per_slot);
    const int index = step[2 * s + 1];
    if (index < 0 || index >= nsched) return;            // idle (or a counter outside the table): nothing of this slot is written
    if (i == (int64_t)s * per_slot) step[2 * s] = index - 1;
    ddim_update_rng(cfg_eps_at(eps, 1, slots, C, Ft, cond_f, HW, scale[s], i), coef + (int64_t)s * nsched * 4, index, x, seeds + 2 * s,
                    temperature[s], (uint32_t)(i - (int64_t)s * per_slot), x_prev, pred_x0, i);
}

// ---- GIVEN latents (masked sampling, stochastic_encode; CompVis ldm/models/diffusion/ddim.py:144-147, 207-221): q(e) is the given
// latent x0 noised to the level of coefficient row `index`, its noise n either read from a tensor or normal e of Philox stream 2 of
// the clip's seed at that index.  One expression for the three kernels below, so the seeded form gets the bits of the noise-tensor
// form fed seer_philox_normal(seed, 2, index).
__device__ __forceinline__ float q_known(const float* __restrict__ coef, int index, float x0v, float n) {
    return sqrtf(coef[4 * index]) * x0v + coef[4 * index + 3] * n;
}

__device__ __forceinline__ float known_noise(const float* __restrict__ noise, int64_t i, const uint32_t* __restrict__ seed, int index,
                                             uint32_t el) {
    return noise ? noise[i] : seer_philox::normal_at(seed[0], seed[1], seer_philox::STREAM_KNOWN, (uint32_t)index, el);
}

// the blend of one element: m == 0 leaves the word alone (nothing is read but the mask, nothing drawn), m == 1 selects q whatever
// x holds, anything else is CompVis's img_orig * mask + (1. - mask) * img
__device__ __forceinline__ void known_blend_at(float* x, float m, const float* __restrict__ known, const float* __restrict__ coef,
                                               int index, const float* __restrict__ noise, const uint32_t* __restrict__ seed,
                                               uint32_t el, int64_t i) {
    if (m == 0.f) return;
    const float q = q_known(coef, index, known[i], known_noise(noise, i, seed, index, el));
    x[i] = m == 1.f ? q : q * m + (1.f - m) * x[i];
}

// out[bi][e] = q with row index[bi] of coef; a row whose index is outside 0 .. nsched - 1 is not written
__global__ void q_sample_kernel(const float* __restrict__ x0, int b, int64_t per_row, const float* __restrict__ coef, int nsched,
                                const int* __restrict__ index, const float* __restrict__ noise, const uint32_t* __restrict__ seeds,
                                float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)b * per_row) return;
    const int64_t bi = i / per_row;
    const int idx = index[bi];
    if (idx < 0 || idx >= nsched) return;
    out[i] = q_known(coef, idx, x0[i], known_noise(noise, i, seeds + 2 * bi, idx, (uint32_t)(i - bi * per_row)));
}

// x [b, C, Fp, HW] in place; mask [b, Fp, HW] is broadcast over channels.  step != nullptr: index = step[0], the NEXT step's index
// (this kernel runs in front of seer_ddim_step_begin); it is only read.
__global__ void known_blend_kernel(float* x, const float* __restrict__ mask, const float* __restrict__ known, int b, int C, int Fp,
                                   int HW, const float* __restrict__ coef, int index, const int* __restrict__ step,
                                   const float* __restrict__ noise, const uint32_t* __restrict__ seeds) {
    const int64_t per_frames = (int64_t)Fp * HW, per_clip = per_frames * C;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (step) index = step[0];
    if (index < 0 || i >= (int64_t)b * per_clip) return;
    const int64_t bi = i / per_clip;
    const int64_t el = i - bi * per_clip;
    known_blend_at(x, mask[bi * per_frames + el % per_frames], known, coef, index, noise, seeds + 2 * bi, (uint32_t)el, i);
}

// the same over slots, seeded: index = step[s][0] and coef[s]; an idle slot (index < 0 or >= nsched) writes nothing
__global__ void slot_known_blend_kernel(float* x, const float* __restrict__ mask, const float* __restrict__ known, int slots, int C,
                                        int Fp, int HW, const float* __restrict__ coef, int nsched, const int* __restrict__ step,
                                        const uint32_t* __restrict__ seeds) {
    const int64_t per_frames = (int64_t)Fp * HW, per_slot = per_frames * C;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)slots * per_slot) return;
    const int64_t s = i / per_slot;
    const int index = step[2 * s];
    if (index < 0 || index >= nsched) return;
    const int64_t el = i - s * per_slot;
    known_blend_at(x, mask[s * per_frames + el % per_frames], known, coef + s * nsched * 4, index, nullptr, seeds + 2 * s, (uint32_t)el,
                   i);
}

// ---- the same step with a SAMPLER per slot: DDIM and PLMS clips side by side.  state int32 [slots][8] = (phase, valid, newest, -)
// of the NEXT step, then the same three words of the step IN FLIGHT; ring fp32 [slots][3][C*Fp*HW] = the slot's earlier e, x_prov
// [slots][C*Fp*HW] its provisional latent.  The begin kernel reads next words and writes in-flight words, the update kernel reads
// in-flight words and writes next words: as above, no kernel reads and writes the same word.  Phases (plms.py:145-160):
//   0  DDIM, for the whole clip           1  PLMS first step, first evaluation: x_prov = order 0 of x, e -> ring slot 0
//   2  PLMS first step, second evaluation at x_prov and the NEXT timestep: order 1 on x      3  PLMS later steps: order valid + 1
// A phase outside 0..3 is read as 0; in phase 3 a (valid, newest) outside 0..3 x 0..2 is read as (0, 2), as cfg_plms_dev_kernel does.
enum { SLOT_STATE_WORDS = 8, SLOT_IN_FLIGHT = 4 };

__global__ void slot_plms_assemble_kernel(const float* __restrict__ x0_emb, const float* __restrict__ x,
                                          const float* __restrict__ x_prov, int slots, int reps, int C, int f1, int Fp, int HW,
                                          const int* __restrict__ t_table, int nsched, int* __restrict__ step,
                                          int* __restrict__ state, float* __restrict__ sample, int* __restrict__ t_out) {
    const int F = f1 + Fp;
    const int64_t per_slot = (int64_t)C * F * HW;
    const int64_t per = (int64_t)slots * per_slot;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per) return;
    const int s = (int)(i / per_slot);
    const int* next = state + SLOT_STATE_WORDS * s;
    const int phase = next[0];
    if (i == (int64_t)s * per_slot) {                    // the slot's first element: its counter, its state and its timesteps
        int index = step[2 * s];
        step[2 * s + 1] = index;
        int* fly = state + SLOT_STATE_WORDS * s + SLOT_IN_FLIGHT;
        fly[0] = phase, fly[1] = next[1], fly[2] = next[2];
        if (phase == 2) --index;                         // the second evaluation runs at t_next = t_table[max(index - 1, 0)]
        const int row = index < 0 ? 0 : (index < nsched ? index : nsched - 1);      // never outside the table
        const int* t = t_table + 2 * ((int64_t)s * nsched + row);
        for (int r = 0; r < reps; ++r) {
            t_out[2 * (r * slots + s)] = t[0];
            t_out[2 * (r * slots + s) + 1] = t[1];
        }
    }
    const int hw = (int)(i % HW);
    const int f = (int)((i / HW) % F);
    const int64_t bc = i / ((int64_t)HW * F);            // s * C + c
    const float* lat = phase == 2 ? x_prov : x;
    const float v = f < f1 ? x0_emb[(bc * f1 + f) * HW + hw] : lat[(bc * Fp + (f - f1)) * HW + hw];
    for (int r = 0; r < reps; ++r) sample[i + r * per] = v;
}

// CFG always on, eta = 0.  The arithmetic is cfg_eps_at with scale[s], then ddim_update (phase 0) or plms_update (phases 1 to 3)
// with row step[s][1] of coef[s]: an element gets the bits of seer_cfg_ddim_step / seer_cfg_plms_step.  x may alias x_prev.
__global__ void slot_cfg_plms_kernel(const float* __restrict__ eps, int slots, int C, int Ft, int cond_f, int HW,
                                     const float* __restrict__ scale, const float* __restrict__ coef, int nsched,
                                     int* __restrict__ step, int* __restrict__ state, float* ring, const float* x, float* x_prov,
                                     float* x_prev, float* __restrict__ pred_x0) {
    const int64_t per_slot = (int64_t)C * (Ft - cond_f) * HW;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)slots * per_slot) return;
    const int s = (int)(i / per_slot);
    const int index = step[2 * s + 1];
    if (index < 0 || index >= nsched) return;            // idle (or a counter outside the table): nothing of this slot is written
    const int* fly = state + SLOT_STATE_WORDS * s + SLOT_IN_FLIGHT;
    int* next = state + SLOT_STATE_WORDS * s;
    const bool first = i == (int64_t)s * per_slot;
    const float* cf = coef + (int64_t)s * nsched * 4;
    const float e = cfg_eps_at(eps, 1, slots, C, Ft, cond_f, HW, scale[s], i);
    // entry k of the slot's ring, based so that [i] (an index over all slots) is this element: (3 s + k) per_slot + (i - s per_slot)
    float* const rs = ring + 2 * (int64_t)s * per_slot;
    const int phase = fly[0];
    if (phase == 1) {
        if (first) next[0] = 2, next[1] = 1, next[2] = 0;
        plms_update(e, 0, nullptr, nullptr, nullptr, i, cf, index, x, x_prov, nullptr, rs);
    } else if (phase == 2) {
        int newest = fly[2];
        if (newest < 0 || newest > 2) newest = 0;        // never index outside the ring
        if (first) step[2 * s] = index - 1, next[0] = 3;
        plms_update(e, 1, rs + newest * per_slot, nullptr, nullptr, i, cf, index, x, x_prev, pred_x0, nullptr);
    } else if (phase == 3) {
        int valid = fly[1], newest = fly[2];
        if (valid < 0 || valid > 3 || newest < 0 || newest > 2) valid = 0, newest = 2;
        const int slot = newest == 2 ? 0 : newest + 1;
        if (first) step[2 * s] = index - 1, next[1] = valid < 3 ? valid + 1 : 3, next[2] = slot;
        plms_update(e, valid == 0 ? 0 : valid + 1, rs + newest * per_slot, rs + (newest == 0 ? 2 : newest - 1) * per_slot,
                    rs + slot * per_slot, i, cf, index, x, x_prev, pred_x0, rs + slot * per_slot);
    } else {
        if (first) step[2 * s] = index - 1;
        ddim_update(e, cf, index, x, nullptr, x_prev, pred_x0, i);
    }
}

// pointwise channel mix on NCHW fp32 (VAE post_quant_conv, 4 -> 4): y[n,co,p] = sum_ci W[co,ci] x[n,ci,p] + b[co]
__global__ void conv1x1_nchw_kernel(const float* __restrict__ x, int N, int Cin, int Cout, int HW,
                                    const float* __restrict__ Wt, const float* __restrict__ bias, float* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)N * Cout * HW) return;
    const int p = (int)(i % HW);
    const int co = (int)((i / HW) % Cout);
    const int n = (int)(i / ((int64_t)HW * Cout));
    float acc = bias ? bias[co] : 0.f;
    for (int ci = 0; ci < Cin; ++ci) acc += Wt[co * Cin + ci] * x[((int64_t)n * Cin + ci) * HW + p];
    y[i] = acc;
}

__global__ void clamp01_kernel(float* __restrict__ x, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const float v = (x[i] + 1.0f) * 0.5f;
        x[i] = fminf(fmaxf(v, 0.f), 1.f);
    }
}

// DiagonalGaussianDistribution.sample: moments [N, 2C, HW] = (mean | logvar)
__global__ void gaussian_sample_kernel(const float* __restrict__ mom, int C, int HW, const float* __restrict__ noise,
                                       float* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t chw = (int64_t)C * HW;
    const int64_t img = i / chw, r = i - img * chw;
    const float mean = mom[img * 2 * chw + r];
    out[i] = noise ? gaussian_sample_f(mean, mom[img * 2 * chw + chw + r], noise[i]) : mean;
}

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

}  // namespace

extern "C" int seer_rotary_table(const float* freqs, int32_t T, int32_t half, float* cos_sin, void* stream) {
    if (!freqs || !cos_sin || T <= 0 || half <= 0) return SEER_EINVAL;
    const int n = T * half;
    hipLaunchKernelGGL(rotary_table_kernel, dim3((n + 255) / 256), dim3(256), 0, S(stream), freqs, T, half, cos_sin);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_rotary_inplace(void* x, int64_t rows, int32_t ld, int32_t col0_q, int32_t col0_k, int32_t heads,
                                   int32_t head_dim, int32_t rot_dim, int32_t tokens_per_batch, int32_t pos_offset,
                                   const float* cos_sin, void* stream) {
    if (!x || !cos_sin || rows <= 0 || heads <= 0 || rot_dim <= 0 || rot_dim % 8 || rot_dim > head_dim) return SEER_EINVAL;
    if (ld % 8 || col0_q % 8 || col0_k % 8 || head_dim % 8 || tokens_per_batch <= 0) return SEER_EINVAL;
    hipLaunchKernelGGL(rotary_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, S(stream),
                       reinterpret_cast<bf16*>(x), rows, ld, col0_q, col0_k, heads, head_dim, rot_dim, tokens_per_batch,
                       pos_offset, cos_sin);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_timestep_embedding(const int64_t* t, int32_t B, int32_t dim, int32_t flip_sin_to_cos,
                                       float freq_shift, float* out, void* stream) {
    if (!t || !out || B <= 0 || dim <= 0 || dim % 2) return SEER_EINVAL;
    const int n = B * dim / 2;
    hipLaunchKernelGGL(timestep_embedding_kernel, dim3((n + 255) / 256), dim3(256), 0, S(stream), t, B, dim,
                       flip_sin_to_cos, freq_shift, out);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

// kernels whose dynamic LDS may exceed the 64 KiB default: opt in once per kernel (160 KiB per CU on gfx950)
template <typename K>
int ensure_lds(K kernel, size_t bytes, std::atomic<bool>* done) {      // setting the attribute twice is harmless: the flag only has to be race-free
    if (bytes > 160 * 1024) return SEER_EINVAL;
    if (bytes > 64 * 1024 && !done->load(std::memory_order_acquire)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
            return SEER_ELAUNCH;
        done->store(true, std::memory_order_release);
    }
    return SEER_OK;
}

extern "C" int seer_linear_smallm(const float* x, int32_t B, int32_t K, const void* W, const float* bias, int32_t N,
                                  int32_t silu_in, int32_t silu_out, float* y, int32_t dtype, void* stream) {
    if (!x || !W || !y || B <= 0 || B > 8 || K <= 0 || K % 8 || N <= 0) return SEER_EINVAL;
    const size_t lds = (size_t)B * K * sizeof(float);
    static std::atomic<bool> done[4] = {{false}, {false}, {false}, {false}};
    // the batch class is the outer choice, the storage type the inner one; FLAG: the first of the class's two `done` flags
#define SEER_LSM(MB, R, GRID, FLAG)                                                                                                 \
    seer_dispatch_dtype(dtype, [&](auto f16) {                                                                                      \
        constexpr bool F16 = decltype(f16)::value;                                                                                  \
        const int rc = ensure_lds(linear_smallm_kernel<MB, R, F16>, lds, &done[FLAG + !F16]);                                       \
        if (rc != SEER_OK) return rc;                                                                                               \
        hipLaunchKernelGGL((linear_smallm_kernel<MB, R, F16>), dim3(GRID), dim3(256), lds, S(stream), x, B, K,                      \
                           reinterpret_cast<const bf16*>(W), bias, N, silu_in, silu_out, y);                                        \
        SEER_LAUNCH_CHECK();                                                                                                        \
        return SEER_OK;                                                                                                             \
    })
    if (B <= 2) return SEER_LSM(2, 4, (N + 15) / 16, 0);
    return SEER_LSM(8, 2, (N + 7) / 8, 2);
#undef SEER_LSM
}

extern "C" int seer_conv_in(const float* x, int32_t B, int32_t Cin, int32_t F, int32_t H, int32_t W_, const float* Wt,
                            const float* bias, int32_t Cout, void* y, int32_t dtype, void* stream) {
    static std::atomic<bool> done[2] = {{false}, {false}};
    return seer_dispatch_dtype(dtype, [&](auto f16) {
        constexpr bool F16 = decltype(f16)::value;
        if (!x || !Wt || !y || B <= 0 || Cin <= 0 || F <= 0 || H <= 0 || W_ <= 0 || Cout <= 0 || Cout % 8 || Cout > 2048)
            return SEER_EINVAL;
        const int ppb = 32;
        const size_t lds = ((size_t)9 * Cin * Cout + (size_t)ppb * 9 * Cin) * sizeof(float);
        const int rc = ensure_lds(conv_in_kernel<F16>, lds, &done[F16]);
        if (rc != SEER_OK) return rc;
        const int64_t npix = (int64_t)B * F * H * W_;
        hipLaunchKernelGGL(conv_in_kernel<F16>, dim3((unsigned)((npix + ppb - 1) / ppb)), dim3(256), lds, S(stream), x, B, Cin, F, H,
                           W_, Wt, bias, Cout, reinterpret_cast<bf16*>(y), ppb);
        SEER_LAUNCH_CHECK();
        return SEER_OK;
    });
}

extern "C" int seer_conv_out(const void* x, int32_t B, int32_t C0, int32_t F, int32_t H, int32_t W_, const float* Wt,
                             const float* bias, int32_t Cout, float* y, int32_t dtype, void* stream) {
    if (dtype != SEER_DT_BF16 && dtype != SEER_DT_F16) return SEER_EINVAL;
    if (!x || !Wt || !y || B <= 0 || C0 <= 0 || C0 % 8 || F <= 0 || H <= 0 || W_ <= 0) return SEER_EINVAL;
    const int64_t npix = (int64_t)B * F * H * W_;
    const int ppb = 32;
    dim3 grid((unsigned)((npix + ppb - 1) / ppb));
    const size_t lds = (size_t)Cout * 9 * C0 * sizeof(float);
    const bf16* xb = reinterpret_cast<const bf16*>(x);
    if (dtype == SEER_DT_F16) {
        if (Cout != 3) return SEER_ENOSYS;            // the VAE decoder's RGB head is the one fp16 consumer
        static std::atomic<bool> done16{false};
        const int rc = ensure_lds(conv_out_kernel<3, true>, lds, &done16);
        if (rc != SEER_OK) return rc;
        hipLaunchKernelGGL((conv_out_kernel<3, true>), grid, dim3(256), lds, S(stream), xb, B, C0, F, H, W_, Wt, bias, y, ppb);
    } else if (Cout == 4) {
        static std::atomic<bool> done{false};
        const int rc = ensure_lds(conv_out_kernel<4>, lds, &done);
        if (rc != SEER_OK) return rc;
        hipLaunchKernelGGL(conv_out_kernel<4>, grid, dim3(256), lds, S(stream), xb, B, C0, F, H, W_, Wt, bias, y, ppb);
    } else if (Cout == 3) {
        static std::atomic<bool> done{false};
        const int rc = ensure_lds(conv_out_kernel<3>, lds, &done);
        if (rc != SEER_OK) return rc;
        hipLaunchKernelGGL(conv_out_kernel<3>, grid, dim3(256), lds, S(stream), xb, B, C0, F, H, W_, Wt, bias, y, ppb);
    } else {
        return SEER_ENOSYS;
    }
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_cast_f32(const float* x, int64_t n, void* y, int32_t dtype, void* stream) {
    return seer_dispatch_dtype(dtype, [&](auto f16) {
        if (!x || !y || n <= 0) return SEER_EINVAL;
        const int64_t nt = (n + 3) / 4;
        hipLaunchKernelGGL(cast_f32_bf16_kernel<decltype(f16)::value>, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, S(stream), x, n,
                           reinterpret_cast<bf16*>(y));
        SEER_LAUNCH_CHECK();
        return SEER_OK;
    });
}

extern "C" int seer_nchw_f32_to_nhwc_bf16(const float* x, int32_t N, int32_t C, int32_t HW, void* y, void* stream) {
    if (!x || !y || N <= 0 || C <= 0 || HW <= 0) return SEER_EINVAL;
    dim3 grid((HW + 31) / 32, (C + 31) / 32, N);
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, grid, dim3(256), 0, S(stream), x, C, HW, reinterpret_cast<bf16*>(y));
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}
extern "C" int seer_nhwc_bf16_to_nchw_f32(const void* x, int32_t N, int32_t C, int32_t HW, float* y, void* stream) {
    if (!x || !y || N <= 0 || C <= 0 || HW <= 0) return SEER_EINVAL;
    dim3 grid((HW + 31) / 32, (C + 31) / 32, N);
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, grid, dim3(256), 0, S(stream), reinterpret_cast<const bf16*>(x), C, HW, y);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_cfg_ddim_step(const float* eps, int32_t cfg, int32_t b, int32_t C, int32_t F_total, int32_t cond_f,
                                  int32_t HW, float scale, const float* coef, int32_t index, const float* x,
                                  const float* noise, float* x_prev, float* pred_x0, void* stream) {
    if (!eps || !coef || !x || !x_prev || b <= 0 || C <= 0 || F_total <= cond_f || cond_f < 0 || HW <= 0 || index < 0)
        return SEER_EINVAL;
    const int64_t n = (int64_t)b * C * (F_total - cond_f) * HW;
    hipLaunchKernelGGL(cfg_ddim_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), eps, cfg, b, C,
                       F_total, cond_f, HW, scale, coef, index, x, noise, x_prev, pred_x0);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_ddim_step_begin(const float* x0_emb, const float* x, int32_t b, int32_t reps, int32_t C, int32_t f1,
                                    int32_t F_pred, int32_t HW, const int64_t* t_table, int32_t* step, float* sample,
                                    int64_t* t_out, void* stream) {
    if (!x || !t_table || !step || !sample || !t_out || b <= 0 || reps <= 0 || C <= 0 || f1 < 0 || F_pred <= 0 || HW <= 0 ||
        (f1 > 0 && !x0_emb))
        return SEER_EINVAL;
    const int64_t n = (int64_t)b * C * (f1 + F_pred) * HW;
    hipLaunchKernelGGL(ddim_assemble_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), x0_emb, x, b, reps, C, f1,
                       F_pred, HW, t_table, step, sample, t_out);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_cfg_ddim_step_dev(const float* eps, int32_t cfg, int32_t b, int32_t C, int32_t F_total, int32_t cond_f,
                                      int32_t HW, float scale, const float* coef, int32_t* step, const float* x,
                                      const float* noise, float* x_prev, float* pred_x0, void* stream) {
    if (!eps || !coef || !step || !x || !x_prev || b <= 0 || C <= 0 || F_total <= cond_f || cond_f < 0 || HW <= 0) return SEER_EINVAL;
    const int64_t n = (int64_t)b * C * (F_total - cond_f) * HW;
    hipLaunchKernelGGL(cfg_ddim_dev_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), eps, cfg, b, C, F_total,
                       cond_f, HW, scale, coef, step, x, noise, x_prev, pred_x0);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

// the slot kernels rely on 4-byte alignment of every pointer (the int64 tables included) and on a grid that fits one dimension
static inline bool slot_ptrs_ok(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if (reinterpret_cast<uintptr_t>(p) & 3) return false;
    return true;
}

extern "C" int seer_slot_step_begin(const float* x0_emb, const float* x, int32_t slots, int32_t reps, int32_t C, int32_t f1,
                                    int32_t F_pred, int32_t HW, const int64_t* t_table, int32_t nsched, int32_t* step, float* sample,
                                    int64_t* t_out, void* stream) {
    if (!x || !t_table || !step || !sample || !t_out || slots < 1 || nsched < 1 || (reps != 1 && reps != 2) || C <= 0 || f1 < 0 ||
        F_pred <= 0 || HW <= 0 || (f1 > 0 && !x0_emb))
        return SEER_EINVAL;
    if (!slot_ptrs_ok({x0_emb, x, t_table, step, sample, t_out})) return SEER_EINVAL;
    const int64_t n = (int64_t)slots * C * ((int64_t)f1 + F_pred) * HW;
    if ((n + 255) / 256 > 0x7fffffff) return SEER_EINVAL;
    hipLaunchKernelGGL(slot_assemble_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), x0_emb, x, slots, reps, C, f1,
                       F_pred, HW, reinterpret_cast<const int*>(t_table), nsched, step, sample, reinterpret_cast<int*>(t_out));
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_slot_cfg_ddim_step(const float* eps, int32_t slots, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                                       const float* scale, const float* coef, int32_t nsched, int32_t* step, const float* x,
                                       float* x_prev, float* pred_x0, void* stream) {
    if (!eps || !scale || !coef || !step || !x || !x_prev || slots < 1 || nsched < 1 || C <= 0 || cond_f < 0 || cond_f >= F_total ||
        HW <= 0)
        return SEER_EINVAL;
    if (!slot_ptrs_ok({eps, scale, coef, step, x, x_prev, pred_x0})) return SEER_EINVAL;
    const int64_t n = (int64_t)slots * C * ((int64_t)F_total - cond_f) * HW;
    if ((n + 255) / 256 > 0x7fffffff) return SEER_EINVAL;
    hipLaunchKernelGGL(slot_cfg_ddim_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), eps, slots, C, F_total, cond_f,
                       HW, scale, coef, nsched, step, x, x_prev, pred_x0);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

// the *_rng entry points: a clip's element index is a 32-bit Philox counter word times four, so a clip stays below 2^31 elements
static inline bool rng_clip_ok(int32_t C, int32_t F_total, int32_t cond_f, int32_t HW) {
    return C > 0 && HW > 0 && cond_f >= 0 && cond_f < F_total && (int64_t)C * ((int64_t)F_total - cond_f) * HW < ((int64_t)1 << 31);
}

static int launch_cfg_ddim_rng(const float* eps, int32_t cfg, int32_t b, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                               float scale, const float* coef, int32_t index, int32_t* step, const float* x, const uint32_t* seeds,
                               float temperature, float* x_prev, float* pred_x0, void* stream) {
    if (!eps || !coef || !x || !seeds || !x_prev || b <= 0 || !rng_clip_ok(C, F_total, cond_f, HW)) return SEER_EINVAL;
    if (!slot_ptrs_ok({eps, coef, step, x, seeds, x_prev, pred_x0})) return SEER_EINVAL;
    const int64_t n = (int64_t)b * C * ((int64_t)F_total - cond_f) * HW;
    if ((n + 255) / 256 > 0x7fffffff) return SEER_EINVAL;
    hipLaunchKernelGGL(cfg_ddim_rng_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), eps, cfg, b, C, F_total, cond_f,
                       HW, scale, coef, index, step, x, seeds, temperature, x_prev, pred_x0);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_cfg_ddim_step_rng(const float* eps, int32_t cfg, int32_t b, int32_t C, int32_t F_total, int32_t cond_f,
                                      int32_t HW, float scale, const float* coef, int32_t index, const float* x,
                                      const uint32_t* seeds, float temperature, float* x_prev, float* pred_x0, void* stream) {
    if (index < 0) return SEER_EINVAL;
    return launch_cfg_ddim_rng(eps, cfg, b, C, F_total, cond_f, HW, scale, coef, index, nullptr, x, seeds, temperature, x_prev, pred_x0,
                               stream);
}

extern "C" int seer_cfg_ddim_step_rng_dev(const float* eps, int32_t cfg, int32_t b, int32_t C, int32_t F_total, int32_t cond_f,
                                          int32_t HW, float scale, const float* coef, int32_t* step, const float* x,
                                          const uint32_t* seeds, float temperature, float* x_prev, float* pred_x0, void* stream) {
    if (!step) return SEER_EINVAL;
    return launch_cfg_ddim_rng(eps, cfg, b, C, F_total, cond_f, HW, scale, coef, 0, step, x, seeds, temperature, x_prev, pred_x0,
                               stream);
}

extern "C" int seer_slot_cfg_ddim_step_rng(const float* eps, int32_t slots, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                                           const float* scale, const float* coef, int32_t nsched, int32_t* step, const float* x,
                                           const uint32_t* seeds, const float* temperature, float* x_prev, float* pred_x0,
                                           void* stream) {
    if (!eps || !scale || !coef || !step || !x || !seeds || !temperature || !x_prev || slots < 1 || nsched < 1 ||
        !rng_clip_ok(C, F_total, cond_f, HW))
        return SEER_EINVAL;
    if (!slot_ptrs_ok({eps, scale, coef, step, x, seeds, temperature, x_prev, pred_x0})) return SEER_EINVAL;
    const int64_t n = (int64_t)slots * C * ((int64_t)F_total - cond_f) * HW;
    if ((n + 255) / 256 > 0x7fffffff) return SEER_EINVAL;
    hipLaunchKernelGGL(slot_cfg_ddim_rng_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), eps, slots, C, F_total,
                       cond_f, HW, scale, coef, nsched, step, x, seeds, temperature, x_prev, pred_x0);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

// given latents: exactly one of noise and seeds; a clip's element index is a Philox counter word, as in the *_rng entry points
static inline bool known_clip_ok(int32_t C, int32_t F_pred, int32_t HW) {
    return C > 0 && F_pred > 0 && HW > 0 && (int64_t)C * F_pred * HW < ((int64_t)1 << 31);
}

extern "C" int seer_q_sample(const float* x0, int32_t b, int64_t per_row, const float* coef, int32_t nsched, const int32_t* index,
                             const float* noise, const uint32_t* seeds, float* out, void* stream) {
    if (!x0 || !coef || !index || !out || (noise != nullptr) == (seeds != nullptr) || b <= 0 || nsched < 1 || per_row <= 0 ||
        per_row >= ((int64_t)1 << 31))
        return SEER_EINVAL;
    if (!slot_ptrs_ok({x0, coef, index, noise, seeds, out})) return SEER_EINVAL;
    const int64_t n = (int64_t)b * per_row;
    if ((n + 255) / 256 > 0x7fffffff) return SEER_EINVAL;
    hipLaunchKernelGGL(q_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), x0, b, per_row, coef, nsched, index,
                       noise, seeds, out);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_known_blend(float* x, const float* mask, const float* known, int32_t b, int32_t C, int32_t F_pred, int32_t HW,
                                const float* coef, int32_t index, const int32_t* step, const float* noise, const uint32_t* seeds,
                                void* stream) {
    if (!x || !mask || !known || !coef || (noise != nullptr) == (seeds != nullptr) || b <= 0 || !known_clip_ok(C, F_pred, HW))
        return SEER_EINVAL;
    if (!slot_ptrs_ok({x, mask, known, coef, step, noise, seeds})) return SEER_EINVAL;
    const int64_t n = (int64_t)b * C * F_pred * HW;
    if ((n + 255) / 256 > 0x7fffffff) return SEER_EINVAL;
    hipLaunchKernelGGL(known_blend_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), x, mask, known, b, C, F_pred, HW,
                       coef, index, step, noise, seeds);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_slot_known_blend(float* x, const float* mask, const float* known, int32_t slots, int32_t C, int32_t F_pred,
                                     int32_t HW, const float* coef, int32_t nsched, const int32_t* step, const uint32_t* seeds,
                                     void* stream) {
    if (!x || !mask || !known || !coef || !step || !seeds || slots < 1 || nsched < 1 || !known_clip_ok(C, F_pred, HW)) return SEER_EINVAL;
    if (!slot_ptrs_ok({x, mask, known, coef, step, seeds})) return SEER_EINVAL;
    const int64_t n = (int64_t)slots * C * F_pred * HW;
    if ((n + 255) / 256 > 0x7fffffff) return SEER_EINVAL;
    hipLaunchKernelGGL(slot_known_blend_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), x, mask, known, slots, C,
                       F_pred, HW, coef, nsched, step, seeds);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_slot_plms_step_begin(const float* x0_emb, const float* x, const float* x_prov, int32_t slots, int32_t reps,
                                         int32_t C, int32_t f1, int32_t F_pred, int32_t HW, const int64_t* t_table, int32_t nsched,
                                         int32_t* step, int32_t* state, float* sample, int64_t* t_out, void* stream) {
    if (!x || !x_prov || !t_table || !step || !state || !sample || !t_out || slots < 1 || nsched < 1 || (reps != 1 && reps != 2) ||
        C <= 0 || f1 < 0 || F_pred <= 0 || HW <= 0 || (f1 > 0 && !x0_emb) || x_prov == x)
        return SEER_EINVAL;
    if (!slot_ptrs_ok({x0_emb, x, x_prov, t_table, step, state, sample, t_out})) return SEER_EINVAL;
    const int64_t n = (int64_t)slots * C * ((int64_t)f1 + F_pred) * HW;
    if ((n + 255) / 256 > 0x7fffffff) return SEER_EINVAL;
    hipLaunchKernelGGL(slot_plms_assemble_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), x0_emb, x, x_prov, slots,
                       reps, C, f1, F_pred, HW, reinterpret_cast<const int*>(t_table), nsched, step, state, sample,
                       reinterpret_cast<int*>(t_out));
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_slot_cfg_plms_step(const float* eps, int32_t slots, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                                       const float* scale, const float* coef, int32_t nsched, int32_t* step, int32_t* state,
                                       float* ring, const float* x, float* x_prov, float* x_prev, float* pred_x0, void* stream) {
    if (!eps || !scale || !coef || !step || !state || !ring || !x || !x_prov || !x_prev || slots < 1 || nsched < 1 || C <= 0 ||
        cond_f < 0 || cond_f >= F_total || HW <= 0 || x_prov == x)
        return SEER_EINVAL;
    if (!slot_ptrs_ok({eps, scale, coef, step, state, ring, x, x_prov, x_prev, pred_x0})) return SEER_EINVAL;
    const int64_t n = (int64_t)slots * C * ((int64_t)F_total - cond_f) * HW;
    if ((n + 255) / 256 > 0x7fffffff) return SEER_EINVAL;
    hipLaunchKernelGGL(slot_cfg_plms_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), eps, slots, C, F_total, cond_f,
                       HW, scale, coef, nsched, step, state, ring, x, x_prov, x_prev, pred_x0);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_cfg_plms_step(const float* eps, int32_t cfg, int32_t b, int32_t C, int32_t F_total, int32_t cond_f,
                                  int32_t HW, float scale, const float* coef, int32_t index, int32_t order, const float* x,
                                  const float* h1, const float* h2, const float* h3, float* x_prev, float* pred_x0, float* e_out,
                                  void* stream) {
    if (!eps || !coef || !x || !x_prev || b <= 0 || C <= 0 || F_total <= cond_f || cond_f < 0 || HW <= 0 || index < 0 ||
        order < 0 || order > 4 || (order >= 1 && !h1) || (order >= 3 && !h2) || (order >= 4 && !h3))
        return SEER_EINVAL;
    const int64_t n = (int64_t)b * C * (F_total - cond_f) * HW;
    hipLaunchKernelGGL(cfg_plms_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), eps, cfg, b, C, F_total,
                       cond_f, HW, scale, coef, index, order, x, h1, h2, h3, x_prev, pred_x0, e_out);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_cfg_plms_step_dev(const float* eps, int32_t cfg, int32_t b, int32_t C, int32_t F_total, int32_t cond_f,
                                      int32_t HW, float scale, const float* coef, int32_t* step, float* ring, int32_t* ring_state,
                                      const float* x, float* x_prev, float* pred_x0, void* stream) {
    if (!eps || !coef || !step || !ring || !ring_state || !x || !x_prev || b <= 0 || C <= 0 || F_total <= cond_f || cond_f < 0 ||
        HW <= 0)
        return SEER_EINVAL;
    const int64_t n = (int64_t)b * C * (F_total - cond_f) * HW;
    hipLaunchKernelGGL(cfg_plms_dev_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), eps, cfg, b, C, F_total,
                       cond_f, HW, scale, coef, step, ring, ring_state, x, x_prev, pred_x0);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_conv1x1_nchw_f32(const float* x, int32_t N, int32_t Cin, int32_t Cout, int32_t HW, const float* Wt,
                                     const float* bias, float* y, void* stream) {
    if (!x || !Wt || !y || N <= 0 || Cin <= 0 || Cout <= 0 || HW <= 0) return SEER_EINVAL;
    const int64_t n = (int64_t)N * Cout * HW;
    hipLaunchKernelGGL(conv1x1_nchw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), x, N, Cin, Cout,
                       HW, Wt, bias, y);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_clamp01(float* x, int64_t n, void* stream) {
    if (!x || n <= 0) return SEER_EINVAL;
    hipLaunchKernelGGL(clamp01_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), x, n);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_gaussian_sample(const float* moments, int32_t N, int32_t C, int32_t HW, const float* noise, float* out,
                                    void* stream) {
    if (!moments || !out || N <= 0 || C <= 0 || HW <= 0) return SEER_EINVAL;
    const int64_t n = (int64_t)N * C * HW;
    hipLaunchKernelGGL(gaussian_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), moments, C, HW,
                       noise, out, n);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_abi_version(void) { return 26; }
extern "C" const char* seer_build_arch(void) { return "gfx950"; }
extern "C" const char* seer_strerror(int code) {
    switch (code) {
        case SEER_OK: return "ok";
        case SEER_EINVAL: return "invalid argument (shape/alignment/flags)";
        case SEER_ENOSYS: return "shape class not built";
        case SEER_ELAUNCH: return "kernel launch failed";
        default: return "unknown error";
    }
}
