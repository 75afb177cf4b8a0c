// The second pass of a split-K seer_gemm_bf16 launch: C = epilogue( sum of the K slices the tile units left in the workspace ).
#include "gemm_tiles.h"

namespace {

// split-K second pass: C = epilogue( sum over slices, in slice order ).  One quad of 4 output columns of row m; returns the
// four values as stored (bf16-rounded unless the output is fp32).
__device__ __forceinline__ f32x4 splitk_reduce_quad(const seer_gemm_desc& p, int m, int n) {
    const float* ws = reinterpret_cast<const float*>(p.workspace) + (int64_t)m * p.N + n;
    f32x4 a = *reinterpret_cast<const f32x4*>(ws);
#pragma unroll 4
    for (int z = 1; z < p.splits; ++z) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(ws + (int64_t)z * p.M * p.N);
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] += b[r];
    }
    float v[4] = {a[0], a[1], a[2], a[3]};
    if (p.bias) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(p.bias + n);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += bv[r];
    }
    if (p.rowvec) {
        const f32x4 tv = *reinterpret_cast<const f32x4*>(p.rowvec + (int64_t)(m / p.rows_per_batch) * p.rowvec_ld + n);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += tv[r];
    }
    if (p.epilogue & SEER_EPI_SILU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = silu_f(v[r]);
    }
    if (p.epilogue & SEER_EPI_QUICKGELU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = quick_gelu_f(v[r]);
    }
    if ((p.epilogue & SEER_EPI_COLSCALE) && n < p.col_scale_cols) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] *= p.col_scale;
    }
    const bool h16 = (p.epilogue & SEER_EPI_F16) != 0;      // IEEE-half storage (the fp16 engine): same bytes, other conversions
    if (p.residual) {
        const u32x2 rv = *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16*>(p.residual) + (int64_t)m * p.ldr + n);
        if (h16) {
            const f32x2 r01 = unpack2t<true>(rv[0]), r23 = unpack2t<true>(rv[1]);
            v[0] += r01[0]; v[1] += r01[1]; v[2] += r23[0]; v[3] += r23[1];
        } else {
            v[0] += __builtin_bit_cast(float, rv[0] << 16);
            v[1] += __builtin_bit_cast(float, rv[0] & 0xffff0000u);
            v[2] += __builtin_bit_cast(float, rv[1] << 16);
            v[3] += __builtin_bit_cast(float, rv[1] & 0xffff0000u);
        }
    }
    if (p.epilogue & SEER_EPI_OUT_F32) {
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.C) + (int64_t)m * p.ldc + n) = f32x4{v[0], v[1], v[2], v[3]};
        return f32x4{v[0], v[1], v[2], v[3]};
    }
    u32x2 o;
    if (h16) {
        o[0] = pack2h(v[0], v[1]);
        o[1] = pack2h(v[2], v[3]);
        *reinterpret_cast<u32x2*>(reinterpret_cast<bf16*>(p.C) + (int64_t)m * p.ldc + n) = o;
        const f32x2 s01 = unpack2t<true>(o[0]), s23 = unpack2t<true>(o[1]);
        return f32x4{s01[0], s01[1], s23[0], s23[1]};
    }
    o[0] = pack2(v[0], v[1]);
    o[1] = pack2(v[2], v[3]);
    *reinterpret_cast<u32x2*>(reinterpret_cast<bf16*>(p.C) + (int64_t)m * p.ldc + n) = o;
    return f32x4{__builtin_bit_cast(float, o[0] << 16), __builtin_bit_cast(float, o[0] & 0xffff0000u),
                 __builtin_bit_cast(float, o[1] << 16), __builtin_bit_cast(float, o[1] & 0xffff0000u)};
}

__global__ void __launch_bounds__(256) seer_splitk_reduce_kernel(const seer_gemm_desc p) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int n4 = p.N / 4;
    if (idx >= (int64_t)p.M * n4) return;
    const int m = (int)(idx / n4);
    const int n = (int)(idx - (int64_t)m * n4) * 4;
    (void)splitk_reduce_quad(p, m, n);
}

// the same pass with column sums (seer_gemm_desc::colsum): a block owns splitk_cs_rows(M) rows x 256 columns, thread -> (column
// quad, row lane) with the rows of a lane added in order, the four row lanes of a column added in order by its thread;
// colsum[ceil(M / rows)][N][2].  Few rows (the 4x4 / 8x8 levels): one row per thread, as many blocks as the plain reduce pass --
// at 16 rows per block the 384-row convs ran 120 blocks of 64-deep load chains, +12 us (profiles/r02_gn_colsums.log).
// (Round 2 took this kernel out when a two-process test differed in the last bits with column sums on; the cause was elsewhere --
// a packed-fp32 instruction form in the rotary epilogue, profiles/r03_flake_root_cause.md -- and it is back.)
// (splitk_cs_rows / splitk_fx_rows: gemm_tiles.h, the planner answers the host queries with them)
__global__ void __launch_bounds__(256) seer_splitk_reduce_colsum_kernel(const seer_gemm_desc p) {
    __shared__ float part[4][64][8];
    const int cq = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int n = (blockIdx.x * 64 + cq) * 4;
    const int cs_rows = splitk_cs_rows(p.M, p.tile == SEER_TILE_AUTO_INVARIANT);
    const int mb = blockIdx.y * cs_rows;
    float sm[4] = {0.f, 0.f, 0.f, 0.f}, sq[4] = {0.f, 0.f, 0.f, 0.f};
    if (n < p.N) {
        for (int m = mb + rl; m < min(mb + cs_rows, p.M); m += 4) {
            const f32x4 v = splitk_reduce_quad(p, m, n);
#pragma unroll
            for (int r = 0; r < 4; ++r) { sm[r] += v[r]; sq[r] += v[r] * v[r]; }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) { part[rl][cq][r * 2] = sm[r]; part[rl][cq][r * 2 + 1] = sq[r]; }
    __syncthreads();
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col < p.N) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            a += part[k][threadIdx.x >> 2][(threadIdx.x & 3) * 2];
            b += part[k][threadIdx.x >> 2][(threadIdx.x & 3) * 2 + 1];
        }
        *reinterpret_cast<f32x2*>(p.colsum + ((int64_t)blockIdx.y * p.N + col) * 2) = f32x2{a, b};
    }
}

// the same pass for ACCUMULATED column sums (seer_gemm_desc::colsum_fx).  The atomics are the cost here (one per address every
// ~12 ns, ~1.3 TB/s of them chip-wide): a block owns RB = RL * RPL rows x CB columns and adds ONE pair per column -- 16 x fewer
// than one per 4-row strip (measured with 4 / 16-row strips: +10..15 us per conv, profiles/r04_gn_fx_producers.md).  Thread -> (column
// quad, row lane); the row lanes of a column are added in order by the column's thread.
template <int CB, int RL, int RPL>
__global__ void __launch_bounds__(256) seer_splitk_reduce_fx_kernel(const seer_gemm_desc p) {
    constexpr int NQ = CB / 4, RB = RL * RPL;
    static_assert(NQ * RL == 256, "one thread per (column quad, row lane)");
    __shared__ float part[RL][NQ][8];
    const int cq = threadIdx.x % NQ, rl = threadIdx.x / NQ;
    const int n = blockIdx.x * CB + cq * 4;
    const int mb = blockIdx.y * RB;
    float sm[4] = {0.f, 0.f, 0.f, 0.f}, sq[4] = {0.f, 0.f, 0.f, 0.f};
    if (n < p.N) {
#pragma unroll
        for (int i = 0; i < RPL; ++i) {
            const int m = mb + rl + i * RL;
            if (m < p.M) {
                const f32x4 v = splitk_reduce_quad(p, m, n);
#pragma unroll
                for (int r = 0; r < 4; ++r) { sm[r] += v[r]; sq[r] += v[r] * v[r]; }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) { part[rl][cq][r * 2] = sm[r]; part[rl][cq][r * 2 + 1] = sq[r]; }
    __syncthreads();
    const int col = blockIdx.x * CB + threadIdx.x;
    if (threadIdx.x < CB && col < p.N) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int k = 0; k < RL; ++k) {
            a += part[k][threadIdx.x >> 2][(threadIdx.x & 3) * 2];
            b += part[k][threadIdx.x >> 2][(threadIdx.x & 3) * 2 + 1];
        }
        int64_t* o = fx_slot(p, blockIdx.y, mb) + col;
        fx_add(o, a);
        fx_add(o + p.N, b);
    }
}

}  // namespace

int seer_gemm_reduce_launch(const seer_gemm_desc& d, int reduce, hipStream_t st) {
    if (reduce == SEER_GEMM_REDUCE_COLSUM_FX64) {
        hipLaunchKernelGGL((seer_splitk_reduce_fx_kernel<64, 16, 4>), dim3((unsigned)((d.N + 63) / 64), (unsigned)((d.M + 63) / 64)),
                           dim3(256), 0, st, d);
    } else if (reduce == SEER_GEMM_REDUCE_COLSUM_FX32) {
        hipLaunchKernelGGL((seer_splitk_reduce_fx_kernel<32, 32, 1>), dim3((unsigned)((d.N + 31) / 32), (unsigned)((d.M + 31) / 32)),
                           dim3(256), 0, st, d);
    } else if (reduce == SEER_GEMM_REDUCE_COLSUM) {
        const int cs_rows = splitk_cs_rows(d.M, d.tile == SEER_TILE_AUTO_INVARIANT);
        hipLaunchKernelGGL(seer_splitk_reduce_colsum_kernel, dim3((unsigned)((d.N + 255) / 256),
                           (unsigned)((d.M + cs_rows - 1) / cs_rows)), dim3(256), 0, st, d);
    } else {
        const int64_t n = (int64_t)d.M * (d.N / 4);
        hipLaunchKernelGGL(seer_splitk_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d);
    }
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}
