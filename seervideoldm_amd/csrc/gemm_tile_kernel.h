// The tile kernel of seer_gemm_bf16 and its launchers: bf16 MFMA GEMM / implicit-GEMM 3x3 convolution for gfx950 (MI355X).
// A header: the build units gemm_tiles_*.hip (gemm_tile_units.inc) each emit the instantiations of their rows of gemm_tiles.h.
//
//   C[m, n] = epilogue( sum_k A(m, k) * W[n, k] )        (see include/seer_hip.h, seer_gemm_bf16)
//
// Structure (v1): 256 threads = 4 waves (2 x 2), block tile BM x BN x 64, v_mfma_f32_16x16x32_bf16,
// LDS tiles of 128-byte rows with a 16-byte-chunk XOR swizzle (chunk ^= row & 7: conflict-free
// ds_read_b128 fragment reads), register-staged global->LDS double buffering with ONE barrier per K tile
// (loads for tile t+1 are issued before the MFMAs of tile t and written to the other buffer after them).
// The MFMA is issued "swapped" (W fragment as the A operand, activation fragment as the B operand) so that
// every lane ends up holding 4 CONSECUTIVE output columns of one output row: the epilogue (bias, time-embedding
// row vector, residual, GEGLU, SiLU) works on 4-wide vectors and stores 8 bytes per lane.
//
// Implicit GEMM conv: k = (ky, kx, ci); Cin % 64 == 0 so a 64-wide K tile never straddles a filter tap; the
// tap -> pixel offset is wave-uniform scalar work, the per-row pixel decode is hoisted out of the K loop.
#pragma once
#include "gemm_tiles.h"
#include <mutex>
#include <type_traits>

// Measurement build only (-DSEER_GEMM_STAMPS, scripts/lab_pp8stamps.cpp): every wave of the first 64 blocks records
// wall_clock64() at the phase boundaries of its tile.  256x256 tile: entry, prologue issued, prologue landed, K loop done, rows
// re-aligned, epilogue math done, tile staged, tile stored.  LDS-direct ring tiles: entry, set-up done, first K tile landed,
// K loop done, then epilogue math done, tile staged, tile stored (split-K: partial tile stored).
#ifdef SEER_GEMM_STAMPS
__device__ long long seer_pp8_stamps[64 * 8 * 16];
extern "C" long long* seer_lab_pp8_stamps() {
    long long* p = nullptr;
    (void)hipGetSymbolAddress(reinterpret_cast<void**>(&p), HIP_SYMBOL(seer_pp8_stamps));
    return p;
}
// entry / exit time of wave 0 of every block (first 8192 blocks of z = 0): the dispatch ramp and the tail of a launch
__device__ long long seer_block_span[8192 * 2];
extern "C" long long* seer_lab_block_span() {
    long long* p = nullptr;
    (void)hipGetSymbolAddress(reinterpret_cast<void**>(&p), HIP_SYMBOL(seer_block_span));
    return p;
}
#define PSPAN(which)                                                                                                   \
    do {                                                                                                               \
        if (threadIdx.x == 0 && blockIdx.z == 0 && blockIdx.x < 8192) seer_block_span[blockIdx.x * 2 + (which)] = wall_clock64(); \
    } while (0)
#define PSTAMP()                                                                                                       \
    do {                                                                                                               \
        if (blockIdx.x < 64 && blockIdx.z == 0 && (threadIdx.x & 63) == 0 && nst_ < 16)                                \
            seer_pp8_stamps[(blockIdx.x * 8 + (threadIdx.x >> 6)) * 16 + nst_] = wall_clock64();                       \
        ++nst_;                                                                                                        \
    } while (0)
#else
#define PSTAMP() do { } while (0)
#define PSPAN(which) do { } while (0)
#endif

namespace {

// measurement-only builds (scripts/probe_gemm.sh; results are WRONG): bit 0 = no global->LDS refills inside the K loop,
// bit 1 = no LDS fragment reads, bit 2 = no MFMAs.  The shipped library is built with 0.
#ifndef SEER_GEMM_PROBE
#define SEER_GEMM_PROBE 0
#endif

// 16 zero bytes: the source of out-of-image taps for the LDS-direct (global_load_lds) conv gather
__device__ __attribute__((aligned(16))) unsigned int seer_zero_page[4] = {0u, 0u, 0u, 0u};

template <int BM, int BN, bool CONV, bool GEGLU, bool SPLIT, int NS, int WM = 2, int WN = 2, bool F16 = false>
__global__ void __launch_bounds__(64 * WM * WN) seer_gemm_kernel(const seer_gemm_desc p) {
    using TS = TileShape<BM, BN, NS, WM, WN>;
    constexpr int NT = TS::NT;                     // threads per block
    constexpr int RPP = NT / 8;                    // tile rows staged per pass (8 lanes x 16 B cover one 128-B row)
    constexpr int WTM = BM / WM, WTN = BN / WN;
    constexpr bool PP8 = TS::PP8;
    static_assert(WN == 2 || PP8, "wave grids other than WM x 2 exist only as the 256 x 256 ping-pong kernel");
    constexpr int TM = WTM / 16, TN = WTN / 16;
    constexpr int A_CH = BM / RPP, B_CH = BN / RPP;  // 16-byte chunks per thread per K tile
    static_assert(BM % RPP == 0 && BN % RPP == 0, "tile rows must be a multiple of the rows staged per pass");
    static_assert(!GEGLU || (TN % 2 == 0), "GEGLU needs value/gate n-tile pairs inside one wave");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int STAGE = TS::STAGE;             // elements per stage: [A tile BM x 64][B tile BN x 64]
    bf16* const smem_b = reinterpret_cast<bf16*>(smem);

    [[maybe_unused]] int nst_ = 0;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // scalar: LDS-DMA destinations stay in SGPRs
    const int wm = wave / WN, wn = wave % WN;
    PSTAMP();
    PSPAN(0);

    // ---- block -> tile mapping: XCD-contiguous chunks (blocks b and b+8 share an XCD), grouped along M
    const int tiles_m = (p.M + BM - 1) / BM;
    const int tiles_n = (p.N + BN - 1) / BN;
    const int nwg = tiles_m * tiles_n;
    int wg;
    {
        const int L = blockIdx.x;
        const int xcd = L & 7;
        const int q = nwg >> 3, r = nwg & 7;
        wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (L >> 3);
    }
#ifndef SEER_GEMM_GM
#define SEER_GEMM_GM 4          // M tiles per block group (round 1 chose 8 from a back-to-back sweep, profiles/r01_gemm_group_sweep.log; inside the
                               // step -- cold operands -- 4 is the best of 1, 2, 3, 4, 6, 8, 16, 32: 9.59 against 9.64 ms and 9.77 against 9.81 on two
                               // boxes, profiles/r06_gemm_group_in_step.log)
#endif
    constexpr int GM = SEER_GEMM_GM;
    const int group = wg / (GM * tiles_n);
    const int first_m = group * GM;
    const int gsz = min(tiles_m - first_m, GM);
    const int tm = first_m + (wg % (GM * tiles_n)) % gsz;
    const int tn = (wg % (GM * tiles_n)) / gsz;
    const int m0 = tm * BM, n0 = tn * BN;

    const int z = SPLIT ? 0 : blockIdx.z;          // SPLIT: blockIdx.z is the K slice, not a batch index
    const bf16* __restrict__ A = reinterpret_cast<const bf16*>(p.A) + (int64_t)z * p.strideA;
    const bf16* __restrict__ A2 = reinterpret_cast<const bf16*>(p.A2);
    const bf16* __restrict__ W = reinterpret_cast<const bf16*>(p.W) + (int64_t)z * p.strideW;

    // ---- per-thread staging descriptors
    const int c8 = (tid & 7) * 8;     // element offset of this thread's chunk inside the K tile
    const int srow = tid >> 3;        // 0..RPP-1
    int64_t a_off[A_CH];              // plain: row offset into A ; conv: image base offset
    int64_t a_off2[A_CH];
    int a_oy[A_CH], a_ox[A_CH];
    // PP8 stages half tiles: chunk c = 2 * half + i is one 8-row group of "half" (the rows of quadrant-row `half` of both wave
    // rows: tile rows wm * 128 + half * 64 + [0, 64); 16 of them per wave), see the main loop
    auto a_tile_row = [&](int c) { return PP8 ? (wave >> 2) * 128 + (c >> 1) * 64 + 16 * (wave & 3) + 8 * (c & 1) + (lane >> 3) : srow + RPP * c; };
    auto b_tile_row = [&](int c) {
        const int hn = 16 * wave + 8 * (c & 1) + (lane >> 3);
        return PP8 ? (hn >> 5) * 64 + (c >> 1) * 32 + (hn & 31) : srow + RPP * c;
    };
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
        int gm = m0 + a_tile_row(i);
        gm = gm < p.M ? gm : p.M - 1;
        if constexpr (CONV) {
            // upsample == 2: one of the four 2x2 phase convs of "nearest 2x + conv3x3" (seer_hip.h): rows index the SOURCE
            // grid, output pixel (2 y + a, 2 x + b) of phase (a, b) = blockIdx.z reads source rows y + a - 1 + {0, 1}
            const bool phase_mode = p.upsample == 2;
            const int gw = phase_mode ? p.Win : p.Wout;
            const int hw = phase_mode ? p.Hin * p.Win : p.Hout * p.Wout;
            const int img = gm / hw;
            const int rem = gm - img * hw;
            const int oy = rem / gw;
            const int pad0 = p.pad_after_only ? 0 : 1;     // rows / columns of padding before the image
            a_oy[i] = phase_mode ? oy + ((int)blockIdx.z >> 1) - 1 : oy * p.stride - pad0;
            a_ox[i] = phase_mode ? (rem - oy * gw) + ((int)blockIdx.z & 1) - 1 : (rem - oy * gw) * p.stride - pad0;
            a_off[i] = (int64_t)img * p.Hin * p.Win * p.Cin;
            a_off2[i] = 0;
        } else {
            a_off[i] = (int64_t)gm * p.lda;
            a_off2[i] = (int64_t)gm * p.lda2;
            // the same row relative to the tile's first row, in ELEMENTS (32 bits): the LDS-direct fetches address
            // "wave-uniform 64-bit base + one VGPR" (global_load_lds v, s[..]) instead of forming a 64-bit address per piece
            a_oy[i] = (gm - m0) * p.lda;
            a_ox[i] = (gm - m0) * p.lda2;
        }
    }
    // LDS-direct conv gather without per-piece address arithmetic (not the nearest-2x read-through form, whose source pixel is not
    // affine in the tap): a_pix = byte offset of tap (0, 0) of the piece row's pixel, this lane's chunk included; bit 9 i + tap of
    // a_okb[i / 3]: tap inside the image.  A K tile then costs one scalar tap offset and, per piece, a select between
    // a_pix + tap offset and an offset past the end of the tensor, which the buffer bounds check turns into zeros -- no 64-bit
    // address, no zero page, no branch, no division (round 4: the loop is bound by instruction issue, profiles/r04_t320_stamps.log)
    [[maybe_unused]] int a_pix[A_CH];
    [[maybe_unused]] unsigned a_okb[(A_CH + 2) / 3] = {};
    [[maybe_unused]] unsigned a_bytes = 0;
    bool conv_fast = false;
    if constexpr (CONV && NS >= 2) {
        const int64_t hw_out = p.upsample == 2 ? (int64_t)p.Hin * p.Win : (int64_t)p.Hout * p.Wout;
        const int64_t in_bytes = (p.M / hw_out) * p.Hin * p.Win * p.Cin * 2;
        conv_fast = p.upsample != 1 && in_bytes < ((int64_t)1 << 31) && (int64_t)p.K * p.Cin < ((int64_t)1 << 32);
        a_bytes = (unsigned)in_bytes;
        if (conv_fast) {
            const int ksz = p.upsample == 2 ? 2 : 3;
            const int sch = ((tid & 7) ^ (srow & 7)) * 8;
#pragma unroll
            for (int i = 0; i < A_CH; ++i) {
                const int iy0 = a_oy[i], ix0 = a_ox[i];
                a_pix[i] = (int)(a_off[i] + ((int64_t)iy0 * p.Win + ix0) * p.Cin + sch) * 2;
                unsigned bits = 0u;
                for (int ky = 0; ky < ksz; ++ky)
                    for (int kx = 0; kx < ksz; ++kx)
                        if (iy0 + ky >= 0 && iy0 + ky < p.Hin && ix0 + kx >= 0 && ix0 + kx < p.Win) bits |= 1u << (ky * ksz + kx);
                a_okb[i / 3] |= bits << (9 * (i % 3));
            }
        }
    }
    const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(A), 0, (int)a_bytes, 0x00020000);
    const unsigned cin_magic = CONV ? 0xFFFFFFFFu / (unsigned)(p.Cin > 0 ? p.Cin : 1) + 1u : 0u;     // tap = umulhi(kbase, magic)
    // plain operands of the LDS-direct ring as buffer resources over the tile's rows (see issue_tile)
    const __amdgpu_buffer_rsrc_t r_a1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(A + (CONV ? 0 : (int64_t)m0 * p.lda)), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_a2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(A2 && !CONV ? A2 + (int64_t)m0 * p.lda2 : A), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(W + (int64_t)n0 * p.K), 0, 0x7fffffff, 0x00020000);

    int64_t b_off[B_CH];
    int b_rel[B_CH];                  // (gn - n0) * K: the W row relative to the tile's first, in elements
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
        int gn = n0 + b_tile_row(i);
        gn = gn < p.N ? gn : p.N - 1;
        b_off[i] = (int64_t)gn * p.K;
        b_rel[i] = (gn - n0) * p.K;
    }

    u32x4 areg[A_CH], breg[B_CH];

    auto load_tile = [&](int kt) {
        const int kbase = kt * BK;
        if constexpr (CONV) {
            const int tap = kbase / p.Cin;
            const int ci0 = kbase - tap * p.Cin;
            const int ksz = p.upsample == 2 ? 2 : 3;
            const int ky = tap / ksz, kx = tap - ky * ksz;
            const int Hs = p.upsample == 1 ? p.Hin * 2 : p.Hin;
            const int Ws = p.upsample == 1 ? p.Win * 2 : p.Win;
#pragma unroll
            for (int i = 0; i < A_CH; ++i) {
                const int iy = a_oy[i] + ky, ix = a_ox[i] + kx;
                const bool ok = (iy >= 0) & (iy < Hs) & (ix >= 0) & (ix < Ws);
                const int sy = p.upsample == 1 ? (iy >> 1) : iy;
                const int sx = p.upsample == 1 ? (ix >> 1) : ix;
                u32x4 v = {0u, 0u, 0u, 0u};
                if (ok) {
                    const bf16* src = A + a_off[i] + ((int64_t)sy * p.Win + sx) * p.Cin + ci0 + c8;
                    v = *reinterpret_cast<const u32x4*>(src);
                }
                areg[i] = v;
            }
        } else {
            const bool second = kbase >= p.K1;
#pragma unroll
            for (int i = 0; i < A_CH; ++i) {
                const bf16* src = second ? (A2 + a_off2[i] + (kbase - p.K1) + c8) : (A + a_off[i] + kbase + c8);
                areg[i] = *reinterpret_cast<const u32x4*>(src);
            }
        }
#pragma unroll
        for (int i = 0; i < B_CH; ++i) {
            breg[i] = *reinterpret_cast<const u32x4*>(W + b_off[i] + kbase + c8);
        }
    };
    auto store_tile = [&](int buf) {
        bf16* as = smem_b + buf * STAGE;
        bf16* bs = as + BM * BK;
        const int sw = ((tid & 7) ^ (srow & 7)) * 8;   // (row & 7) == (srow & 7) because rows step by RPP (a multiple of 8)
#pragma unroll
        for (int i = 0; i < A_CH; ++i) *reinterpret_cast<u32x4*>(as + (srow + RPP * i) * BK + sw) = areg[i];
#pragma unroll
        for (int i = 0; i < B_CH; ++i) *reinterpret_cast<u32x4*>(bs + (srow + RPP * i) * BK + sw) = breg[i];
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- residual tile prefetch: the epilogue's bf16 residual (8 B per accumulator quad) is requested before the K loop so
    // its HBM/L2 latency hides under the main loop instead of adding a dependent round trip to every block's tail
    const bf16* R = reinterpret_cast<const bf16*>(p.residual);
    constexpr bool RES_PRE = !GEGLU && !SPLIT && TM * TN <= 16;     // the 256x256 tile has no registers to spare for it
    u32x2 rpre[RES_PRE ? TM : 1][RES_PRE ? TN : 1];
    if constexpr (RES_PRE) {
        if (R) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int m = m0 + wm * WTM + i * 16 + (lane & 15);
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n = n0 + wn * WTN + j * 16 + (lane >> 4) * 4;
                    rpre[i][j] = (m < p.M && n < p.N) ? *reinterpret_cast<const u32x2*>(R + (int64_t)m * p.ldr + n)
                                                        : u32x2{0u, 0u};
                }
            }
        }
    }

    // folded LayerNorm (seer_gemm_desc::ln_rowstat): thread t < BM REQUESTS the accumulated (sum, sum of squares) of tile row t here
    // and keeps the raw pair through the K loop; the epilogue converts it and hands (mean * rstd, rstd) to the lanes that own the
    // row through LDS.  (Converting here put a wait for the load -- an L2 round trip -- in front of the first LDS-DMA of every
    // tile: +3 us on the GEGLU projections with their 7.5 tiles per CU, profiles/r04_ln_fold_overheads.md.)
    constexpr bool LN_OK = !SPLIT && TS::ln_ok;
    typedef __attribute__((ext_vector_type(2))) long long i64x2;
    i64x2 ln_raw = {0, 0};
    if constexpr (LN_OK) {
        if (p.ln_rowstat && tid < BM) {
            const int m = min(m0 + tid, p.M - 1);
            ln_raw = *reinterpret_cast<const i64x2*>(reinterpret_cast<const long long*>(p.ln_rowstat) + (int64_t)m * 2);
        }
    }
    // ... and the lane's wsum quads, requested before the K loop like the bias (a dependent L2 round trip at the head of the
    // epilogue otherwise)
    f32x4 spre[LN_OK ? TN : 1];
    if constexpr (LN_OK) {
        if (p.ln_rowstat) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn * WTN + j * 16 + (lane >> 4) * 4;
                spre[j] = n < p.N ? *reinterpret_cast<const f32x4*>(p.ln_wsum + n) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }

    // bias prefetch, same reason (a dependent L2 round trip at the head of every block's epilogue otherwise); the 160-wide
    // tiles have no registers to spare for it
    constexpr bool BIAS_PRE = !SPLIT && TN <= 4 && !PP8;
    f32x4 bpre[TN];
    if constexpr (BIAS_PRE) {
        if (p.bias) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn * WTN + j * 16 + (lane >> 4) * 4;
                bpre[j] = n < p.N ? *reinterpret_cast<const f32x4*>(p.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }

    // per-batch row vector (time embedding): one row serves the whole tile whenever the tile does not straddle two batch
    // elements -> prefetch it as well
    constexpr bool RV_PRE = !SPLIT && !GEGLU && TN <= 4 && !PP8;
    f32x4 rvpre[TN];
    bool rv_pre_ok = false;
    if constexpr (RV_PRE) {
        if (p.rowvec) {
            const int rb0 = m0 / p.rows_per_batch;
            rv_pre_ok = ((min(m0 + BM, p.M) - 1) / p.rows_per_batch) == rb0;
            if (rv_pre_ok) {
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n = n0 + wn * WTN + j * 16 + (lane >> 4) * 4;
                    rvpre[j] = n < p.N ? *reinterpret_cast<const f32x4*>(p.rowvec + (int64_t)rb0 * p.rowvec_ld + n)
                                       : f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
        }
    }

    const int nk_all = p.K / BK;
    const int kt0 = SPLIT ? (int)((int64_t)nk_all * blockIdx.z / p.splits) : 0;
    const int nk = SPLIT ? (int)((int64_t)nk_all * (blockIdx.z + 1) / p.splits) : nk_all;
    const int frow = lane & 15;        // operand row inside a 16-row fragment
    const int fq = lane >> 4;          // 16-byte chunk inside a 32-wide k-step

    // all fragment reads of the K tile (both 32-wide k-steps) are issued before the first MFMA: one exposed LDS latency
    // per tile instead of one per k-step (with 1-2 waves per SIMD nothing else hides it); the compiler's counted
    // lgkmcnt waits let the first MFMAs start as soon as the k-step-0 fragments are back.
    auto compute_tile = [&](int buf) {
        const bf16* as = smem_b + buf * STAGE + (wm * WTM) * BK;
        const bf16* bs = smem_b + buf * STAGE + BM * BK + (wn * WTN) * BK;
        bf16x8 af[2][TM], wf[2][TN];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int sw = (((ks * 4 + fq) ^ (frow & 7)) * 8);
#pragma unroll
            for (int j = 0; j < TN; ++j) wf[ks][j] = *reinterpret_cast<const bf16x8*>(bs + (j * 16 + frow) * BK + sw);
#pragma unroll
            for (int i = 0; i < TM; ++i) af[ks][i] = *reinterpret_cast<const bf16x8*>(as + (i * 16 + frow) * BK + sw);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = mma16<F16>(wf[ks][j], af[ks][i], acc[i][j]);
    };

    if constexpr (PP8) {
        // ---- 256 x 256 x 64 tile, 8 waves as 2 (M) x 4 (N), 128 x 64 wave tiles: the 8-phase ping-pong loop of the CDNA guide's
        // "256^2 8-phase template" (cdna_hip_programming.md), built from its description.  Why: a 128 x 128 tile needs 1 byte of
        // LDS fill per 64 FLOP and the fill path gives a CU ~50-70 GB/s (profiles/r02_lab_fill.log) -> at most ~1.1 PF; 256 x 256
        // halves the bytes per FLOP, but a block-wide "all read, all multiply" loop leaves LDS and matrix pipe idle in turn
        // (0.5-0.8 PF, profiles/r02_lab_gemm_t256.log).  Here:
        //   * a K tile is four 16 KB HALF tiles  h0 = A rows of quadrant-row 0, h1 = W columns of quadrant-column 1,
        //     h2 = A rows of quadrant-row 1, h3 = W columns of quadrant-column 0  (quadrant-row r of the block = rows
        //     wm * 128 + r * 64 + [0, 64) of both wave rows; quadrant-column c = columns wn * 64 + c * 32 + [0, 32));
        //   * a K tile is four PHASES, one 64 x 32 quadrant of the wave tile each (16 MFMAs over K = 64):
        //       q0 = (r0, c0) reads h0, h3 | q1 = (r0, c1) reads h1 | q2 = (r1, c1) reads h2 | q3 = (r1, c0) reads h3
        //     so every half tile has its LAST read one phase before the phase that restages it (tile u + 2 into the same buffer):
        //       q1 stages h0, q2 stages h1, q3 stages h2, q0 of the next tile stages h3  -> 3-4 half tiles always in flight;
        //   * every phase is  [fragment reads + 2 LDS-DMA + lgkmcnt(0)]  s_barrier  [16 MFMAs]  s_barrier,  and wave row 1 runs
        //     ONE BARRIER behind wave row 0: while one wave of a SIMD multiplies, the other reads and stages;
        //   * one counted wait per K tile (q3): vmcnt(6) leaves the three youngest half tiles in flight, never 0 in the loop.
        // Ordering (guide, "Read a staged buffer one phase AFTER the wait that retires it"): the q3 wait sits before q3's first
        // barrier and the first read of the tile it retires is in q0; fragment reads are retired (lgkmcnt(0)) BEFORE the phase's
        // first barrier, which is what makes restaging one phase later safe with the two wave rows a barrier apart.
        static_assert(NS == 2 && A_CH == 4 && B_CH == 4, "two 64 KB buffers of four half tiles");
        constexpr int HALF = 128 * BK;                               // elements per half tile
        const int T = nk - kt0;
        const int schunk = ((tid & 7) ^ ((tid >> 3) & 7)) * 8;
        // LDS: [buffer][h0 = A r0 | h2 = A r1 | h3 = W c0 | h1 = W c1], 16 KB each
        auto half_base = [&](int u, int h) { return smem_b + ((u & 1) * 4 + (h == 0 ? 0 : h == 2 ? 1 : h == 3 ? 2 : 3)) * HALF; };
        auto stage_half = [&](int u, int h) {                         // this wave's 2 x 1 KB of half tile h of K tile u
            if (u >= T) return;
            const int kbase = (kt0 + u) * BK;
            bf16* dst = half_base(u, h) + (16 * wave) * BK;
            if (h == 0 || h == 2) {
                const int c0 = h == 0 ? 0 : 2;
                if constexpr (CONV) {
                    const int tap = kbase / p.Cin;
                    const int ci0 = kbase - tap * p.Cin;
                    const int ksz = p.upsample == 2 ? 2 : 3;
                    const int ky = tap / ksz, kx = tap - ky * ksz;
                    const int Hs = p.upsample == 1 ? p.Hin * 2 : p.Hin;
                    const int Ws = p.upsample == 1 ? p.Win * 2 : p.Win;
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int iy = a_oy[c0 + i] + ky, ix = a_ox[c0 + i] + kx;
                        const bool ok = (iy >= 0) & (iy < Hs) & (ix >= 0) & (ix < Ws);
                        const int sy = p.upsample == 1 ? (iy >> 1) : iy;
                        const int sx = p.upsample == 1 ? (ix >> 1) : ix;
                        const bf16* src = ok ? (A + a_off[c0 + i] + ((int64_t)sy * p.Win + sx) * p.Cin + ci0 + schunk)
                                             : reinterpret_cast<const bf16*>(seer_zero_page);
                        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                         (__attribute__((address_space(3))) void*)(dst + 8 * i * BK), 16, 0, 0);
                    }
                } else {
                    const bool second = kbase >= p.K1;
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const bf16* src = second ? (A2 + a_off2[c0 + i] + (kbase - p.K1) + schunk) : (A + a_off[c0 + i] + kbase + schunk);
                        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                         (__attribute__((address_space(3))) void*)(dst + 8 * i * BK), 16, 0, 0);
                    }
                }
            } else {
                const int c0 = h == 3 ? 0 : 2;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const bf16* src = W + b_off[c0 + i] + kbase + schunk;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                     (__attribute__((address_space(3))) void*)(dst + 8 * i * BK), 16, 0, 0);
                }
            }
        };
        bf16x8 fa[2][4], fb[2][2];
        auto read_a = [&](int u, int r) {                             // 64 rows of this wave x K 64: 8 ds_read_b128
            const bf16* as = half_base(u, r == 0 ? 0 : 2) + (wm * 64) * BK;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int sw = (((ks * 4 + fq) ^ (frow & 7)) * 8);
#pragma unroll
                for (int i = 0; i < 4; ++i) fa[ks][i] = *reinterpret_cast<const bf16x8*>(as + (i * 16 + frow) * BK + sw);
            }
        };
        auto read_b = [&](int u, int c) {                             // 32 columns of this wave x K 64: 4 ds_read_b128
            const bf16* bs = half_base(u, c == 0 ? 3 : 1) + (wn * 32) * BK;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int sw = (((ks * 4 + fq) ^ (frow & 7)) * 8);
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[ks][j] = *reinterpret_cast<const bf16x8*>(bs + (j * 16 + frow) * BK + sw);
            }
        };
        auto barrier = [&]() {
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_barrier" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
        };
        // the MFMA half of a phase: quadrant (r, c) of the wave tile, between the phase's two barriers
#define SEER_PP8_MMA(R, C)                                                                                                   \
        do {                                                                                                                 \
            barrier();                                                                                                       \
            __builtin_amdgcn_s_setprio(1);                                                                                   \
            _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                                 \
                _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                \
                    _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                            \
                        acc[4 * (R) + i][2 * (C) + j] =                                                                      \
                            mma16<F16>(fb[ks][j], fa[ks][i], acc[4 * (R) + i][2 * (C) + j]);                                                \
            __builtin_amdgcn_s_setprio(0);                                                                                   \
            barrier();                                                                                                       \
        } while (0)

        PSTAMP();
        // prologue: K tile 0 whole, K tile 1 up to h2 (its h3 goes out in q0 of tile 0)
        stage_half(0, 0); stage_half(0, 1); stage_half(0, 2); stage_half(0, 3);
        stage_half(1, 0); stage_half(1, 1); stage_half(1, 2);
        if (T > 1) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        barrier();
        PSTAMP();
        if (wm == 1) barrier();                                       // wave row 1 runs one barrier behind from here on
        for (int u = 0; u < T; ++u) {
            // q0
            read_b(u, 0);
            read_a(u, 0);
            stage_half(u + 1, 3);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            SEER_PP8_MMA(0, 0);
            // q1
            read_b(u, 1);
            stage_half(u + 2, 0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            SEER_PP8_MMA(0, 1);
            // q2
            read_a(u, 1);
            stage_half(u + 2, 1);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            SEER_PP8_MMA(1, 1);
            // q3: the wait that retires K tile u + 1 (all but the halves h0..h2 of tile u + 2 staged in q1..q3)
            read_b(u, 0);
            stage_half(u + 2, 2);
            if (u + 2 < T) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            SEER_PP8_MMA(1, 0);
        }
#undef SEER_PP8_MMA
        PSTAMP();
        if (wm == 0) barrier();                                       // re-align the two wave rows
        PSTAMP();
    } else if constexpr (NS == 0) {
        load_tile(kt0);
        store_tile(0);
        __syncthreads();
        for (int kt = kt0; kt < nk; ++kt) {
            const int buf = (kt - kt0) & 1;
            if (kt + 1 < nk) load_tile(kt + 1);
            compute_tile(buf);
            if (kt + 1 < nk) store_tile(buf ^ 1);
            __syncthreads();
        }
    } else {
        // ---- LDS-direct ring.  One wave instruction writes 1 KiB = 8 rows x 128 B, lane l -> (row l>>3, slot l&7); the
        // XOR swizzle goes on the SOURCE chunk (slot ^ row&7), the LDS image stays lane-linear (cdna guide, rule 21).
        constexpr int LPT = A_CH + B_CH;           // global_load_lds per wave per K tile
        const int schunk = ((tid & 7) ^ (srow & 7)) * 8;
        // plain operands as buffer loads: wave-uniform resource at the tile's first row, per-lane byte offset that is constant
        // over K (hoisted here), scalar offset that advances with K -- per piece one M0 write and one buffer_load ... lds.
        // (The offset arguments are cast to int explicitly: without the casts hipcc (ROCm 7.2) silently drops the HOST stub of every
        //  instantiation that reaches this call -- no diagnostic, undefined __device_stub__ symbols at load time.)
        unsigned av1[A_CH], av2[A_CH], bv[B_CH];
        if constexpr (!CONV) {
#pragma unroll
            for (int i = 0; i < A_CH; ++i) {
                av1[i] = (unsigned)(a_oy[i] + schunk) * 2u;
                av2[i] = (unsigned)(a_ox[i] + schunk) * 2u;
            }
        }
#pragma unroll
        for (int i = 0; i < B_CH; ++i) bv[i] = (unsigned)(b_rel[i] + schunk) * 2u;

        auto issue_tile = [&](int kt, int stage) {
            const int kbase = kt * BK;
            bf16* as = smem_b + stage * STAGE + (8 * wave) * BK;      // this wave's 8-row group (wave-uniform)
            bf16* bs = smem_b + stage * STAGE + BM * BK + (8 * wave) * BK;
            if constexpr (CONV) {
                if (conv_fast) {
                    const int tap = (int)__umulhi((unsigned)kbase, cin_magic);
                    const int ci0 = kbase - tap * p.Cin;
                    const int ksz = p.upsample == 2 ? 2 : 3;
                    const int ky = tap / ksz, kx = tap - ky * ksz;
                    const int tap_b = (ky * p.Win + kx) * p.Cin * 2;
#pragma unroll
                    for (int i = 0; i < A_CH; ++i) {
                        const bool ok = ((a_okb[i / 3] >> (9 * (i % 3) + tap)) & 1u) != 0u;
                        const unsigned voff = ok ? (unsigned)(a_pix[i] + tap_b) : a_bytes;
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, (__attribute__((address_space(3))) void*)(as + RPP * i * BK), 16, voff,
                                                                 ci0 * 2, 0, 0);
                    }
                } else {
                const int tap = kbase / p.Cin;
                const int ci0 = kbase - tap * p.Cin;
                const int ksz = p.upsample == 2 ? 2 : 3;
                const int ky = tap / ksz, kx = tap - ky * ksz;
                const int Hs = p.upsample == 1 ? p.Hin * 2 : p.Hin;
                const int Ws = p.upsample == 1 ? p.Win * 2 : p.Win;
#pragma unroll
                for (int i = 0; i < A_CH; ++i) {
                    const int iy = a_oy[i] + ky, ix = a_ox[i] + kx;
                    const bool ok = (iy >= 0) & (iy < Hs) & (ix >= 0) & (ix < Ws);
                    const int sy = p.upsample == 1 ? (iy >> 1) : iy;
                    const int sx = p.upsample == 1 ? (ix >> 1) : ix;
                    const bf16* src = ok ? (A + a_off[i] + ((int64_t)sy * p.Win + sx) * p.Cin + ci0 + schunk)
                                         : reinterpret_cast<const bf16*>(seer_zero_page);
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                     (__attribute__((address_space(3))) void*)(as + RPP * i * BK), 16, 0, 0);
                }
                }
            } else {
                if (kbase >= p.K1) {               // (wave-uniform: the second source of a skip concat)
#pragma unroll
                    for (int i = 0; i < A_CH; ++i)
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(r_a2, (__attribute__((address_space(3))) void*)(as + RPP * i * BK), 16, (int)av2[i],
                                                                 (int)((kbase - p.K1) * 2), 0, 0);
                } else {
#pragma unroll
                    for (int i = 0; i < A_CH; ++i)
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(r_a1, (__attribute__((address_space(3))) void*)(as + RPP * i * BK), 16, (int)av1[i],
                                                                 (int)(kbase * 2), 0, 0);
                }
            }
#pragma unroll
            for (int i = 0; i < B_CH; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(r_w, (__attribute__((address_space(3))) void*)(bs + RPP * i * BK), 16, (int)bv[i], (int)(kbase * 2), 0, 0);
        };
        // Early refill: a stage is only occupied from "landed" to "fragments in registers".  Per K tile: wait for the tile,
        // barrier, read ALL its fragments (both k-steps) into VGPRs, barrier, refill the SAME stage with tile kt+NS, then run
        // the MFMAs from registers -> NS tiles (not NS-1) are in flight while the MFMAs of a tile run, at the same LDS bytes.
        bf16x8 af[2][TM], wf[2][TN];
        auto read_frags = [&](int buf) {
            const bf16* as = smem_b + buf * STAGE + (wm * WTM) * BK;
            const bf16* bs = smem_b + buf * STAGE + BM * BK + (wn * WTN) * BK;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int sw = (((ks * 4 + fq) ^ (frow & 7)) * 8);
#pragma unroll
                for (int j = 0; j < TN; ++j) wf[ks][j] = *reinterpret_cast<const bf16x8*>(bs + (j * 16 + frow) * BK + sw);
#pragma unroll
                for (int i = 0; i < TM; ++i) af[ks][i] = *reinterpret_cast<const bf16x8*>(as + (i * 16 + frow) * BK + sw);
            }
        };
#if SEER_GEMM_PROBE & 8
        // probe build: the same operand registers through 32x32x16 MFMAs (half the MFMA issues for the same pipe time; the numbers
        // are meaningless) -- prices what a 32x32 fragment layout could buy before anyone writes it
        constexpr bool P32 = (TM % 2 == 0) && (TN % 2 == 0) && !F16;
        f32x16 acc32[P32 ? TM / 2 : 1][P32 ? TN / 2 : 1] = {};
#endif
        auto mma_tile = [&]() {
#if SEER_GEMM_PROBE & 8
            if constexpr (P32) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int i = 0; i < TM / 2; ++i)
#pragma unroll
                            for (int j = 0; j < TN / 2; ++j)
                                acc32[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[ks][2 * j + h], af[ks][2 * i + h], acc32[i][j], 0, 0, 0);
                return;
            }
#endif
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = mma16<F16>(wf[ks][j], af[ks][i], acc[i][j]);
        };
        {
        PSTAMP();
#pragma unroll
        for (int s_ = 0; s_ < NS; ++s_)
            if (kt0 + s_ < nk) issue_tile(kt0 + s_, s_);
#if SEER_GEMM_PROBE & 2
        read_frags(0);
#endif
        int stage = 0;
        for (int kt = kt0; kt < nk; ++kt) {
            const int pending = min(NS - 1, nk - 1 - kt);   // tiles issued after tile kt
            if (NS >= 4 && pending >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * LPT) : "memory");
            else if (NS >= 3 && pending == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPT) : "memory");
            else if (pending == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LPT) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("s_barrier" ::: "memory");            // every wave's part of tile kt has landed
#ifdef SEER_GEMM_STAMPS
            if (kt == kt0) PSTAMP();
#endif
#if !(SEER_GEMM_PROBE & 2)
            read_frags(stage);
#endif
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            asm volatile("s_barrier" ::: "memory");            // every wave holds its fragments: the stage is free
#if !(SEER_GEMM_PROBE & 1)
            if (kt + NS < nk) issue_tile(kt + NS, stage);
#endif
#if !(SEER_GEMM_PROBE & 4)
            mma_tile();
#else
            // probe build (scripts/probe_gemm.sh): keep the fragment reads alive without issuing MFMAs
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
                for (int j = 0; j < TN; ++j) asm volatile("" ::"v"(wf[ks][j]));
#pragma unroll
                for (int i = 0; i < TM; ++i) asm volatile("" ::"v"(af[ks][i]));
            }
#endif
            stage = (stage + 1 == NS) ? 0 : stage + 1;
        }
        PSTAMP();
#if SEER_GEMM_PROBE & 8
        if constexpr (P32) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[i][j][e] = acc32[i / 2][j / 2][((i & 1) * 2 + (j & 1)) * 4 + e];
        }
#endif
        }
        // (measured and rejected on MI355X, profiles/r01_gemm_microbench_v5.log: issuing the LDS-DMA pieces between the MFMAs
        //  with sched_group_barrier instead of in one burst is 5-20 % SLOWER at 2 blocks/CU: the other block already covers
        //  the burst, and spreading the pieces delays the next tile's arrival at the barrier.)
    }

#ifdef SEER_GEMM_EPI_NOP
    // bug-hunt build (scripts/exp_flake.py): a long pause between the last MFMA of the K loop and the first read of an accumulator
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
#endif
    // ---- split-K: raw fp32 partial tile to the workspace slice of this K range; the reduce kernel does the epilogue
    if constexpr (SPLIT) {
        float* ws = reinterpret_cast<float*>(p.workspace) + (int64_t)blockIdx.z * p.M * p.N;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m0 + wm * WTM + i * 16 + frow;
            if (m >= p.M) continue;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn * WTN + j * 16 + fq * 4;
                if (n >= p.N) continue;
                // write-through: up to 31 MB of partials per launch would otherwise sit dirty in L2 until the boundary in front
                // of the reduce pass
                store16_out(ws + (int64_t)m * p.N + n, __builtin_bit_cast(u32x4, acc[i][j]));
            }
        }
        PSTAMP();
        PSPAN(1);
        return;
    }

    // ---- epilogue: lane holds rows n = 4*fq + r (r = 0..3) of the 16x16 D tile, column m = frow
    const bool out_f32 = (p.epilogue & SEER_EPI_OUT_F32) != 0;
    const bool do_silu = (p.epilogue & SEER_EPI_SILU) != 0;
    const bool do_qgelu = (p.epilogue & SEER_EPI_QUICKGELU) != 0;
    const bool trans = (p.epilogue & SEER_EPI_TRANS_OUT) != 0;
    bf16* Cb = reinterpret_cast<bf16*>(p.C) + (int64_t)z * p.strideC;
    // output row of GEMM row m: the identity, except for the phase convs, whose row (img, y, x) is pixel (2 y + a, 2 x + b)
    auto crow = [&](int m) -> int64_t {
        if constexpr (CONV) {
            if (p.upsample == 2) {
                const int hw = p.Hin * p.Win;
                const int img = m / hw, rem = m - img * hw;
                const int y = rem / p.Win, x = rem - y * p.Win;
                return ((int64_t)img * p.Hout + 2 * y + ((int)blockIdx.z >> 1)) * p.Wout + 2 * x + ((int)blockIdx.z & 1);
            }
        }
        return m;
    };
    float* Cf = reinterpret_cast<float*>(p.C) + (int64_t)z * p.strideC;
    const bool do_rot = (p.epilogue & SEER_EPI_ROTARY) != 0;

    // bf16 row-major outputs leave through LDS: the MFMA layout gives a lane 8 B in each of 16 different rows (32-B row
    // segments per wave instruction, measured ~1.5 TB/s); staged through the (now idle) K-loop LDS the block stores 16 B per
    // lane along whole output rows instead.
    constexpr int BNO = TS::bno(GEGLU);                 // output columns of the block tile
    constexpr bool CSWZ = TS::cswz(GEGLU);              // staged rows: dense and chunk-swizzled, or padded (TileShape)
    constexpr int CPITCH = TS::cpitch(GEGLU);           // staged row pitch in bytes
    static_assert(BM * CPITCH <= 2 * STAGE * (int)sizeof(bf16), "staged C tile must fit in the K-loop LDS");
    const bool staged = !out_f32 && !trans && (p.ldc % 8 == 0) && (p.N % (GEGLU ? 16 : 8) == 0) &&
                        ((reinterpret_cast<uintptr_t>(Cb) & 15) == 0);
    if (staged) __syncthreads();                        // every wave is done with the K-loop stages
    // folded LayerNorm: acc <- rstd * acc - (mean * rstd) * wsum[n], first term of the epilogue (the host admits it only for
    // staged launches: the row statistics travel through the idle K-loop LDS)
    constexpr int LNROW_OFF = TS::lnrow_off(GEGLU);
    bool do_ln = false;
    float lmr[TM], lr[TM];
    if constexpr (LN_OK) {
        do_ln = p.ln_rowstat != nullptr && staged;
        if (do_ln) {
            float* lnrow = reinterpret_cast<float*>(smem + LNROW_OFF);
            if (tid < BM) {
                // E[x^2] - mean^2 in DOUBLE on the exact integer totals: a row whose mean is 100 standard deviations away keeps
                // its variance (in fp32 the difference of the two ~1e4-times-larger terms loses it); BM threads, once per tile
                const double k = 1.0 / ((double)(1 << SEER_LN_FX_SHIFT) * (double)p.K);
                const double mean = (double)ln_raw[0] * k;
                double var = (double)ln_raw[1] * k - mean * mean;
                var = var > 0.0 ? var : 0.0;
                const float r = (float)(1.0 / __builtin_sqrt(var + (double)p.ln_eps));
                *reinterpret_cast<f32x2*>(lnrow + tid * 2) = f32x2{(float)mean * r, r};
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const f32x2 v = *reinterpret_cast<const f32x2*>(lnrow + (wm * WTM + i * 16 + frow) * 2);
                lmr[i] = v[0];
                lr[i] = v[1];
            }
        }
    }

    // ---- fast epilogue: a full tile whose epilogue is bias / GEGLU / preloaded row vector / rotary / column scale / preloaded
    // residual into the staged C tile (every FF, projection, q|k|v and conv GEMM of the U-Net).  The general body below tests each descriptor flag for each of the
    // TM x TN accumulator quads and recomputes the staging address per quad: ~30 VALU instructions per quad, 3.2 us of VALU
    // issue per 256x256 tile and 1.6 us per 128x128 tile (profiles/r02_pp8_stamps.log).  Here every term is its own pass over
    // the accumulators behind ONE wave-uniform branch, in the general body's order of additions, and the staging address is one
    // XOR per fragment column plus an immediate offset per fragment row.  The two bodies are NOT bit-identical in every class: the
    // folded LayerNorm's term in front of a GEGLU differed in its last bits on MI355X (below; probably an fma contracted in one
    // body and not in the other).  Follow-up: make ln_term contract alike in both, then the layout-invariant request can take
    // this body again and stop paying the general body's VALU time on every tile.
    // row statistics of the output (seer_gemm_desc::rowstat): each lane adds the fp32 values of its quads per fragment row, the
    // four lanes of a row meet by two lane exchanges, one atomic pair per (row, wave column)
    constexpr bool RS_OK = !GEGLU && !SPLIT && TS::ln_ok;
    bool do_rs = false;
    float rsum[TM], rsq[TM];
    if constexpr (RS_OK) {
        do_rs = p.rowstat != nullptr;
#pragma unroll
        for (int i = 0; i < TM; ++i) { rsum[i] = 0.f; rsq[i] = 0.f; }
    }
    // (the layout-invariant request keeps EVERY tile on the general body: a row must not get other bits for sitting in a full tile in
    //  one launch and in the ragged last tile of another -- measured on MI355X: the GEGLU projection with the folded LayerNorm, 192 rows
    //  against 384, differed in its last bits between the two bodies)
    const bool fast_epi = staged && m0 + BM <= p.M && n0 + BN <= p.N && !do_silu && !do_qgelu && p.tile != SEER_TILE_AUTO_INVARIANT &&
                          (!GEGLU || !(do_rot || (p.epilogue & SEER_EPI_COLSCALE))) && (!p.rowvec || (RV_PRE && rv_pre_ok)) &&
                          (!R || RES_PRE);          // a residual that was not prefetched takes the general body
    if (fast_epi) {
        if constexpr (LN_OK) {
            if (do_ln) {
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const f32x4 sv = spre[j];
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[i][j][r] = ln_term(acc[i][j][r], lr[i], sv[r], lmr[i]);
                }
            }
        }
        if (p.bias) {
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                f32x4 bv;
                if constexpr (BIAS_PRE) bv = bpre[j];
                else bv = *reinterpret_cast<const f32x4*>(p.bias + n0 + wn * WTN + j * 16 + fq * 4);
#pragma unroll
                for (int i = 0; i < TM; ++i) acc[i][j] += bv;
            }
        }
        if constexpr (GEGLU) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int j = 0; j < TN; j += 2) {
                    const f32x4 g = acc[i][j + 1];
                    const f32x2 ge0 = gelu_erf_f2(f32x2{g[0], g[1]}), ge1 = gelu_erf_f2(f32x2{g[2], g[3]});
                    acc[i][j][0] *= ge0[0]; acc[i][j][1] *= ge0[1]; acc[i][j][2] *= ge1[0]; acc[i][j][3] *= ge1[1];
                }
                if constexpr (PP8) __builtin_amdgcn_sched_barrier(0);    // one fragment row of erf temporaries at a time
            }
        }
        if constexpr (RV_PRE) {
            if (p.rowvec) {
#pragma unroll
                for (int j = 0; j < TN; ++j) {
#pragma unroll
                    for (int i = 0; i < TM; ++i) acc[i][j] += rvpre[j];
                }
            }
        }
        if constexpr (!GEGLU) {
            if (do_rot && n0 + wn * WTN < p.rot_cols) {      // (wave-uniform: a wave whose columns are all v columns has nothing to rotate)
                // rotary on the q|k columns (attention.py:649-651), as in the general body, with the channel of each fragment
                // column and the position of each fragment row computed once per lane instead of once per quad.
                // (Measured and dropped, profiles/r03_rotary_loads.log: unconditional (cos, sin) loads issued together per fragment
                //  row, the unrotated quads kept by a select -- 33.5 vs 32.2 us on the 24 576-row projection: the cost of the
                //  epilogue is the 63 MB of table reads per launch, not their latency.)
                int tj[TN];                                 // float offset of the lane's (cos, sin) pairs in a table row, or -1
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n = n0 + wn * WTN + j * 16 + fq * 4;
                    const int ch = n % p.rot_head_dim;
                    tj[j] = (n < p.rot_cols && ch < p.rot_dim) ? (ch / 2) * 2 : -1;
                }
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int m = m0 + wm * WTM + i * 16 + frow;
                    const int pos = m % p.rot_tokens_per_batch + p.rot_pos_offset;
                    const float* trow = p.rot_table + (int64_t)pos * (p.rot_dim / 2) * 2;
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        if (tj[j] >= 0) {
                            const f32x4 cs = *reinterpret_cast<const f32x4*>(trow + tj[j]);
                            const f32x2 r01 = rot_pair(f32x2{acc[i][j][0], acc[i][j][1]}, cs[0], cs[1]);
                            const f32x2 r23 = rot_pair(f32x2{acc[i][j][2], acc[i][j][3]}, cs[2], cs[3]);
                            acc[i][j] = f32x4{r01[0], r01[1], r23[0], r23[1]};
                        }
                    }
                }
            }
            if (p.epilogue & SEER_EPI_COLSCALE) {
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    // x * 1.0f is exact: the columns past col_scale_cols keep their bits
                    const float sc = (n0 + wn * WTN + j * 16 + fq * 4) < p.col_scale_cols ? p.col_scale : 1.f;
#pragma unroll
                    for (int i = 0; i < TM; ++i) acc[i][j] *= sc;
                }
            }
        }
        if constexpr (RES_PRE) {
            if (R) {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const u32x2 rv = rpre[i][j];
                        const f32x2 r01 = unpack2t<F16>(rv[0]), r23 = unpack2t<F16>(rv[1]);
                        acc[i][j][0] += r01[0];
                        acc[i][j][1] += r01[1];
                        acc[i][j][2] += r23[0];
                        acc[i][j][3] += r23[1];
                    }
                }
            }
        }
        if constexpr (RS_OK) {
            if (do_rs) {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    float sm = 0.f, sq = 0.f;
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) { sm += acc[i][j][r]; sq = fmaf(acc[i][j][r], acc[i][j][r], sq); }
                    rsum[i] = sm;
                    rsq[i] = sq;
                }
            }
        }
        // byte column of the lane's quad inside the staged row: GEGLU halves the column pitch (value columns only)
        const int cb0 = GEGLU ? (wn * WTN + fq * 8) : (wn * WTN * 2 + fq * 8);
        const int rowb = (wm * WTM + frow) * CPITCH;
#pragma unroll
        for (int j = 0; j < TN; j += (GEGLU ? 2 : 1)) {
            const int cb = cb0 + (GEGLU ? j * 16 : j * 32);
            const int at = rowb + (CSWZ ? (cb ^ (frow << 4)) : cb);
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                u32x2 o;
                o[0] = pack2t<F16>(acc[i][j][0], acc[i][j][1]);
                o[1] = pack2t<F16>(acc[i][j][2], acc[i][j][3]);
                *reinterpret_cast<u32x2*>(smem + at + i * 16 * CPITCH) = o;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m0 + wm * WTM + i * 16 + frow;
            if (m >= p.M) continue;
            const int rb = p.rowvec ? (m / p.rows_per_batch) : 0;
#pragma unroll
            for (int j = 0; j < TN; j += (GEGLU ? 2 : 1)) {
                const int n = n0 + wn * WTN + j * 16 + fq * 4;   // first of 4 consecutive GEMM columns
                if (n >= p.N) continue;
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r];
                if constexpr (LN_OK) {
                    if (do_ln) {
                        const f32x4 sv = spre[j];
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = ln_term(v[r], lr[i], sv[r], lmr[i]);
                    }
                }
                if (p.bias) {
                    f32x4 bv;
                    if constexpr (BIAS_PRE) bv = bpre[j];
                    else bv = *reinterpret_cast<const f32x4*>(p.bias + n);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] += bv[r];
                }
                int nc = n;   // output column
                if constexpr (GEGLU) {
                    float g[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) g[r] = acc[i][j + 1][r];
                    if constexpr (LN_OK) {
                        if (do_ln) {
                            const f32x4 sv = spre[j + 1];
#pragma unroll
                            for (int r = 0; r < 4; ++r) g[r] = ln_term(g[r], lr[i], sv[r], lmr[i]);
                        }
                    }
                    if (p.bias) {
                        f32x4 bg;
                        if constexpr (BIAS_PRE) bg = bpre[j + 1];
                        else bg = *reinterpret_cast<const f32x4*>(p.bias + n + 16);
#pragma unroll
                        for (int r = 0; r < 4; ++r) g[r] += bg[r];
                    }
                    const f32x2 ge0 = gelu_erf_f2(f32x2{g[0], g[1]}), ge1 = gelu_erf_f2(f32x2{g[2], g[3]});
                    v[0] *= ge0[0]; v[1] *= ge0[1]; v[2] *= ge1[0]; v[3] *= ge1[1];
                    nc = ((n - fq * 4) >> 1) + fq * 4;
                }
                if (p.rowvec) {
                    f32x4 tv;
                    if (RV_PRE && rv_pre_ok) tv = rvpre[j];
                    else tv = *reinterpret_cast<const f32x4*>(p.rowvec + (int64_t)rb * p.rowvec_ld + nc);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] += tv[r];
                }
                if (do_silu) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = silu_f(v[r]);
                }
                if (do_qgelu) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = quick_gelu_f(v[r]);
                }
                if (do_rot && n < p.rot_cols) {
                    // rotary on q|k columns (attention.py:649-651): channel inside its head = n % head_dim; the lane's 4
                    // consecutive columns are two interleaved pairs (x0,x1) -> (x0 c - x1 s, x1 c + x0 s)
                    const int ch = n % p.rot_head_dim;
                    if (ch < p.rot_dim) {
                        const int pos = m % p.rot_tokens_per_batch + p.rot_pos_offset;
                        const f32x4 cs = *reinterpret_cast<const f32x4*>(p.rot_table + ((int64_t)pos * (p.rot_dim / 2) + ch / 2) * 2);
                        const f32x2 r01 = rot_pair(f32x2{v[0], v[1]}, cs[0], cs[1]);
                        const f32x2 r23 = rot_pair(f32x2{v[2], v[3]}, cs[2], cs[3]);
                        v[0] = r01[0]; v[1] = r01[1]; v[2] = r23[0]; v[3] = r23[1];
                    }
                }
                if ((p.epilogue & SEER_EPI_COLSCALE) && n < p.col_scale_cols) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] *= p.col_scale;
                }
                if (R) {
                    u32x2 rv;
                    if constexpr (RES_PRE) rv = rpre[i][j];
                    else rv = *reinterpret_cast<const u32x2*>(R + (int64_t)m * p.ldr + nc);
                    const f32x2 r01 = unpack2t<F16>(rv[0]), r23 = unpack2t<F16>(rv[1]);
                    v[0] += r01[0];
                    v[1] += r01[1];
                    v[2] += r23[0];
                    v[3] += r23[1];
                }
                if constexpr (RS_OK) {
                    if (do_rs) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) { rsum[i] += v[r]; rsq[i] = fmaf(v[r], v[r], rsq[i]); }
                    }
                }
                if (trans) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (out_f32) Cf[(int64_t)(nc + r) * p.ldc + m] = v[r];
                        else if constexpr (F16) reinterpret_cast<_Float16*>(Cb)[(int64_t)(nc + r) * p.ldc + m] = (_Float16)v[r];
                        else Cb[(int64_t)(nc + r) * p.ldc + m] = (bf16)v[r];
                    }
                } else if (out_f32) {
                    *reinterpret_cast<f32x4*>(Cf + (int64_t)m * p.ldc + nc) = f32x4{v[0], v[1], v[2], v[3]};
                } else {
                    u32x2 o;
                    o[0] = pack2t<F16>(v[0], v[1]);
                    o[1] = pack2t<F16>(v[2], v[3]);
                    if (staged) {
                        const int row_l = wm * WTM + i * 16 + frow;
                        const int col_l = nc - (GEGLU ? (n0 >> 1) : n0);
                        const int cb = col_l * 2;
                        *reinterpret_cast<u32x2*>(smem + row_l * CPITCH + (CSWZ ? (cb ^ ((row_l & 15) << 4)) : cb)) = o;
                    } else {
                        *reinterpret_cast<u32x2*>(Cb + crow(m) * p.ldc + nc) = o;
                    }
                }
            }
        }
    }   // general epilogue
    if constexpr (RS_OK) {
        if (do_rs) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                float sm = rsum[i], sq = rsq[i];
                sm += __shfl_xor(sm, 16); sq += __shfl_xor(sq, 16);
                sm += __shfl_xor(sm, 32); sq += __shfl_xor(sq, 32);
                // ONE instruction for both: lanes fq = 0 add the sums, lanes fq = 1 the squares of the same 16 rows -- 256 contiguous
                // bytes = four fully used 64-byte atomic requests (the requests are the cost: ~12 ns each per CU)
                const int m = m0 + wm * WTM + i * 16 + frow;
                if (fq < 2 && m < p.M) fx_add_ln(p.rowstat + (int64_t)m * 2 + fq, fq ? sq : sm);
            }
        }
    }
    PSTAMP();
    if (staged) {
        __syncthreads();
        PSTAMP();
        constexpr int CPR = BNO / 8;                    // 16-byte chunks per staged row
        const bool wt_store = p.K <= 3072;
        const int n0o = GEGLU ? (n0 >> 1) : n0;
        const int n_out = GEGLU ? (p.N >> 1) : p.N;
        // ---- column sums of the tile as stored (bf16-rounded): sum and sum of squares per output column over the tile's rows,
        // written to colsum[z][tile_m][N][2].  The GroupNorm that consumes C adds them per (batch element, group) in a fixed
        // order (seer_groupnorm_stats_from_colsums) instead of re-reading C.  Thread -> (column pair, row segment): a wave reads
        // 256 contiguous bytes of one staged row per instruction (conflict-free), row segments are added in order by the
        // column's thread: deterministic, no atomics.
        constexpr int CS_CP = BNO / 2;                  // column pairs
        constexpr int CS_RS = NT / CS_CP;               // row segments
        constexpr bool COLSUM_OK = !GEGLU && !SPLIT && TS::colsum_ok;
        float* cs_scratch = reinterpret_cast<float*>(smem + BM * CPITCH);
        if constexpr (COLSUM_OK) {
            if (p.colsum || p.colsum_fx) {
                const int cp = tid % CS_CP, rs = tid / CS_CP;
                if (rs < CS_RS) {
                    const int rows = min(BM, p.M - m0);
                    const int chunk = cp >> 2, within = (cp & 3) * 4;
                    float s0 = 0.f, q0 = 0.f, s1 = 0.f, q1 = 0.f;
                    for (int r = rs; r < rows; r += CS_RS) {
                        const uint32_t v = *reinterpret_cast<const uint32_t*>(
                            smem + r * CPITCH + (CSWZ ? (chunk ^ (r & 15)) : chunk) * 16 + within);
                        const f32x2 f01 = unpack2t<F16>(v);
                        const float f0 = f01[0], f1 = f01[1];
                        s0 += f0; q0 += f0 * f0;
                        s1 += f1; q1 += f1 * f1;
                    }
                    *reinterpret_cast<f32x4*>(cs_scratch + (rs * CS_CP + cp) * 4) = f32x4{s0, q0, s1, q1};
                }
            }
        }
#pragma unroll
        for (int it = 0; it < (BM * CPR + NT - 1) / NT; ++it) {
            const int c = tid + it * NT;
            const int row = c / CPR, ch = c - row * CPR;
            const int m = m0 + row, n = n0o + ch * 8;
            if (((BM * CPR) % NT == 0 || c < BM * CPR) && m < p.M && n < n_out)
            {
                // write-through below ~3000 of K, where the boundary write-back is a visible share of the launch (projections
                // 11.3 -> 9.6 us, 1x1 shortcuts 15.8 -> 13.8); the long-K convs measured 1-3 % slower with it and keep plain stores
                const u32x4 v = *reinterpret_cast<const u32x4*>(smem + row * CPITCH + (CSWZ ? (ch ^ (row & 15)) : ch) * 16);
                if (wt_store) store16_out(Cb + crow(m) * p.ldc + n, v);
                else *reinterpret_cast<u32x4*>(Cb + crow(m) * p.ldc + n) = v;
            }
        }
        if constexpr (COLSUM_OK) {
            if (p.colsum || p.colsum_fx) {
                __syncthreads();                        // the row-segment partials are parked
                if (tid < BNO && n0o + tid < n_out) {
                    float sm = 0.f, sq = 0.f;
#pragma unroll
                    for (int rs = 0; rs < CS_RS; ++rs) {
                        const float* e = cs_scratch + (rs * CS_CP + (tid >> 1)) * 4 + (tid & 1) * 2;
                        sm += e[0];
                        sq += e[1];
                    }
                    if (p.colsum_fx) {                   // accumulate per batch element (every phase of an upsampling conv adds here)
                        int64_t* o = fx_slot(p, m0 / BM, m0) + n0o + tid;
                        fx_add(o, sm);
                        fx_add(o + p.N, sq);
                    } else {
                        const int tiles_m = (p.M + BM - 1) / BM;
                        float* o = p.colsum + (((int64_t)blockIdx.z * tiles_m + m0 / BM) * p.N + n0o + tid) * 2;
                        *reinterpret_cast<f32x2*>(o) = f32x2{sm, sq};
                    }
                }
            }
        }
    }
    PSTAMP();
    PSPAN(1);
}

// one flag per tile instantiation, at namespace scope (no function-local statics in the library): the dynamic-LDS opt-in of its
// kernels has run
template <int BM, int BN, int NS, int WM, int WN, bool F16>
std::once_flag g_tile_lds_once;

// F16: the IEEE-half instantiation of the same tile (SEER_EPI_F16: the VAE, and the UNet engine under fp16 autocast)
template <int BM, int BN, int NS, int WM = 2, int WN = 2, bool F16 = false>
int launch_tile(const seer_gemm_desc& d, hipStream_t st) {
    const int tiles_m = (d.M + BM - 1) / BM, tiles_n = (d.N + BN - 1) / BN;
    dim3 grid(tiles_m * tiles_n, 1, d.batch > 1 ? d.batch : 1);
    const size_t lds = TileShape<BM, BN, NS, WM, WN>::RING_BYTES;
    constexpr bool GEGLU_OK = TileShape<BM, BN, NS, WM, WN>::GEGLU_OK;
    if (lds > 64 * 1024) {
        // above the default dynamic-LDS limit: opt in once per instantiation (160 KiB per CU on gfx950); std::call_once keeps
        // concurrent first calls from different host threads safe (the header promises thread safety)
        std::call_once(g_tile_lds_once<BM, BN, NS, WM, WN, F16>, [lds] {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&seer_gemm_kernel<BM, BN, true, false, false, NS, WM, WN, F16>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if constexpr (GEGLU_OK)
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&seer_gemm_kernel<BM, BN, false, true, false, NS, WM, WN, F16>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&seer_gemm_kernel<BM, BN, false, false, false, NS, WM, WN, F16>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        });
    }
    const bool conv = d.mode == SEER_GEMM_CONV3X3;
    const bool geglu = (d.epilogue & SEER_EPI_GEGLU) != 0;
    if (conv) {
        hipLaunchKernelGGL((seer_gemm_kernel<BM, BN, true, false, false, NS, WM, WN, F16>), grid, dim3(64 * WM * WN), lds, st, d);
    } else if (geglu) {
        if constexpr (GEGLU_OK)
            hipLaunchKernelGGL((seer_gemm_kernel<BM, BN, false, true, false, NS, WM, WN, F16>), grid, dim3(64 * WM * WN), lds, st, d);
        else
            return SEER_EINVAL;          // (plan_gemm refuses GEGLU on these tiles)
    } else {
        hipLaunchKernelGGL((seer_gemm_kernel<BM, BN, false, false, false, NS, WM, WN, F16>), grid, dim3(64 * WM * WN), lds, st, d);
    }
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

// the K slices of a split-K launch: raw fp32 partial tiles into the workspace; seer_gemm_reduce_launch (gemm_reduce.hip) follows
template <int BM, int BN, int NS, bool F16 = false>
int launch_split_tile(const seer_gemm_desc& d, hipStream_t st) {
    const int tiles_m = (d.M + BM - 1) / BM, tiles_n = (d.N + BN - 1) / BN;
    dim3 grid(tiles_m * tiles_n, 1, d.splits);
    const size_t lds = TileShape<BM, BN, NS>::RING_BYTES;
    if (d.mode == SEER_GEMM_CONV3X3)
        hipLaunchKernelGGL((seer_gemm_kernel<BM, BN, true, false, true, NS, 2, 2, F16>), grid, dim3(256), lds, st, d);
    else
        hipLaunchKernelGGL((seer_gemm_kernel<BM, BN, false, false, true, NS, 2, 2, F16>), grid, dim3(256), lds, st, d);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

}  // namespace
