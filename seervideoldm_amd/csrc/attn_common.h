// What attention.hip, attention40.hip and attention_bwd.hip share: the window token map and the block decode, the lane-half
// exchange, the tile geometry of a head dim, the transposed LDS fragment read (also gemm_tn.hip's), the two-operand tile stager, and
// the host checks of a descriptor's addressing.  Nothing specific to one kernel lives here.
#pragma once
#include "seer_common.h"

// ---- (a) token addressing.  Position `pos` of a (window, batch, head) sequence -> token row of the [F][H][W] frame stack:
// identity without a window, else frame pos / ws^2 and the (wy, wx) of pos inside the ws x ws window whose corner is (wy0, wx0).
struct AttnTokMap {
    int ws_log2;   // -1: identity
    int HW, W_, wy0, wx0;
    __device__ __forceinline__ int operator()(int pos) const {
        if (ws_log2 < 0) return pos;
        const int ws2 = 2 * ws_log2;
        const int f = pos >> ws2;
        const int rem = pos & ((1 << ws2) - 1);
        const int wy = rem >> ws_log2, wx = rem & ((1 << ws_log2) - 1);
        return f * HW + (wy0 + wy) * W_ + wx0 + wx;
    }
};
// block row y = (window, batch, head), head fastest -> head, batch element b and the map of the block's window
__device__ __forceinline__ AttnTokMap attn_block_origin(const seer_attn_desc& p, int ws_log2, int y, int& head, int& b) {
    head = y % p.heads;
    b = y / p.heads;
    AttnTokMap tok;
    tok.ws_log2 = ws_log2;
    tok.HW = p.H * p.W;
    tok.W_ = p.W;
    tok.wy0 = tok.wx0 = 0;
    if (ws_log2 >= 0) {
        const int win = b / p.batch;
        b = b - win * p.batch;
        const int nwx = p.W >> ws_log2;
        tok.wy0 = (win / nwx) << ws_log2;
        tok.wx0 = (win % nwx) << ws_log2;
    }
    return tok;
}

// ---- (b) v_permlane32_swap a, b:  a' = [a.lo | b.lo], b' = [a.hi | b.hi]; with a = b = v every lane sees both halves' values.
// Inline asm, not __builtin_amdgcn_permlane32_swap: hipcc (ROCm 7.2) returns the builtin's FIRST result for both elements of
// its result pair (scripts/lab_probe3.cpp prints it; the same holds for permlane16_swap), so max(r[0], r[1]) silently dropped the
// other half's 16 keys from the running maximum.  Mild scores hide that (any reference near the maximum is fine); scores 130+ log2
// units apart overflowed exp2 and gave NaN rows -- found by the sharp-softmax cases of scripts/lab_attn.cpp / tests/test_gpu_kernels.py.
// The s_nop pair covers the VALU-write -> permlane-read hazard, which nobody pads inside an asm statement.
__device__ __forceinline__ float xhalf_max(float v) {
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
    return fmaxf(a, b);
}
__device__ __forceinline__ float lower_half_value(float v) {      // value of lane (l & 31) in every lane l
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
    return a;
}

// ---- (c) tile geometry of head dim D in the kernels that stream ATTN_KT-row tiles through padded LDS images
constexpr int ATTN_KT = 64;
template <int D>
struct AttnGeom {
    static constexpr int DP = (D + 15) / 16 * 16;      // contraction length of the row products (zero padded)
    static constexpr int KSTEPS = DP / 16;
    static constexpr int NDT = (D + 31) / 32;          // 32-row d tiles of a transposed accumulator
    static constexpr int DV = NDT * 32;
    static constexpr int RS = DP + 8;                  // padded row stride (elements): odd number of 16-byte chunks
    static constexpr int CH = D / 8;                   // 16-byte chunks per row in global memory
    static constexpr int NCH = (ATTN_KT * CH + 255) / 256;   // chunks per thread per tile and operand
};

// ---- (d) one A fragment out of a row-major [row][column] LDS image by hardware transpose: two ds_read_b64_tr_b16, the second
// 8 rows (rows8_stride elements) further on
__device__ __forceinline__ bf16x8 tr_frag(const bf16* a0, int rows8_stride) {
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(a0));
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(a0 + rows8_stride));
    bf16x8 f;
    f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3];
    f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
    return f;
}

// ---- (e) the two-operand tile stager of a 256-thread block: ATTN_KT rows of two row-major global operands (row strides ss1 / ss2
// elements, D columns) travel through registers into two LDS images.  prefetch: rows row0 .. row0 + ATTN_KT - 1 of an n-row sequence
// through the token map, rows past the end clamped to n - 1 (their scores are masked); commit: into images of row strides rs1 / rs2.
// tid is the kernel's own threadIdx.x, and ss1 / ss2 / n are references to the descriptor fields the kernel names: taken by value
// (or tid re-read here) hipcc hoists n - 1 and the stride reads out of the two call sites and picks another division of idx at
// D = 160 -- a few scalar adds fewer, but not the instruction streams the kernels were measured with (profiles/attn_common.md).
template <int D>
struct AttnStager {
    using G = AttnGeom<D>;
    u32x4 r1[G::NCH], r2[G::NCH];
    __device__ __forceinline__ void prefetch(int tid, const AttnTokMap& tok, const bf16* __restrict__ g1, const int& ss1,
                                             const bf16* __restrict__ g2, const int& ss2, int row0, const int& n) {
#pragma unroll
        for (int i = 0; i < G::NCH; ++i) {
            const int idx = tid + 256 * i;
            if (idx < ATTN_KT * G::CH) {
                const int row = idx / G::CH, ch = idx - row * G::CH;
                int rg = row0 + row;
                rg = rg < n ? rg : n - 1;
                const int64_t tr = tok(rg);
                r1[i] = *reinterpret_cast<const u32x4*>(g1 + tr * ss1 + ch * 8);
                r2[i] = *reinterpret_cast<const u32x4*>(g2 + tr * ss2 + ch * 8);
            }
        }
    }
    __device__ __forceinline__ void commit(int tid, bf16* img1, int rs1, bf16* img2, int rs2) const {
#pragma unroll
        for (int i = 0; i < G::NCH; ++i) {
            const int idx = tid + 256 * i;
            if (idx < ATTN_KT * G::CH) {
                const int row = idx / G::CH, ch = idx - row * G::CH;
                *reinterpret_cast<u32x4*>(img1 + row * rs1 + ch * 8) = r1[i];
                *reinterpret_cast<u32x4*>(img2 + row * rs2 + ch * 8) = r2[i];
            }
        }
    }
};

// ---- (f) host side
// (window, batch) pairs of a launch: grid rows = this * heads
inline int attn_launch_batches(const seer_attn_desc& d, int ws_log2) {
    return ws_log2 < 0 ? d.batch : d.batch * (d.H >> ws_log2) * (d.W >> ws_log2);
}
// window and causal fields of a descriptor; *ws_log2 = -1 without a window.  same_frames: the backward's rule (queries and keys are
// the same F frames) instead of the forward's (Fq > 0 query frames of a frame shard against F key frames)
inline int attn_check_addressing(const seer_attn_desc& d, int* ws_log2, bool same_frames) {
    *ws_log2 = -1;
    if (d.window_ws > 0) {
        if (d.window_ws != 4 && d.window_ws != 8) return SEER_EINVAL;
        *ws_log2 = d.window_ws == 4 ? 2 : 3;
        if (d.H % d.window_ws || d.W % d.window_ws) return SEER_EINVAL;
        if (same_frames ? (d.Fq != d.F || d.Sk != d.Sq) : d.Fq <= 0) return SEER_EINVAL;
        if (d.Sq != d.Fq * d.window_ws * d.window_ws || d.Sk != d.F * d.window_ws * d.window_ws) return SEER_EINVAL;
    }
    if (d.causal_offset < 0 || (d.causal && d.Sq + d.causal_offset > d.Sk)) return SEER_EINVAL;
    return SEER_OK;
}
int seer_attn40_launch(const seer_attn_desc& d, int ws_log2, hipStream_t st);   // attention40.hip, called by seer_attn_fwd for head_dim 40
