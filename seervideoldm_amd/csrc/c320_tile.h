// What ff_fused.hip and rowchain.hip share: the 96 x 320 row-owner tile.  Rows of their operators are independent, so a workgroup of
// four waves (one per SIMD) OWNS 96 rows of a 320-channel activation (24 576 rows = 256 workgroups = one per CU, one round) and keeps
// them in LDS for the whole launch:
//   * a tile is five K panels [96 rows][128 B], the 16-byte chunks of a row XOR-swizzled by row & 7; it arrives by LDS-DMA with the
//     swizzle on the source side, is normalised IN PLACE by its kernel (a wave owns 24 rows, 8 lanes a row) and leaves as whole rows;
//   * the weights of a 320 x 320 product STREAM from L2 straight into registers: wave w owns 80 output columns and nobody else reads
//     their rows, so staging them in LDS would buy nothing.  The host packs a matrix in FRAGMENT order (c320_frag_src): every load is
//     one contiguous KiB per wave, and every wait is a compile-time count, because the order of issue never changes;
//   * MFMAs are issued "swapped" (the weight fragment is the A operand), so a lane holds 4 consecutive output columns of one row.
// Only plain fp32 instructions beside MFMAs: packed ones stall them (profiles/r05_lab_mfma_valu.log; build.py turns them off).
// Nothing specific to one of the two kernels lives here.
#pragma once
#include "seer_common.h"
#include <mutex>

// ---- (a) geometry
constexpr int C320_C = 320;                    // channels of the level
constexpr int C320_BM = 96;                    // rows per workgroup
constexpr int C320_KS = C320_C / 64;           // 5 K steps of 64 over the channels
constexpr int C320_PANEL = C320_BM * 128;      // 12 288: one [96 rows][64 k] panel
constexpr int C320_T_BYTES = C320_KS * C320_PANEL;     // 61 440
constexpr int C320_W_BLOCK = 10 * 1024;        // one wave's weight fragments of a K step of 64: [k32 2][5 column fragments][64 lanes][16 B]

// ---- (b) helpers
__device__ __forceinline__ unsigned lds_u32(const void* ptr) {
    return (unsigned)(size_t)(const __attribute__((address_space(3))) void*)ptr;
}
// Every wave issues its vector-memory operations in ONE fixed order, so every wait is a compile-time count of the operations that
// were issued AFTER the one waited for (vmcnt retires in order; older operations -- tile loads, row stores -- retire first).
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// workgroup barrier that leaves the vector-memory counter alone (__syncthreads() drains it)
__device__ __forceinline__ void barrier_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ bf16x8 as_bf(const u32x4& v) { return __builtin_bit_cast(bf16x8, v); }

// ---- (c) fragments that land in registers asynchronously.  The destination registers are outputs of the REQUEST and in-out operands
// of the WAIT; between the two nothing may name them (asm_check.py::check_async_vregs walks the assembly for that).  Two rules follow:
// requests are UNCONDITIONAL (a request under a branch would make the fragment registers a merge of two definitions, and the copy at
// the join would read registers whose load is in flight -- so past the end of a stream a kernel asks for data nobody reads), and a
// fragment has ONE wait site on every path, for the same reason.
// activation fragment: LDS -> registers one sub step ahead.  Rows frow, 16 + frow, ... 80 + frow of a panel (2 KiB apart).
struct AFrag { u32x4 r[6]; };
__device__ __forceinline__ void a_req(AFrag& f, unsigned addr) {
    asm volatile("ds_read_b128 %0, %6\n\tds_read_b128 %1, %6 offset:2048\n\tds_read_b128 %2, %6 offset:4096\n\t"
                 "ds_read_b128 %3, %6 offset:6144\n\tds_read_b128 %4, %6 offset:8192\n\tds_read_b128 %5, %6 offset:10240"
                 : "=&v"(f.r[0]), "=&v"(f.r[1]), "=&v"(f.r[2]), "=&v"(f.r[3]), "=&v"(f.r[4]), "=&v"(f.r[5]) : "v"(addr) : "memory");
}
__device__ __forceinline__ void a_got(AFrag& f) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f.r[0]), "+v"(f.r[1]), "+v"(f.r[2]), "+v"(f.r[3]), "+v"(f.r[4]), "+v"(f.r[5])::"memory");
}
// streamed weight fragment: one K step of a wave's 80 rows, k32 0 x 5 column fragments, k32 1 x 5 (1 KiB apart).  ACC: into
// ACCUMULATION registers -- in flight across a whole epilogue they would be the register allocator's first spill candidates in the V
// file, and a spill of an in-flight register copies stale data; MFMAs take their weight operand from there directly.  (The register
// class is a string of the constraint, which no template argument can carry: one text, two classes.)
template <bool ACC> struct W10 { u32x4 r[10]; };
#define C320_REQ10(RC)                                                                                                                        \
    asm volatile("global_load_dwordx4 %0, %4, %5\n\tglobal_load_dwordx4 %1, %4, %5 offset:1024\n\t"                                           \
                 "global_load_dwordx4 %2, %4, %5 offset:2048\n\tglobal_load_dwordx4 %3, %4, %5 offset:3072"                                   \
                 : "=&" RC(w.r[0]), "=&" RC(w.r[1]), "=&" RC(w.r[2]), "=&" RC(w.r[3]) : "v"(voff), "s"(base) : "memory");                     \
    asm volatile("global_load_dwordx4 %0, %4, %5\n\tglobal_load_dwordx4 %1, %4, %5 offset:1024\n\t"                                           \
                 "global_load_dwordx4 %2, %4, %5 offset:2048\n\tglobal_load_dwordx4 %3, %4, %5 offset:3072"                                   \
                 : "=&" RC(w.r[4]), "=&" RC(w.r[5]), "=&" RC(w.r[6]), "=&" RC(w.r[7]) : "v"(voff), "s"(base + 4096) : "memory");              \
    asm volatile("global_load_dwordx4 %0, %2, %3\n\tglobal_load_dwordx4 %1, %2, %3 offset:1024"                                               \
                 : "=&" RC(w.r[8]), "=&" RC(w.r[9]) : "v"(voff), "s"(base + 8192) : "memory")
#define C320_GOT10(RC)                                                                                                                        \
    asm volatile("s_waitcnt vmcnt(%10)"                                                                                                       \
                 : "+" RC(w.r[0]), "+" RC(w.r[1]), "+" RC(w.r[2]), "+" RC(w.r[3]), "+" RC(w.r[4]), "+" RC(w.r[5]), "+" RC(w.r[6]),            \
                   "+" RC(w.r[7]), "+" RC(w.r[8]), "+" RC(w.r[9])                                                                             \
                 : "n"(N) : "memory")
template <bool ACC> __device__ __forceinline__ void req10(W10<ACC>& w, unsigned voff, const unsigned char* base) {
    if constexpr (ACC) { C320_REQ10("a"); } else { C320_REQ10("v"); }
}
template <int N, bool ACC> __device__ __forceinline__ void got10(W10<ACC>& w) {
    if constexpr (ACC) { C320_GOT10("a"); } else { C320_GOT10("v"); }
}
#undef C320_REQ10
#undef C320_GOT10

// ---- (d) a tile between global memory and LDS.  A piece = 8 rows x 128 B; lane l -> row drow = l >> 3, LDS position l & 7 holds
// source chunk (l & 7) ^ (row & 7), dchunk = its element offset inside the 64-wide K step; 60 pieces, 15 per wave.  This thread's
// place in the tile of rows m0 .. m0 + 95 of an M-row operand: the kernel's own values, held as the code this replaces held them --
// I = int in ff_fused.hip (its store was written out in the kernel), const int& in rowchain.hip (its stager and store were closures).
// Either kernel compiles to other instructions with the other choice, or with drow / dchunk computed here (profiles/c320_tile.md).
template <class I> struct C320Place {
    I m0, wave, lane;
    const int& M;                           // (the kernel's argument field, read where it is used)
    I drow, dchunk;
    // LDS-DMA of an activation tile
    __device__ __forceinline__ void load_tile(unsigned char* dst, const bf16* src, int ld) const {
#pragma unroll
        for (int i = 0; i < 15; ++i) {
            const int q = wave * 15 + i, pnl = q / 12, rg = q - pnl * 12;
            const int m = min(m0 + rg * 8 + drow, M - 1);              // (a ragged last tile reads its last row again)
            const bf16* s = src + (int64_t)m * ld + pnl * 64 + dchunk;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)s,
                                             (__attribute__((address_space(3))) void*)(dst + pnl * C320_PANEL + rg * 1024), 16, 0, 0);
        }
    }
    // whole rows of a tile out: the inverse.  FULL: every row of every tile is inside the operand
    template <bool FULL> __device__ __forceinline__ void store_tile(const unsigned char* src, bf16* dst, int ld) const {
#pragma unroll
        for (int i = 0; i < 15; ++i) {
            const int q = wave * 15 + i, pnl = q / 12, rg = q - pnl * 12;
            const u32x4 v = *reinterpret_cast<const u32x4*>(src + pnl * C320_PANEL + rg * 1024 + lane * 16);
            if (FULL || m0 + rg * 8 + drow < M) store16_out(dst + (int64_t)(m0 + rg * 8 + drow) * ld + pnl * 64 + dchunk, v);
        }
    }
};
// the quad (row, columns n .. n + 3), n a multiple of 4, of the tile at `base`: what a lane of an epilogue reads or writes.  base: a
// pointer, or 0 for the byte offset that two tiles share
template <class B> __device__ __forceinline__ B c320_quad(B base, int row, int n) {
    return base + (n >> 6) * C320_PANEL + row * 128 + ((((n & 63) >> 3) ^ (row & 7)) * 16) + (n & 7) * 2;
}
// ... of row 16 i + frow, for an epilogue that has no other use for the row
template <class B> __device__ __forceinline__ B c320_quad(B base, int i, int frow, int n) { return c320_quad(base, 16 * i + frow, n); }

// ---- (e) Y += T W^T for the five K steps of one fragment-packed 320 x 320 matrix `w` (this wave's block of it), T at LDS address T0.
// On entry K steps 0 and 1 are requested (w0, w1); `head` holds the caller's waits for them, its ONE wait site (c).  Sub step
// (s, k32) reads panel s at this lane's offsets fo0 / fo1; the next sub step's activation fragments are requested before this one's
// MFMAs, and a K step's registers are requested again, two steps on, as soon as its last MFMA has issued.
// CHAIN: before it returns, the first two K steps of `next` are requested -- the next product's requests ride under this one's last
// MFMAs and its epilogue (S1 before S0).  Not CHAIN: nothing is requested behind S4.
template <bool CHAIN, bool ACC, class Head, class Mfma>
__device__ __forceinline__ void c320_product(W10<ACC>& w0, W10<ACC>& w1, unsigned T0, unsigned fo0, unsigned fo1, unsigned voff,
                                             const unsigned char* w, const unsigned char* next, Head&& head, Mfma&& mfma_y) {
    AFrag a0, a1;
    a_req(a0, T0 + fo0);
    a_got(a0);
    head();
    // S0 (w0)
    a_req(a1, T0 + fo1);                                    mfma_y(&w0.r[0], a0); a_got(a1);
    a_req(a0, T0 + C320_PANEL + fo0);                       mfma_y(&w0.r[5], a1); a_got(a0);
    req10(w0, voff, w + 2 * 4 * C320_W_BLOCK);                                     // S2 -> w0
    // S1 (w1)
    a_req(a1, T0 + C320_PANEL + fo1);                       mfma_y(&w1.r[0], a0); a_got(a1);
    a_req(a0, T0 + 2 * C320_PANEL + fo0);                   mfma_y(&w1.r[5], a1); a_got(a0);
    req10(w1, voff, w + 3 * 4 * C320_W_BLOCK);                                     // S3 -> w1; behind S2: S3
    // S2
    a_req(a1, T0 + 2 * C320_PANEL + fo1); got10<10>(w0);    mfma_y(&w0.r[0], a0); a_got(a1);
    a_req(a0, T0 + 3 * C320_PANEL + fo0);                   mfma_y(&w0.r[5], a1); a_got(a0);
    req10(w0, voff, w + 4 * 4 * C320_W_BLOCK);                                     // S4 -> w0; behind S3: S4
    // S3
    a_req(a1, T0 + 3 * C320_PANEL + fo1); got10<10>(w1);    mfma_y(&w1.r[0], a0); a_got(a1);
    a_req(a0, T0 + 4 * C320_PANEL + fo0);                   mfma_y(&w1.r[5], a1); a_got(a0);
    if constexpr (CHAIN) req10(w1, voff, next + 1 * 4 * C320_W_BLOCK);             // the next product's S1 -> w1; behind S4: that
    // S4
    a_req(a1, T0 + 4 * C320_PANEL + fo1); got10<CHAIN ? 10 : 0>(w0); mfma_y(&w0.r[0], a0); a_got(a1);
    mfma_y(&w0.r[5], a1);
    if constexpr (CHAIN) req10(w0, voff, next);                                    // ... and its S0 -> w0
}
// the 30 MFMAs of one sub step: six row fragments x five column fragments
template <bool F16> __device__ __forceinline__ void c320_mfma_y(f32x4 (&Y)[6][5], const u32x4* w5, const AFrag& a) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j) Y[i][j] = mma16<F16>(as_bf(w5[j]), as_bf(a.r[i]), Y[i][j]);
}

// ---- (f) fragment order of a packed matrix with 320 rows, one thread per 16 bytes: unit ii of the pack is
// out[s][w][k32][j][lane] = W[row0 + 80 w + 16 j + (lane & 15)][64 s + 32 k32 + 8 (lane >> 4) .. + 7]
struct C320Src { int row, k; };
__device__ __forceinline__ C320Src c320_frag_src(int ii, int row0) {
    const int lane = ii & 63, r = ii >> 6;                  // r = ((s * 4 + w) * 2 + k32) * 5 + j
    const int j = r % 5, r2 = r / 5, k32 = r2 & 1, w = (r2 >> 1) & 3, s = r2 >> 3;
    return {row0 + 80 * w + 16 * j + (lane & 15), 64 * s + 32 * k32 + 8 * (lane >> 4)};
}

// ---- (g) host side
// a row stride (elements) that a 320-wide operand of these kernels can have: rows of whole 16-byte chunks, at least the tile's width
inline bool c320_ld_ok(int64_t ld) { return ld % 8 == 0 && ld >= C320_C; }
template <class... P> inline bool c320_misaligned16(const P*... p) { return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) != 0; }
// opts the four <F16, flag> instantiations of a kernel template in to `bytes` of dynamic LDS, once per process (`once`: a
// namespace-scope std::once_flag of the caller's)
#define C320_LDS_OPT_IN(once, kernel, bytes)                                                                                          \
    std::call_once(once, [] {                                                                                                         \
        for (const void* k : {reinterpret_cast<const void*>(&kernel<false, false>), reinterpret_cast<const void*>(&kernel<true, false>), \
                              reinterpret_cast<const void*>(&kernel<false, true>), reinterpret_cast<const void*>(&kernel<true, true>)})   \
            (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);                                         \
    })
