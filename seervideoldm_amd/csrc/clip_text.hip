// The two kernels of the CLIP text tower (transformers CLIPTextModel, the text_encoder of runwayml/stable-diffusion-v1-5) that the
// engine's GEMM / LayerNorm kernels do not cover (include/seer_hip.h: seer_attn_causal64, seer_embed_tokens).
//
// seer_attn_causal64: causal self-attention with a key padding mask over one short sequence (L <= 128), head_dim 64.
//   One wave per (sample, head, 16-query tile).  Query tile t sees key tiles 0..t only, and sees ALL of them in one pass: the
//   scores of the tile's 16 queries against up to 128 keys are 8 accumulator quads per lane, so the softmax is a plain two-pass
//   max / sum over registers -- no online rescaling, no running statistics.
//     S^T = K Q^T   v_mfma_f32_16x16x32_bf16, A = K fragment (rows = keys), B = Q fragment: both are 16-byte global loads of the
//                   token-major rows as they are (lane (r, g) holds row r, columns 8g..8g+7 of a 32-wide K step); no LDS.
//                   D: lane (c, g) holds keys 4g..4g+3 of the tile for query c -- one query per lane column, so max and sum are
//                   in-lane over the quads plus two lane exchanges (xor 16, xor 32).
//     O^T = V^T P^T the accumulator quads of TWO key tiles, rounded to bf16, ARE the B operand of a 32-key step (lane (c, g), element
//                   e: key 4g + e of the even tile for e < 4, key 4g + e - 4 of the odd tile for e >= 4).  The matching A operand
//                   is V^T in that key order: V is staged once into LDS transposed, Vt[d][pos(key)] with
//                   pos = 32 (key / 32) + 8 ((key / 4) % 4) + 4 ((key / 16) % 2) + key % 4, so a fragment is one 16-byte LDS read.
//                   D: lane (c, g) holds channels 4g..4g+3 of a 16-channel tile for query c: the 1/sum is in-lane, the store 8 bytes.
//   Grid per 16-query tile rather than per (sample, head): at b = 1 a (sample, head) grid is 12 waves on 256 CUs; the tiles make
//   it 60, and the V of a head (<= 16 KB) is read from L2 by at most 8 of them.  Blocks are numbered longest tile first.
#include "seer_common.h"

namespace {

constexpr int HD = 64;                  // head dim
constexpr int LMAX = 128;               // longest sequence: 8 key tiles of 16 = 32 score registers per lane
constexpr int VPITCH = LMAX + 8;        // Vt row pitch (elements): 272 B = 17 chunks of 16 B, odd: rows d, d+1, .. spread over the banks
constexpr float kNegInf = -__builtin_inff();

__global__ void __launch_bounds__(64) seer_attn_causal64_kernel(const bf16* __restrict__ Q, const bf16* __restrict__ K,
                                                                  const bf16* __restrict__ V, const int ld, bf16* __restrict__ O,
                                                                  const int ldo, const uint8_t* __restrict__ mask, const int heads,
                                                                  const int L, const int qtiles) {
    __shared__ __attribute__((aligned(16))) bf16 vt[HD * VPITCH];
    const int lane = threadIdx.x;
    const int fr = lane & 15, g = lane >> 4;
    int blk = blockIdx.x;
    const int t = qtiles - 1 - blk % qtiles;        // longest tiles first
    blk /= qtiles;
    const int head = blk % heads, b = blk / heads;
    const int64_t row0 = (int64_t)b * L;
    const int col = head * HD;
    const int nkt = t + 1;                          // key tiles 0..t
    const int nk32 = (nkt + 1) >> 1;                // 32-key steps of the PV product

    // ---- V -> LDS, transposed, in the key order of the P fragments; keys >= L are zeros (P is 0 there: 0 * garbage must stay 0)
    for (int i = lane; i < nk32 * 32 * (HD / 8); i += 64) {
        const int key = i >> 3, c = i & 7;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (key < L) v = *reinterpret_cast<const u32x4*>(V + (row0 + key) * ld + col + 8 * c);
        const int pos = (key & ~31) + 8 * ((key >> 2) & 3) + 4 * ((key >> 4) & 1) + (key & 3);
        const bf16x8 e = __builtin_bit_cast(bf16x8, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) vt[(8 * c + k) * VPITCH + pos] = e[k];
    }

    // ---- S^T = K Q^T
    const int q = t * 16 + fr;                      // this lane's query
    const int qrow = q < L ? q : L - 1;
    bf16x8 qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(Q + (row0 + qrow) * ld + col + 32 * ks + 8 * g);
    float s[8][4];
    float m = kNegInf;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int r = 0; r < 4; ++r) s[j][r] = kNegInf;
        if (j < nkt) {                              // wave-uniform
            const int kr = 16 * j + fr;
            const bf16* kp = K + (row0 + (kr < L ? kr : L - 1)) * ld + col + 8 * g;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = mma16<false>(*reinterpret_cast<const bf16x8*>(kp), qf[0], acc);
            acc = mma16<false>(*reinterpret_cast<const bf16x8*>(kp + 32), qf[1], acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = 16 * j + 4 * g + r;
                bool vis = key <= q && key < L;
                if (vis && mask) vis = mask[row0 + key] != 0;
                if (vis) {
                    s[j][r] = acc[r];
                    m = fmaxf(m, acc[r]);
                }
            }
        }
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    // a query without a visible key: every s is -inf; with m = 0 every p is exp2(-inf) = 0, the sum 0 and the row is written as zeros
    const float ms = m == kNegInf ? 0.f : m;
    float lsum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[j][r] = __builtin_amdgcn_exp2f(s[j][r] - ms);       // Q carries scale * log2(e)
            lsum += s[j][r];
        }
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    const float inv = lsum > 0.f ? 1.0f / lsum : 0.f;

    __syncthreads();                                // Vt is complete

    // ---- O^T = V^T P^T
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        if (jj < nk32) {                            // wave-uniform
            bf16x8 pb;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pb[r] = (bf16)s[2 * jj][r];
                pb[4 + r] = (bf16)s[2 * jj + 1][r];
            }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const bf16x8 vf = *reinterpret_cast<const bf16x8*>(vt + (16 * dt + fr) * VPITCH + 32 * jj + 8 * g);
                o[dt] = mma16<false>(vf, pb, o[dt]);
            }
        }
    }
    if (q < L) {
        bf16* op = O + (row0 + q) * ldo + col + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
            *reinterpret_cast<u32x2*>(op + 16 * dt) = u32x2{pack2(o[dt][0] * inv, o[dt][1] * inv), pack2(o[dt][2] * inv, o[dt][3] * inv)};
    }
}

// x[row][:] = tok[clamp(ids[row])][:] + pos[row % L][:], fp32 sum, bf16 store; one block per row, 16 bytes per thread and step
__global__ void __launch_bounds__(128) seer_embed_tokens_kernel(const int64_t* __restrict__ ids, const bf16* __restrict__ tok,
                                                                 const bf16* __restrict__ pos, bf16* __restrict__ x, const int L,
                                                                 const int vocab, const int C, const int ldx) {
    const int64_t row = blockIdx.x;
    int64_t id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);          // no id reads outside the table
    const bf16* tp = tok + id * C;
    const bf16* pp = pos + (row % L) * C;
    bf16* xp = x + row * ldx;
    for (int c = threadIdx.x * 8; c < C; c += 128 * 8) {
        float a[8], p[8];
        unpack8(*reinterpret_cast<const u32x4*>(tp + c), a);
        unpack8(*reinterpret_cast<const u32x4*>(pp + c), p);
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] += p[k];
        *reinterpret_cast<u32x4*>(xp + c) = pack8(a);
    }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" int seer_attn_causal64(const void* Q, const void* K, const void* V, int32_t ld_qkv, void* O, int32_t ldo,
                                  const uint8_t* key_mask, int32_t batch, int32_t heads, int32_t L, void* stream) {
    if (!Q || !K || !V || !O || !aligned(Q, 16) || !aligned(K, 16) || !aligned(V, 16) || !aligned(O, 8)) return SEER_EINVAL;
    if (batch <= 0 || heads <= 0 || L <= 0) return SEER_EINVAL;
    if ((int64_t)heads * HD > ld_qkv || ld_qkv % 8 || (int64_t)heads * HD > ldo || ldo % 4) return SEER_EINVAL;
    if (L > LMAX) return SEER_ENOSYS;               // longer sequences need the tiled kernel (seer_attn_fwd), not built at head_dim 64
    const int qtiles = (L + 15) / 16;
    const int64_t blocks = (int64_t)batch * heads * qtiles;
    if (blocks > 0x7fffffffLL || (int64_t)batch * L > 0x7fffffffLL) return SEER_ENOSYS;
    hipLaunchKernelGGL(seer_attn_causal64_kernel, dim3((unsigned)blocks), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const bf16*>(Q), reinterpret_cast<const bf16*>(K), reinterpret_cast<const bf16*>(V), ld_qkv,
                       reinterpret_cast<bf16*>(O), ldo, key_mask, heads, L, qtiles);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}

extern "C" int seer_embed_tokens(const int64_t* ids, int32_t batch, int32_t L, const void* tok, int32_t vocab, const void* pos,
                                 int32_t L_max, int32_t C, void* x, int32_t ldx, void* stream) {
    if (!ids || !tok || !pos || !x || !aligned(ids, 8) || !aligned(tok, 16) || !aligned(pos, 16) || !aligned(x, 16)) return SEER_EINVAL;
    if (batch <= 0 || L <= 0 || L > L_max || vocab <= 0 || C <= 0 || C % 8 || ldx < C || ldx % 8) return SEER_EINVAL;
    const int64_t rows = (int64_t)batch * L;
    if (rows > 0x7fffffffLL) return SEER_ENOSYS;
    hipLaunchKernelGGL(seer_embed_tokens_kernel, dim3((unsigned)rows), dim3(128), 0, reinterpret_cast<hipStream_t>(stream), ids,
                       reinterpret_cast<const bf16*>(tok), reinterpret_cast<const bf16*>(pos), reinterpret_cast<bf16*>(x), L, vocab, C,
                       ldx);
    SEER_LAUNCH_CHECK();
    return SEER_OK;
}
