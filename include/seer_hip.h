/*
 * seer_hip.h -- C ABI of libseer_hip.so: the MI355X (gfx950) device kernels behind the
 * Seer DDIM denoising hot path (SeerUNet forward + CFG + DDIM update + VAE decode), the two steps that feed it
 * (FSTextTransformer, VAE encode), the CLIP text tower in front of those, and the fine-tuning step of train.py (backward kernels, AdamW).
 *
 * Boundary rules (all entry points):
 *   - extern "C", plain pointers and sizes; every pointer is DEVICE memory unless it says "host".
 *   - explicit stream (a hipStream_t passed as void*); nothing here synchronises, allocates or
 *     keeps global state, so every call is hipGraph-capturable and thread-safe.
 *   - returns 0 on success, a negative SEER_E* code otherwise (never throws).
 *   - activations are token-major / channels-last bf16: [B*F, H*W, C]  (a "token row" = one latent pixel
 *     of one frame; C contiguous).  Weights are bf16 [N][K] with K contiguous
 *     (nn.Linear [out,in] as is; conv [Co,Ci,3,3] repacked to [Co][ky][kx][Ci]).
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference repo).
 */
#ifndef SEER_HIP_H
#define SEER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEER_OK 0
#define SEER_EINVAL (-22)   /* bad shape / alignment / flag combination */
#define SEER_ENOSYS (-38)   /* shape class not built (e.g. head dim) */
#define SEER_ELAUNCH (-5)   /* hipLaunchKernel reported an error */

/* storage type of 16-bit tensors: bf16 by default on the UNet path, IEEE half on the VAE path (the reference decodes in fp32:
 * inference_img.py:118) and in the UNet engine under fp16 autocast.  Every entry point with a `dtype` argument runs the same kernel
 * on either storage type -- wherever its comment says bf16, read "the storage type `dtype`" -- and returns SEER_EINVAL for any other
 * code (ahead of any SEER_ENOSYS shape refusal). */
#define SEER_DT_BF16 0
#define SEER_DT_F16 1

/* library / device info ------------------------------------------------------------------- */
#define SEER_ABI_VERSION 27                 /* bumps when a struct or an entry point below changes */
int seer_abi_version(void);                 /* SEER_ABI_VERSION of the header the library was built from */
const char* seer_strerror(int code);        /* host string */
const char* seer_build_arch(void);          /* "gfx950" */

/* ---- GEMM / implicit-GEMM convolution --------------------------------------------------- */
/* Replaces: nn.Linear (seer/models/attention.py:484-489,742,783), InflatedConv3d 1x1
 * (attention.py:111,126; resnet.py:172) and InflatedConv3d 3x3 incl. stride-2 Downsample3D and the
 * nearest-2x Upsample3D that precedes a conv (resnet.py:8-16,39,52-57,82,144,153).
 *   C[m, n] = epilogue( sum_k A(m, k) * W[n, k] )
 * A(m,k):  mode PLAIN  : A[m*lda + k] for k < K1, A2[m*lda2 + (k-K1)] for k >= K1 (channel concat of two
 *                        tensors: the skip concat of unet_3d_blocks.py:596,712 without materialising it)
 *          mode CONV3X3: m -> (img, oy, ox); k -> (ky, kx, ci);  X[img, oy*stride+ky-1, ox*stride+kx-1, ci]
 *                        (zero outside), read through a nearest 2x upsample when `upsample` == 1.
 *                        `upsample` == 2: the same Upsample3D conv (resnet.py:52-57) as its four 2x2 PHASE convs -- output
 *                        pixel (2y+a, 2x+b) only ever sees source rows y+a-1, y+a and columns x+b-1, x+b, so phase (a, b)
 *                        is a 4-tap conv over the SOURCE grid with taps summed per source pixel (16 tap-products per
 *                        source pixel instead of 36).  M = n_img*Hin*Win, K = 4*Cin with k -> (ty, tx, ci),
 *                        W = [4 phases (a*2+b)][N][K] (seervideoldm_amd.weights.pack_conv3x3_up_phases), Hout = 2 Hin,
 *                        Wout = 2 Win; the launch runs the four phases as its grid.z and scatters the rows into
 *                        C [n_img*Hout*Wout, ldc].  bias and col_scale only (no residual / rowvec / fp32 / transposed out).
 * epilogue: + bias[n] ; + rowvec[(m / rows_per_batch), n] (the time-embedding add of resnet.py:191-193);
 *           + residual[m*ldr + n] ; GEGLU (attention.py:791-793): W rows are interleaved in groups of 16
 *           (16 value rows, then their 16 gate rows), output is N/2 wide: val * gelu_erf(gate).
 * K (and K1) must be multiples of 64; N a multiple of 4 (32 for GEGLU); lda/ldc/ldr multiples of 8.
 */
#define SEER_GEMM_PLAIN 0
#define SEER_GEMM_CONV3X3 1
#define SEER_EPI_GEGLU 1u      /* fused a * gelu(g) */
#define SEER_EPI_OUT_F32 2u    /* C is fp32 instead of bf16 */
#define SEER_EPI_SILU 4u       /* C = silu(acc + bias) (time_embedding.linear_1) */
#define SEER_EPI_TRANS_OUT 8u  /* store C transposed: Ct[n*ldc + m] (used for V^T in the VAE attention) */
#define SEER_EPI_ROTARY 16u    /* rotate the q|k columns (n < rot_cols) of a fused q|k|v projection (attention.py:649-651) */
#define SEER_EPI_COLSCALE 32u  /* multiply the output columns n < col_scale_cols by col_scale (after bias / rotary): the q columns
                                * of a projection leave the GEMM as q * scale * log2(e), rounded to bf16 ONCE, for
                                * SEER_ATTN_Q_PRESCALED (attention.py:622-630 applies the scale inside the attention op) */

#define SEER_EPI_F16 64u       /* A, A2, W, residual and C hold IEEE half (fp16) instead of bf16; fp32 accumulation as always.  For the
                                * VAE, which the reference never autocasts (inference_img.py:118, ddim_sampling_utils.py:37-41):
                                * 11 significand bits at the bf16 MFMA rate.  Plain and conv launches, unsplit; not with GEGLU,
                                * rotary or colsum */
#define SEER_EPI_QUICKGELU 128u /* C = v * sigmoid(1.702 v), v = acc + bias: CLIP's quick-GELU (transformers QuickGELUActivation; the
                                * text tower's mlp.fc1).  Applied where SEER_EPI_SILU is, and refused by the same launch classes (the
                                * weight-stationary kernel, the 256 x 320 tile, the folded LayerNorm: such a request runs on the tile
                                * kernel).  Together with SEER_EPI_SILU: SEER_EINVAL */

typedef struct seer_gemm_desc {
    const void* A;          /* bf16 */
    const void* A2;         /* bf16 or NULL */
    const void* W;          /* bf16 [N][K] */
    const float* bias;      /* fp32 [N] or NULL */
    const void* residual;   /* bf16 [M][ldr] or NULL */
    const float* rowvec;    /* fp32 [M/rows_per_batch][rowvec_ld] or NULL */
    void* C;                /* bf16 (or fp32) [M][ldc] */
    int32_t M, N, K, K1;
    int32_t lda, lda2, ldr, ldc;
    int32_t rows_per_batch, rowvec_ld;
    int32_t mode;           /* SEER_GEMM_* */
    uint32_t epilogue;      /* SEER_EPI_* flags */
    /* conv geometry (mode CONV3X3): input NHWC [n_img, Hin, Win, Cin] (pre-upsample size) */
    int32_t Hin, Win, Cin, Hout, Wout, stride, upsample;
    /* batched GEMM (grid.z): element strides; batch<=1 means a single problem */
    int32_t batch;
    int64_t strideA, strideW, strideC;
    /* tile selection: 0 = auto, else SEER_TILE_* */
    int32_t tile;
    /* split-K (small M, long K: the 4x4 / 8x8 level convs): 0 = auto, 1 = off, n = n slices of the K loop.  Slices write
     * fp32 partial tiles to `workspace` ([splits][M][N] floats) and a second kernel adds them IN SLICE ORDER (deterministic,
     * no atomics) and applies the epilogue.  Ignored (no split) when workspace is NULL or too small. */
    int32_t splits;
    void* workspace;
    int64_t workspace_bytes;
    /* SEER_EPI_ROTARY: cos/sin table of seer_rotary_table ([pos][rot_dim/2][2] fp32); position of row m is
     * m % rot_tokens_per_batch + rot_pos_offset; columns n < rot_cols are heads of rot_head_dim channels of which the first
     * rot_dim are rotated (interleaved pairs) */
    const float* rot_table;
    int32_t rot_tokens_per_batch, rot_pos_offset, rot_head_dim, rot_dim, rot_cols;
    /* CONV3X3 padding: 0 = one pixel on every side (every conv of the UNet and the VAE decoder); 1 = only after the last row
     * and column, X[img, oy*stride+ky, ox*stride+kx, ci] -- the VAE encoder's Downsample, F.pad(x, (0,1,0,1)) + conv(stride 2,
     * padding 0) (ldm/modules/diffusionmodules/model.py:60-78) */
    int32_t pad_after_only;
    /* SEER_EPI_COLSCALE */
    int32_t col_scale_cols;
    float col_scale;
    /* optional: per-tile column sums of C as stored (bf16-rounded), colsum[z][ceil(M / rows)][N][2] = (sum, sum of squares) over
     * the tile's rows, rows = seer_gemm_colsum_rows(desc), z = the phase of an upsample == 2 conv (else 0).  The GroupNorm that
     * consumes C (ResnetBlock3D.norm1/norm2, SpatialTransformer3D.norm: resnet.py / attention.py of the reference run
     * F.group_norm on it) takes its statistics from these sums instead of a pass over C: seer_groupnorm_stats_from_colsums.
     * A split-K launch leaves them through its reduce pass (rows = 4 or 16).  A launch that cannot produce them (GEGLU, fp32 /
     * transposed output, the weight-stationary kernel) fails with SEER_EINVAL when colsum is set: ask seer_gemm_colsum_rows
     * first. */
    float* colsum;
    /* in-launch split-K (the 256 x 320 tile kernel, SEER_TILE_T256x320): two 32-bit counters per output tile,
     * seer_gemm_sync_bytes(desc) bytes.  ZERO before the first launch that uses them; every launch leaves them zero again, so
     * one buffer serves all launches that are ordered on one stream (launches that may overlap in time need their own).  NULL:
     * the launch falls back to the two-launch split-K of the smaller tiles. */
    void* sync;
    int64_t sync_bytes;
    /* the same column sums, ACCUMULATED per batch element in 64-bit fixed point instead of written per tile:
     * colsum_fx[rep][b][2][N] (planes: sum, sum of squares) += round(partial * 2^SEER_GN_FX_SHIFT) by integer atomic adds, b = (first
     * row of the partial) / colsum_fx_rows, rep = (index of the partial) % colsum_fx_reps (replicas keep the adds per address
     * low: an atomic on one address retires every ~12 ns).  Integer addition commutes, so the totals do not depend on the
     * order the tiles finish in (bit-identical from run to run, like the per-tile form).  ZERO the buffer before the first launch
     * that adds to it; every launch whose rows belong to the same tensor (the four phases of an upsample == 2 conv) adds to the
     * same buffer.  colsum_fx_reps and the row granularity come from seer_gemm_colsum_fx_layout; set colsum OR colsum_fx.  The
     * consumer is seer_groupnorm_apply_fx: one launch, no statistics pass and no finalize pass.  Range: |sum|, sum of squares
     * < 2^43 per (batch element, column). */
    int64_t* colsum_fx;
    int32_t colsum_fx_rows, colsum_fx_reps;
    /* ---- LayerNorm folded into the GEMM that consumes it (BasicTransformerBlock: norm1 -> to_q|k|v, norm2 -> attn2.to_q,
     * norm3 -> ff.net.0, attention.py:198-200, 231-246, 275-277, 308-327).  With W' = gamma (.) W (scaled along K) and
     * x = the UN-normalised rows,  LN(x) W^T = rstd * (x W'^T - mean * wsum) + (beta W^T + b),  wsum[n] = sum_k W'[n][k]:
     * the LayerNorm launch, its read and its write of the activations disappear.
     * Producer side (the GEMM that writes x): rowstat[m][2] += round((sum, sum of squares) of the wave's columns of row m
     * * 2^SEER_LN_FX_SHIFT), 64-bit integer atomic adds like colsum_fx (one pair per row and wave column; integer adds commute:
     * bit-identical from run to run).  ZERO the buffer before the launch.  The sums are taken from the fp32 values the
     * epilogue is about to round to bf16.  Valid when seer_gemm_rowstat_ok(desc). */
    int64_t* rowstat;
    /* Consumer side: A = x [M][K] (K = the normalised width, A2 NULL), W = W', bias = beta W^T + b; ln_rowstat = the producer's
     * rowstat, ln_wsum fp32 [N] (sums of the bf16-ROUNDED W' rows, so that the mean cancels exactly), ln_eps the LayerNorm's
     * epsilon.  The term is applied to the accumulators before bias / GEGLU / rotary / column scale / residual.  Valid when
     * seer_gemm_lnfold_ok(desc) (unsplit tile-kernel launches with a staged bf16 output; a launch AUTO would give to the
     * weight-stationary kernel says no: LayerNorm + that kernel is the faster pair there). */
    const int64_t* ln_rowstat;
    const float* ln_wsum;
    float ln_eps;
} seer_gemm_desc;
#define SEER_GN_FX_SHIFT 20
#define SEER_LN_FX_SHIFT 24

#define SEER_TILE_AUTO 0
#define SEER_TILE_128x128 1
#define SEER_TILE_64x64 2
#define SEER_TILE_128x64 3
/* LDS-direct (global_load_lds) multi-stage variants: tile _ stages */
#define SEER_TILE_G128x128_2 5
#define SEER_TILE_G128x128_3 6
#define SEER_TILE_G128x64_3 7
#define SEER_TILE_G64x64_3 8
#define SEER_TILE_G64x64_4 9
#define SEER_TILE_G64x64_5 10
#define SEER_TILE_G128x64_4 11
/* 160-wide tiles: N = 320 / 640 (C of the two upper levels) in 2 / 4 column tiles instead of 5 / 10 */
#define SEER_TILE_G128x160_2 12
#define SEER_TILE_G64x160_3 13
/* 8 waves (4 x 2), 256-row tiles */
#define SEER_TILE_G256x128_2 14
#define SEER_TILE_G256x64_3 15
/* 96-row tiles: 24 576 rows (the 32x32 level at CFG batch 2) in 256 row tiles = a whole number of tiles per CU */
#define SEER_TILE_G96x160_2 16
#define SEER_TILE_G96x160_3 17
#define SEER_TILE_G96x128_2 18
/* weight-stationary persistent kernel (gemm_ws.hip): one column panel of W resident in LDS per CU, A streamed through a ring;
 * AUTO picks it for plain GEMMs with K <= 768 and M >= 1024, this value asks for it (falls back to AUTO when not eligible) */
#define SEER_TILE_G256x256_2 21 /* 8 waves, 64x128 wave tiles, 2 x 64 KB stages: the only tile whose FLOPs per LDS-fill byte (128) reach the MFMA roof */
#define SEER_TILE_WS 19
#define SEER_TILE_T256x320 22  /* 8 waves (4 x 2), 64 x 160 wave tiles, 142 FLOP per LDS-fill byte; N % 320 == 0; K slices reduced inside the launch (desc.sync) */
#define SEER_TILE_AUTO_TILED 20   /* AUTO restricted to the tile kernel (A/B runs against the weight-stationary kernel) */
/* AUTO with a LAYOUT-INVARIANT plan: kernel, tile, K slices and reduce pass are a function of mode, stride / upsample, the epilogue
 * flags, N, K, K1 and which optional outputs are asked (colsum / colsum_fx / rowstat / ln_rowstat) -- never of M, n_img, Hin / Win,
 * pointer values, a workspace being handed in, or the device.  An output row is then the same bits whatever other rows the launch
 * holds: its K loop runs the same tile's order, its K slices have the same bounds and are added in slice order.  The plan is a tile
 * launch or the split-K pair, never the weight-stationary or the 256 x 320 kernel (both depend on the device).  A plan with K slices
 * needs desc.workspace of seer_gemm_workspace_bytes(): without it the launch is SEER_EINVAL, not an unsplit launch.  The column sums
 * of a split plan cover fixed row blocks (colsum: 16 rows, colsum_fx: 32), and the four feature queries answer independently of M
 * (seer_gemm_colsum_fx_layout still refuses a rows_per_batch its fixed row block does not divide).  One exception to "no pointer
 * values": whether column sums can be taken from the stored tile reads the 16-byte alignment of C (with ldc and strideC), as under
 * every request, so seer_gemm_colsum_rows / seer_gemm_colsum_fx_layout answer for the alignment they are asked with.
 * Rule table: DESIGN.md. */
#define SEER_TILE_AUTO_INVARIANT 23

int seer_gemm_bf16(const seer_gemm_desc* desc /* host */, void* stream);
/* bytes of workspace the call would use for split-K with this descriptor (0: it will not split) */
int64_t seer_gemm_workspace_bytes(const seer_gemm_desc* desc /* host */);
/* rows per partial of the column sums this exact launch (same tile / splits / workspace fields) would write to desc->colsum,
 * or 0 when it cannot produce them; the buffer is [z][ceil(M / rows)][N][2] floats */
int32_t seer_gemm_colsum_rows(const seer_gemm_desc* desc /* host */);
/* colsum_fx form of this exact launch for tensors of rows_per_batch rows per batch element: returns the rows one partial covers
 * (rows_per_batch must be a multiple; 0: the launch cannot accumulate column sums) and sets *reps = the replica count to
 * allocate and pass as colsum_fx_reps */
int32_t seer_gemm_colsum_fx_layout(const seer_gemm_desc* desc /* host */, int32_t rows_per_batch, int32_t* reps /* host */);
/* 1 when this exact launch can accumulate the row statistics of its output (desc->rowstat), else 0 */
int32_t seer_gemm_rowstat_ok(const seer_gemm_desc* desc /* host */);
/* 1 when this exact launch (ln_rowstat / ln_wsum set) applies the folded LayerNorm, 0 when the caller has to run
 * seer_layernorm and the unfolded weights instead */
int32_t seer_gemm_lnfold_ok(const seer_gemm_desc* desc /* host */);
/* bytes of zeroed counter memory (desc->sync) the call would use to reduce its K slices inside the launch (0: none) */
int64_t seer_gemm_sync_bytes(const seer_gemm_desc* desc /* host */);
/* The launch plan of this exact descriptor (read-only; nothing is launched): out = status (what seer_gemm_bf16 would return
 * before it launches), kernel (SEER_GEMM_KERNEL_*), tile (SEER_TILE_*: the tile instantiation; SEER_TILE_T256x320 on that
 * kernel; under SEER_GEMM_KERNEL_WS the tile that runs should that launch hand back), K slices, reduce pass (SEER_GEMM_REDUCE_*).
 * A negative status -- bad arguments, or a feature (column sums, row statistics, GEGLU) the selected launch cannot carry -- comes
 * with kernel NONE and zeros.  This is the HOST's decision.  Two things happen
 * after it and depend on the device's CU count: the 256 x 320 launch clamps its K slices to the resident workgroups, and the
 * weight-stationary launch may hand back to the tile kernel.  Returns SEER_EINVAL for a NULL argument, else SEER_OK. */
#define SEER_GEMM_KERNEL_NONE 0
#define SEER_GEMM_KERNEL_TILE 1      /* seer_gemm_kernel, one launch */
#define SEER_GEMM_KERNEL_SPLITK 2    /* its split-K form + a reduce pass (desc.workspace) */
#define SEER_GEMM_KERNEL_WS 3        /* weight-stationary (gemm_ws.hip) */
#define SEER_GEMM_KERNEL_T320 4      /* 256 x 320 tile (gemm_t320.hip); K slices reduced inside the launch */
#define SEER_GEMM_REDUCE_NONE 0
#define SEER_GEMM_REDUCE_PLAIN 1
#define SEER_GEMM_REDUCE_COLSUM 2         /* + per-tile column sums (desc.colsum) */
#define SEER_GEMM_REDUCE_COLSUM_FX64 3    /* + accumulated column sums (desc.colsum_fx) on 64-row blocks */
#define SEER_GEMM_REDUCE_COLSUM_FX32 4    /* ... on 32-row blocks */
int seer_gemm_plan(const seer_gemm_desc* desc /* host */, int32_t out[5] /* host */);

/* ---- attention -------------------------------------------------------------------------- */
/* Replaces xformers.ops.memory_efficient_attention as called from CrossAttention
 * (attention.py:622-630: spatial self / text cross, attn_bias None) and from WindowSTempAttention
 * (attention.py:632-703: LowerTriangularMask over window tokens ordered (f, wy, wx)).
 *   O[b, sq, h, :] = softmax_j( scale * <Q[b,sq,h,:], K[b,j,h,:]> (+ causal mask j<=i) ) V[b,j,h,:]
 * Q/K/V/O are addressed as ptr + b*bs + s*ss + h*d (+ element), so they can be column slices of a fused
 * [tokens, 3C] projection output.  window_ws > 0 selects the temporal window form: the batch index runs
 * over (window, b) and sequence position p = (f, wy, wx) maps to token f*H*W + (win_y*ws+wy)*W + win_x*ws+wx
 * (window_partition/window_reverse of attention.py:42-69 folded into the addressing).
 * head_dim in {40, 80, 160} (SeerUNet levels) or 96 (FSTextTransformer, 768 / 8; its attention over frames uses
 * ss = tokens-per-frame rows and bs = one row); bf16 in/out, fp32 softmax statistics and accumulation.
 */
typedef struct seer_attn_desc {
    const void* Q; const void* K; const void* V; void* O;   /* bf16 */
    int64_t q_bs, k_bs, v_bs, o_bs;     /* batch strides (elements) */
    int32_t q_ss, k_ss, v_ss, o_ss;     /* sequence(token) strides (elements) */
    int32_t batch, heads, head_dim;
    int32_t Sq, Sk;
    int32_t causal;
    float scale;
    /* temporal windows (0 = off): K/V hold F frames per batch element, Q/O hold Fq (== F unless frame-sharded) */
    int32_t window_ws, F, H, W;
    int32_t Fq;
    /* causal: key j visible to query i iff j <= i + causal_offset (0 unless the queries are a frame shard whose first
     * query sits at sequence position causal_offset of the key sequence) */
    int32_t causal_offset;
    /* optional (training): fp32 [batch' * heads][Sq] with batch' = batch (x windows); receives log2(sum_j 2^(scale*log2(e)*s_ij))
     * per query, the statistic seer_attn_bwd needs to rebuild the probabilities.  NULL at inference. */
    float* lse;
    /* SEER_ATTN_* flags */
    uint32_t flags;
    /* kernel selection, a descriptor field so that A/B runs need no global state: 0 = auto; 1 = generic kernel, one K|V LDS
     * buffer; 6 = generic kernel, ping-pong buffers; head_dim 40 only: 3 = the d = 40 kernel (fast path with the in-launch
     * fallback; 32 queries per wave), 2 = the same with 64 queries per wave (what 0 picks from four rounds of resident workgroups
     * up), 5 = the kernel running its tracked-reference form directly (what lse != NULL selects), 7 = the 64-query form on a
     * three-stage K|V ring in LDS (Sq % 256 == 0, Sk % 128 == 0, not causal, not windowed: what 0 picks for such launches) */
    int32_t variant;
    /* head strides (elements): head h of Q / K / V starts h * q_hs / k_hs / v_hs elements after the batch element's base.
     * 0 = head_dim: the heads are adjacent column groups of token-major rows (the layout of a fused [tokens, 3C] projection).
     * A HEAD-MAJOR operand -- [batch][head][token][head_dim], token stride = head_dim, head stride = tokens * head_dim, what
     * seer_gemm_bf16 writes with SEER_EPI_HEADMAJOR -- makes every K / V tile of a head one dense run of memory: at head_dim 40
     * the LDS-DMA of a 128-key tile then moves 80 whole 128-byte lines instead of ~200 partial ones (80-byte pieces at a
     * 1920-byte pitch), which is what bounds the d = 40 kernel on token-major operands.  O is always token-major. */
    int64_t q_hs, k_hs, v_hs;
} seer_attn_desc;

/* Q already holds q * scale * log2(e) (the producing GEMM's epilogue multiplied it in, SEER_EPI_COLSCALE): the kernel takes
 * exp2 of the raw dot products and ignores `scale`.  Without the flag the d = 40 kernel multiplies Q itself (one more
 * bf16 rounding of q) and the generic kernel scales the fp32 scores. */
#define SEER_ATTN_Q_PRESCALED 1u
/* Q, K, V and O hold IEEE half (fp16) instead of bf16 -- the UNet engine under fp16 autocast (every reference yaml ships
 * mixed_precision: "fp16").  fp32 scores, statistics and accumulation as always; P is rounded to fp16 for the PV product.  head_dim 40
 * from 256 keys up runs the d = 40 kernel's TRACKED form (its fast path needs bf16's exponent range), everything else the generic
 * kernel (variant 0, 1 or 5; no lse: inference only). */
#define SEER_ATTN_F16 2u

int seer_attn_fwd(const seer_attn_desc* desc /* host */, void* stream);

/* ---- CLIP text tower (transformers CLIPTextModel, text_encoder of runwayml/stable-diffusion-v1-5; train.py:330-334,
 * inference_img.py:147-161) -- the two pieces next to seer_gemm_bf16 / seer_layernorm ------------------------------------------ */
/* Causal self-attention with a key padding mask over short sequences, head_dim 64 (CLIPAttention with the causal mask and
 * `attention_mask` of CLIPTextTransformer.forward):
 *   O[b*L + i][64 h + :] = sum_j softmax_j( <Q[b*L + i][64 h + :], K[b*L + j][64 h + :]> ) V[b*L + j][64 h + :]
 * over the keys j that are VISIBLE to query i of sample b:  j <= i  and  key_mask[b][j] != 0.
 * Q, K, V: bf16 column slices of ONE fused [batch * L][>= 3 * heads * 64] projection -- the same row stride ld_qkv (elements, a
 * multiple of 8), heads are adjacent 64-column groups, pointers 16-byte aligned.  O: bf16 token-major [batch * L][ldo], ldo a multiple
 * of 4, 8-byte aligned.  key_mask: uint8 [batch][L], or NULL = every key visible.  1 <= L <= 128, any heads.
 * Q ARRIVES PRESCALED by scale * log2(e) (scale = 64^-0.5) from the producing GEMM's SEER_EPI_COLSCALE, the convention of
 * SEER_ATTN_Q_PRESCALED: the kernel takes exp2 of the raw dot products.  fp32 scores and statistics, P rounded to bf16 for the PV
 * product, v_mfma_f32_16x16x32_bf16 for both products; one pass (a 16-query tile sees all its keys at once: no online rescaling).
 * A query WITHOUT a visible key (a mask that hides key 0 .. i) writes ZEROS, never NaN or inf.  transformers leaves such a row to
 * the softmax of a row of equal minima (a uniform average, or NaN, by version): outside its contract; here it is defined, so a host
 * never has to synchronise to validate a mask.
 * SEER_EINVAL: a NULL / misaligned pointer, a stride below heads * 64 or off its multiple, batch, heads or L < 1.  SEER_ENOSYS:
 * L > 128 (not built).  Both are decided before any launch. */
int seer_attn_causal64(const void* Q, const void* K, const void* V, int32_t ld_qkv, void* O, int32_t ldo, const uint8_t* key_mask,
                       int32_t batch, int32_t heads, int32_t L, void* stream);
/* CLIPTextEmbeddings: x[b*L + l][:] = tok[ids[b][l]][:] + pos[l][:], summed in fp32, stored as bf16 [batch * L][ldx].  ids int64
 * [batch][L] on the DEVICE; tok bf16 [vocab][C], pos bf16 [L_max][C], C % 8 == 0, L <= L_max, ldx >= C and a multiple of 8, pointers
 * 16-byte aligned.  An id outside [0, vocab - 1] is CLAMPED into it inside the kernel: no id can read out of bounds (hosts that want
 * an error check their ids before the upload). */
int seer_embed_tokens(const int64_t* ids, int32_t batch, int32_t L, const void* tok, int32_t vocab, const void* pos, int32_t L_max,
                      int32_t C, void* x, int32_t ldx, void* stream);

/* Backward of the call above (the training step, train.py:380-381 through attention.py:622-630 / 632-703):
 * given dO, writes dQ, dK, dV (bf16, addressed like Q/K/V with their own strides, so they can be the column slices of one
 * [tokens, 3C] gradient buffer that feeds a single dX GEMM).  fwd must be the descriptor of the forward call with O and
 * lse filled in by it; delta is a [batch' * heads][Sq] fp32 scratch (<dO, O> per query).  Frame-sharded queries (Fq != F)
 * are not supported.  Deterministic: two launches (dQ; dK|dV), no atomics. */
typedef struct seer_attn_bwd_desc {
    seer_attn_desc fwd;
    const void* dO; void* dQ; void* dK; void* dV;     /* bf16 */
    int64_t do_bs, dq_bs, dk_bs, dv_bs;
    int32_t do_ss, dq_ss, dk_ss, dv_ss;
    float* delta;
} seer_attn_bwd_desc;
int seer_attn_bwd(const seer_attn_bwd_desc* desc /* host */, void* stream);

/* Rotary embedding on q and k in place (rotary-embedding-torch 0.1.5 rotate_queries_or_keys as called at
 * attention.py:649-651): first rot_dim channels of every head, interleaved pairs (x0,x1) -> (x0 c - x1 s, x1 c + x0 s),
 * angle = fp32(pos) * freqs[j] with freqs the module's `rotary_emb.freqs` buffer (10000^(-2j/rot_dim)),
 * pos = token index inside its batch element (f*H*W + y*W + x) + pos_offset (pos_offset = first frame * H*W under
 * frame sharding).  seer_rotary_table fills cos_sin fp32 [T][half][2] once per (level, F); seer_rotary_inplace
 * rotates x: bf16 [rows, ld] where head h of q occupies columns [col0_q + h*head_dim, ...) and of k [col0_k + ...). */
int seer_rotary_table(const float* freqs, int32_t T, int32_t half, float* cos_sin, void* stream);
int seer_rotary_inplace(void* x, int64_t rows, int32_t ld, int32_t col0_q, int32_t col0_k, int32_t heads,
                        int32_t head_dim, int32_t rot_dim, int32_t tokens_per_batch, int32_t pos_offset,
                        const float* cos_sin, void* stream);

/* ---- normalisation ---------------------------------------------------------------------- */
/* GroupNorm over (C/G, F, H, W) per (b, g) on channels-last data -- torch.nn.GroupNorm applied to the 5-D
 * tensor (resnet.py:179,197; attention.py:133; unet_3d_condition.py:368).  Two sources = channel concat.
 * stats: writes (sum, sumsq) per (b, g) to stats[b][g][2] (fp32).  Deterministic: per-block partials go to `workspace`
 * (seer_groupnorm_workspace_floats(...) floats) and are added in block order -- no float atomics, so two runs, or two
 * identical batch elements, give bit-identical statistics.  Under frame sharding the caller all-reduces `stats`
 * between the two calls.
 * apply: y = (x-mean)*rstd*gamma+beta, optional SiLU, bf16 out [rows, C1+C2]; count = elements per group over
 * ALL shards (so mean = sum/count). */
int64_t seer_groupnorm_workspace_floats(int32_t C, int32_t batch, int64_t rows_per_batch, int32_t groups);
int seer_groupnorm_stats(const void* x1, int32_t C1, const void* x2, int32_t C2, int32_t batch,
                         int64_t rows_per_batch, int32_t groups, float* stats, float* workspace, int32_t dtype, void* stream);
/* The same stats[b][g][2] from the column sums the producers of x1 / x2 left behind (seer_gemm_desc::colsum) -- no pass over
 * the activations.  Source i: C_i channels, partial rows [phases_i][tiles_i][C_i][2]; the tiles of a phase cover the batch
 * elements in order, tiles_i / batch each (tiles_i % batch == 0).  One wave per (b, g) adds its channels' partials in a fixed
 * order: deterministic; equal to seer_groupnorm_stats up to the fp32 order of additions. */
int seer_groupnorm_stats_from_colsums(const float* cs1, int32_t C1, int32_t phases1, int32_t tiles1, const float* cs2,
                                      int32_t C2, int32_t phases2, int32_t tiles2, int32_t batch, int32_t groups,
                                      float* stats, void* stream);
int seer_groupnorm_apply(const void* x1, int32_t C1, const void* x2, int32_t C2, int32_t batch,
                         int64_t rows_per_batch, int32_t groups, const float* stats, double count, float eps,
                         const float* gamma, const float* beta, int32_t silu, void* y, int32_t dtype, void* stream);
/* seer_groupnorm_stats_from_colsums + seer_groupnorm_apply in ONE launch: every block re-derives the statistics of the groups it
 * normalises from the producers' column sums (same arguments as the two calls).  Single-process runs only: a
 * frame-sharded run has to all-reduce the statistics between the two steps and keeps the two calls.  SEER_ENOSYS when the
 * channel layout does not slice into whole groups of 64..128 channels (the caller then makes the two calls). */
int seer_groupnorm_apply_from_colsums(const void* x1, int32_t C1, const void* x2, int32_t C2, const float* cs1, int32_t phases1,
                                      int32_t tiles1, const float* cs2, int32_t phases2, int32_t tiles2, int32_t batch,
                                      int64_t rows_per_batch, int32_t groups, double count, float eps, const float* gamma,
                                      const float* beta, int32_t silu, void* y, int32_t dtype, void* stream);
/* GroupNorm apply whose statistics are the fixed-point column sums the producers ACCUMULATED (seer_gemm_desc::colsum_fx):
 * fx1 [reps1][batch][2][C1], fx2 [reps2][batch][2][C2] int64 (NULL with C2 = 0).  One launch per GroupNorm; every block converts the sums of
 * the groups it normalises (double precision) and streams its rows.  stats_out (or NULL): receives (sum, sum of squares) per
 * (batch element, group) as fp32 [batch][groups][2], what seer_groupnorm_bwd takes.  SEER_ENOSYS as above. */
int seer_groupnorm_apply_fx(const void* x1, int32_t C1, const void* x2, int32_t C2, const int64_t* fx1, int32_t reps1,
                            const int64_t* fx2, int32_t reps2, int32_t batch, int64_t rows_per_batch, int32_t groups, double count, float eps, const float* gamma,
                            const float* beta, int32_t silu, void* y, float* stats_out, int32_t dtype, void* stream);
/* The same accumulated sums from the ACTIVATIONS: fx [batch][2][C] int64 (one replica; ADDED to: zero it first) receives
 * sum_r round(x[r][c] * 2^20) and sum_r round(x[r][c]^2 * 2^20) over the rows of each batch element.  Every element is rounded on
 * its own, so the totals are exact integer sums: independent of the order of the additions and -- frame shards -- of which rank
 * held which rows (an int64 all-reduce of the shards' sums IS the unsharded result).  The statistics pass of a frame-sharded step
 * for GroupNorm sources without accumulated producer sums (resnet.py:179,197, attention.py:133 normalise over all frames). */
int seer_groupnorm_stats_fx(const void* x, int32_t C, int32_t batch, int64_t rows_per_batch, int64_t* fx, int32_t dtype,
                            void* stream);
/* FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net", CVPR 2024; diffusers' apply_freeu / fourier_filter with threshold 1) on a
 * decoder resnet's two inputs in front of their channel concat, ONE launch (csrc/freeu.hip).  Token-major activations of `images`
 * images of H x W pixels, rows = images * H * W, 16-bit storage type `dtype`, fp32 arithmetic for either type (diffusers runs a
 * half-precision FFT on fp16 power-of-two planes: a stated difference):
 *   backbone  x [rows][Cx] -> x_out:  x_out[r][c] = rnd(x[r][c] * b) for c < Cx / 2, the bits of x[r][c] for the other channels;
 *   skip      skip [rows][Cs] -> skip_out, per (image, channel) over that image's H x W plane:
 *                 skip_out[h][w] = rnd(skip[h][w] + (s - 1) / (H W) * sum_{kh in K_H, kw in K_W} Re(X[kh][kw] e^{+2 pi i (kh h / H + kw w / W)}))
 *                 X[kh][kw]      = sum_{h, w} skip[h][w] e^{-2 pi i (kh h / H + kw w / W)}
 *             K_N = the distinct values of {0, -1 mod N} ({0} for N = 1, {0, 1} for N = 2): Re ifft2(mask * fft2(skip)) with the mask
 *             s on the fft-shifted block [H/2 - 1 : H/2 + 1, W/2 - 1 : W/2 + 1] and 1 elsewhere.
 * Either pair may be NULL (both pointers): the other half runs alone, with the bits it has in the joint launch.
 *   params    fp32 [2] = (b, s), DEVICE memory, read by the kernel: a captured launch follows a change of the values.
 *   twiddles  fp32 [2][2 H + 2 W]: row 0 = cos(2 pi h / H) (H values), sin(2 pi h / H), cos(2 pi w / W) (W values), sin(2 pi w / W) of
 *             the caller's float64 table (exact 0 / +-1 at the multiples of a quarter turn) rounded to fp32, row 1 = what that
 *             rounding left (float64 value - row 0, as fp32); the kernel evaluates no sin or cos.
 * The skip half runs in two-float arithmetic (a value = hi + lo of two fp32 numbers, error-free sums and products): a correction kept
 * in one fp32 number is too coarse for fp16 storage where skip and correction cancel.  The result is rounded to fp32 once and then to
 * the storage type.
 * A workgroup owns an image and 512 channels, a thread 8 channels, a wave every fourth row.  Order of summation of a coefficient, per
 * channel: the pixels of a row left to right (compensated: the sum and the sum of its rounding errors), the wave's rows top to bottom,
 * the four waves' partials in wave order (through LDS; no atomics).  An element's bits depend on its own (image, channel) plane, H, W,
 * the table and the scalars only.
 * x_out == x (in place, the same address) is allowed; the skip is read twice and skip_out must not overlap it.
 * SEER_EINVAL, nothing launched: both pairs NULL, or half a pair; an output that overlaps an input of the other pair, the other
 * output, or its own input other than x_out == x; images, H or W < 1; rows != images * H * W; Cx or Cs not a positive multiple of 8;
 * an activation pointer off 16 bytes, params or twiddles NULL or off 4 bytes; more than 65535 channel slices. */
int seer_freeu(const void* x, void* x_out, int32_t Cx, const void* skip, void* skip_out, int32_t Cs, int64_t rows, int32_t images,
               int32_t H, int32_t W, const float* params, const float* twiddles, int32_t dtype, void* stream);
/* Step caching (DeepCache, Ma et al., CVPR 2024; TaylorSeer, Liu et al., 2025; csrc/step_cache.hip): the feature that enters the
 * shallowest decoder layers of the UNet, kept over the last three full evaluations and forecast on the evaluations between them.
 *   ring      three slots of n elements of the 16-bit storage type `dtype`, slot_stride elements apart; slot 0 is the newest.
 * seer_cache_push:      slot2 <- slot1, slot1 <- slot0, slot0 <- x (n elements).  A thread reads its elements of all three sources
 *                       before it writes; values move as bits (NaN payloads included: a slot that was never written may hold anything),
 *                       so one kernel serves both storage types.  x is not written.
 * seer_cache_forecast:  out[i] = rnd(fmaf(w2, f2[i], fmaf(w1, f1[i], w0 * f0[i]))), f_k = slot k; fp32 arithmetic in exactly this order,
 *                       ONE round-to-nearest-even conversion to the storage type.
 *   w         fp32 [3], DEVICE memory, read by the kernel: the launch is a node of a captured graph whose arguments are frozen.
 *             A slot whose weight is exactly 0 is NOT READ and its term is left out (for slot 0 the sum starts from +0): it may hold
 *             NaN.  So w = (1, 0, 0) returns the finite values of slot 0 bit for bit.
 * Flat and memory bound: 16-byte accesses (8 elements per thread), the n % 8 elements of the tail by one thread, no LDS, no atomics.
 * SEER_EINVAL, nothing launched: a NULL pointer; n < 1; slot_stride < n; slot_stride no multiple of 8 (a slot would leave 16-byte
 * alignment); x, ring or out off 16 bytes, w off 4 bytes; x or out overlapping the ring's 2 * slot_stride + n elements; a dtype other
 * than SEER_DT_BF16 / SEER_DT_F16. */
int seer_cache_push(const void* x, void* ring, int64_t n, int64_t slot_stride, int32_t dtype, void* stream);
int seer_cache_forecast(const void* ring, int64_t n, int64_t slot_stride, const float* w, void* out, int32_t dtype, void* stream);
/* The feed-forward of a transformer block at the 320-channel level and the transformer's proj_out, ONE launch (csrc/ff_fused.hip):
 *     y = x + [Wp | Wp W2] [h | g] + bcat,   g = GEGLU(LayerNorm(h; gamma, beta, eps) W1^T + b1)
 * i.e. norm3 -> ff.net.0 -> ff.net.2 + residual -> proj_out + residual (seer/models/attention.py:231-248, 308-327, 742-747,
 * 783-793, 126, 141-145).  h, x, y: [M][320] bf16 with row strides ldh, ldx, ldy (elements, multiples of 8; y may alias x);
 * a workgroup owns 96 rows (the last one fewer when M is not a multiple).  w1f, wcf: the two weight matrices in the kernel's FRAGMENT order, made once by the pack entry points below from
 * w1 [2560][320] bf16 (interleaved GEGLU row order: 16 value rows, 16 gate rows, ...) and wcat [320][1600] bf16 = [Wp | Wp W2];
 * b1 [2560] fp32 in the same interleaved order; bcat [320] fp32 = Wp b2 + bp.  colsum_fx (or NULL): [fx_reps][M / fx_rows][2][320]
 * int64, ADDED to, the fixed-point column sums of y as seer_gemm_desc::colsum_fx (fx_rows = rows per batch element, a multiple of
 * 16 and at least 96: a tile may straddle two batch elements).  colsum_tiles (or NULL; M a multiple of 96): [M / 96][320][2] fp32,
 * WRITTEN, (sum, sum of squares) of the stored values per 96-row tile as seer_gemm_desc::colsum.  All pointers 16-byte aligned.  SEER_EINVAL otherwise.
 * The optional prologue: with a != NULL the rows the launch reads as h are  h + a Wo^T + bo  -- the attention's to_out projection and its
 * residual (seer/models/attention.py:237-240, 316-322), computed in the tile and stored nowhere (this launch is their only reader).
 * a [M][320] (row stride lda), wof = Wo [320][320] in the fragment order of seer_rowchain_pack, bo [320] fp32; a == NULL: no prologue
 * (lda, wof, bo ignored).  h, x, y, a and the packed weight matrices are in the storage type `dtype` (the pack entry points move
 * 16-bit words and serve both). */
int seer_ff_fused_c320(const void* a, int32_t lda, const void* wof, const float* bo, const void* h, int32_t ldh, const void* x,
                       int32_t ldx, void* y, int32_t ldy, int64_t M, const float* gamma, const float* beta, float eps,
                       const void* w1f, const float* b1, const void* wcf, const float* bcat, int64_t* colsum_fx, int64_t fx_rows,
                       int32_t fx_reps, float* colsum_tiles, int32_t dtype, void* stream);
/* The row-local chains in front of the attention launches of a transformer block at the 320-channel level, ONE launch (csrc/rowchain.hip):
 *     h   = [GroupNorm(inp)] W1^T + b1 [+ res]                         (stored when h != NULL)
 *     out = LayerNorm(h; ln_gamma, ln_beta, ln_eps) [W2_0 | ... ]^T     n2 = 1..3 thirds of 320 columns (skipped when w2f == NULL)
 * GroupNorm -> proj_in -> norm1 -> to_q | to_k | to_v (seer/models/attention.py:129-145, 231-240, 308-318; the temporal block's rotary
 * embedding :649-651 as rot_*), or attn1.to_out + residual -> norm2 -> attn2.to_q (:316-322).  inp, res, h [M][320], out [M][n2 * 320]
 * in the storage type `dtype` (SEER_DT_*), row strides multiples of 8 elements, h may alias res.  GroupNorm: gn_stats [batch][groups][2]
 * fp32 (sum, sum of squares per (batch element, group): what seer_groupnorm_stats* write), gn_count elements per group, rows_per_batch
 * >= 96 (SEER_ENOSYS otherwise: a workgroup's 96 rows span at most two batch elements); NULL = no normalisation of
 * the input; or gn_fx [gn_fx_reps][batch][2][320] int64, the fixed-point column sums the producer of `inp` ACCUMULATED
 * (seer_gemm_desc::colsum_fx): no statistics launch in front.  ln_gamma / ln_beta NULL = no LayerNorm.  w1f / w2f: the matrices in FRAGMENT order (seer_rowchain_pack).  The first
 * rot_thirds thirds are rotated like SEER_EPI_ROTARY (table of seer_rotary_table, position = row % rot_tokens_per_batch +
 * rot_pos_offset, heads of rot_head_dim channels, the first rot_dim rotated), then the first scale_thirds thirds are multiplied by
 * col_scale (the q columns leave as q * scale * log2(e) for SEER_ATTN_Q_PRESCALED).  All pointers 16-byte aligned. */
typedef struct seer_rowchain_desc {
    const void* inp; int32_t ld_in;
    const float* gn_stats; const int64_t* gn_fx; int32_t gn_fx_reps;
    double gn_count; float gn_eps; const float* gn_gamma; const float* gn_beta; int64_t rows_per_batch; int32_t groups;
    const void* w1f; const float* b1; const void* res; int32_t ldr; void* h; int32_t ldh;
    const float* ln_gamma; const float* ln_beta; float ln_eps;
    const void* w2f; int32_t n2; void* out; int32_t ldo;
    float col_scale; int32_t scale_thirds;
    const float* rot_table; int32_t rot_tokens_per_batch, rot_pos_offset, rot_head_dim, rot_dim, rot_thirds;
    int64_t M;
    int32_t dtype;
} seer_rowchain_desc;
int seer_rowchain_c320(const seer_rowchain_desc* desc /* host */, void* stream);
/* n_mats 320 x 320 matrices -- rows 320 t .. 320 t + 319 of W [n_mats * 320][ld], 16-bit elements -- into the kernel's fragment order:
 * out[t][K step 5][wave 4][k32 2][column fragment 5][lane 64][8], element W[320 t + 80 w + 16 j + (lane & 15)][64 s + 32 k32 + 8 (lane >> 4) + e] */
int seer_rowchain_pack(const void* W, int32_t ld, int32_t n_mats, void* out, void* stream);
/* w1 [2560][320] bf16 -> out (same size): [chunk 20][wave 4][K step 5][k32 2][value | gate][lane 64][8 bf16], element
 * w1[128 c + 32 w + 16 f + (lane & 15)][64 ks + 32 k32 + 8 (lane >> 4) + e]: every fragment load of the kernel is one contiguous KiB */
int seer_ff_fused_pack_w1(const void* w1, void* out, void* stream);
/* wcat [320][1600] bf16 -> out (same size): [K step 25][wave 4][k32 2][column fragment 5][lane 64][8 bf16], element
 * wcat[80 w + 16 j + (lane & 15)][64 s + 32 k32 + 8 (lane >> 4) + e] */
int seer_ff_fused_pack_wcat(const void* wcat, void* out, void* stream);
/* nn.LayerNorm(C) per token row (attention.py:198-200,275-277), eps 1e-5; bf16 in/out, fp32 statistics. */
int seer_layernorm(const void* x, int64_t rows, int32_t C, int32_t ldx, const float* gamma, const float* beta,
                   float eps, void* y, int32_t ldy, int32_t dtype, void* stream);

/* y = softmax(scale * x) over rows of a [rows, n] matrix, x bf16 or fp32, y bf16 (VAE mid attention,
 * ldm/modules/diffusionmodules/model.py:186-197) */
int seer_softmax_rows(const void* x, int32_t x_is_f32, int64_t rows, int32_t n, int32_t ld, float scale, void* y,
                      int32_t ldy, int32_t dtype, void* stream);

/* ---- small / boundary kernels ----------------------------------------------------------- */
/* diffusers Timesteps(320, flip_sin_to_cos, freq_shift) (unet_3d_condition.py:97,307): out[b] = [cos | sin](t*f_i)
 * (or [sin|cos] when flip==0), fp32 [B, dim]. t: int64 [B]. */
int seer_timestep_embedding(const int64_t* t, int32_t B, int32_t dim, int32_t flip_sin_to_cos, float freq_shift,
                            float* out, void* stream);

/* small-M linear: y[b, n] = act( sum_k f(x[b,k]) * W[n,k] + bias[n] ), f = SiLU if silu_in.  x fp32 [B,K], W bf16 [N][K],
 * y fp32.  Used for time_embedding (unet_3d_condition.py:308) and all 22 time_emb_proj at once (resnet.py:192). */
int seer_linear_smallm(const float* x, int32_t B, int32_t K, const void* W, const float* bias, int32_t N,
                       int32_t silu_in, int32_t silu_out, float* y, int32_t dtype, void* stream);

/* conv_in: InflatedConv3d(4->C0, 3x3, pad 1) reading the reference layout [B, Cin, F, H, W] fp32 and writing
 * channels-last bf16 [B*F, H*W, C0] (unet_3d_condition.py:94,311; the VAE's conv_in, ldm/modules/diffusionmodules/model.py:487-491).
 * W fp32 repacked to [3][3][Cin][C0]. */
int seer_conv_in(const float* x, int32_t B, int32_t Cin, int32_t F, int32_t H, int32_t W_, const float* Wt,
                 const float* bias, int32_t Cout, void* y, int32_t dtype, void* stream);
/* conv_out: InflatedConv3d(C0->Cout(4), 3x3, pad 1) reading channels-last bf16 and writing [B, Cout, F, H, W] fp32
 * (unet_3d_condition.py:205,370; the VAE's conv_out, model.py:556-568).  W fp32 [Cout][3][3][C0].  Cout 3 or 4 for SEER_DT_BF16,
 * 3 for SEER_DT_F16 (SEER_ENOSYS otherwise). */
int seer_conv_out(const void* x, int32_t B, int32_t C0, int32_t F, int32_t H, int32_t W_, const float* Wt,
                  const float* bias, int32_t Cout, float* y, int32_t dtype, void* stream);

/* pointwise channel mix on NCHW fp32: the VAE's post_quant_conv (1x1, 4->4; ldm/models/autoencoder.py:330-333).
 * W fp32 [Cout][Cin]. */
int seer_conv1x1_nchw_f32(const float* x, int32_t N, int32_t Cin, int32_t Cout, int32_t HW, const float* Wt,
                          const float* bias, float* y, void* stream);

/* layout / dtype conversion: fp32 [rows, C] -> bf16 (context, weights) */
int seer_cast_f32(const float* x, int64_t n, void* y, int32_t dtype, void* stream);
/* NHWC bf16 -> NCHW fp32 and back (VAE boundary) */
int seer_nchw_f32_to_nhwc_bf16(const float* x, int32_t N, int32_t C, int32_t HW, void* y, void* stream);
int seer_nhwc_bf16_to_nchw_f32(const void* x, int32_t N, int32_t C, int32_t HW, float* y, void* stream);

/* ---- sampler step ------------------------------------------------------------------------ */
/* One export per kernel: a step kernel's mode is read from which of its pointers are set, each mode keeps its own checks, and a
 * half-set mode is SEER_EINVAL, never a silent switch.  The schedule index has exactly one source:
 *   host form    step == NULL and index >= 0;
 *   device form  step != NULL and index == SEER_INDEX_FROM_STEP: the index is step[1], for a step that is captured WHOLE in one
 *                hipGraph (kernel arguments are frozen at capture, the step counter must not be).  step: int32[2] in device memory;
 *                step[0] = index of the next step to run, step[1] = index of the step in flight.
 * Any other combination is refused, so a forgotten `step` does not run as row 0 from the host.  (seer_known_blend, below, keeps its
 * older rule: `step` when set, `index` otherwise.) */
#define SEER_INDEX_FROM_STEP (-1)

/* CFG combine + DDIM update of DDIMSampler.p_sample_ddim (ldm/models/diffusion/ddim_video.py:209-238), fp32:
 *   e   = e_uc + scale*(e_c - e_uc)            (only frames >= cond_f of the UNet output are used)
 *   x0  = (x - sqrt(1-a_t) e)/sqrt(a_t)
 *   x'  = sqrt(a_prev) x0 + sqrt(1-a_prev-sigma^2) e + sigma*noise
 * eps: UNet output [2b (uc then c), C, F_total, HW] fp32 (or [b,...] with scale==1 / e_uc NULL semantics:
 * pass cfg=0); x, x_prev, pred_x0: [b, C, F_pred, HW].  coef: device fp32 [steps][4] = (a_t, a_prev, sigma, sqrt(1-a_t)),
 * row `index` is used (no host->device scalar copies per step, unlike ddim_video.py:219-222).  x_prev may be x; pred_x0 may be NULL.
 *   index source  host form, or device form: the last kernel of a captured step, which then writes step[0] = index - 1.  A counter
 *                 that ran past the schedule's end, step[1] < 0 (a replay after the chain's last step), still gives step[0] =
 *                 index - 1, but reads no coefficient row and writes no element of x_prev or pred_x0.
 *   noise source  at most one of `noise` (a tensor shaped like x; NULL when sigma == 0) and `seeds` ("seeded noise" below, which
 *                 alone reads `temperature`, bounds the clip and asks for aligned pointers); both set is SEER_EINVAL.
 * seer_ddim_step_begin (ddim_video.py:189,201-203) is the first kernel of a captured step: sample[reps*b, C, f1 + F_pred, HW] =
 * cat([x0_emb, x], frames) repeated `reps` times (2 = the [uc, c] CFG pair), t_out[reps*b] = t_table[step[0]], and step[1] = step[0].
 * No kernel reads and writes the same word, so replays of the captured step walk the schedule downwards on their own; the host
 * writes step[0] only to start a chain. */
int seer_cfg_ddim_step(const float* eps, int32_t cfg, int32_t b, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW, float scale,
                       const float* coef, int32_t index, int32_t* step, const float* x, const float* noise, const uint32_t* seeds,
                       float temperature, float* x_prev, float* pred_x0, void* stream);
int seer_ddim_step_begin(const float* x0_emb /* NULL iff f1 == 0 */, const float* x, int32_t b, int32_t reps, int32_t C,
                         int32_t f1, int32_t F_pred, int32_t HW, const int64_t* t_table, int32_t* step, float* sample,
                         int64_t* t_out, void* stream);

/* The captured step over SLOTS (continuous batching, seervideoldm_amd/slots.py): the two kernels above with `slots` in the place of
 * b and everything a replay must not freeze held per slot in device memory.  Row r of a [reps*slots, ...] tensor belongs to slot
 * r % slots (uc rows, then c rows).  step: int32 [slots][2], the pair of seer_ddim_step_begin per slot; t_table: int64
 * [slots][nsched]; coef: fp32 [slots][nsched][4]; scale: fp32 [slots], device memory.
 *   seer_slot_step_begin     for every slot s: index = step[s][0], then step[s][1] = index; the sample rows of slot s =
 *                            cat([x0_emb[s], x[s]], frames), `reps` (1 or 2) times; t_out[rep*slots + s] = t_table[s][max(index, 0)].
 *                            An idle slot (index < 0) gets finite rows as long as its x / x0_emb are (the host zeroes them).
 *                            x_prov and state are NULL both, or set both: a sampler per slot, "a SAMPLER per slot" below.
 *   seer_slot_cfg_ddim_step  for every slot s: index = step[s][1].  index >= 0: the update of seer_cfg_ddim_step with cfg = 1,
 *                            scale[s] and row `index` of coef[s] -- the same device code, so an element gets the bits
 *                            seer_cfg_ddim_step gives it -- then step[s][0] = index - 1.  index < 0 (or >= nsched, which no
 *                            schedule produces): nothing of that slot is written, neither x_prev nor pred_x0 nor step.
 *                            seeds and temperature are NULL both (eta = 0, no noise term) or set both ("seeded noise" below).
 *                            x_prev may be x; pred_x0 may be NULL.
 * No kernel reads and writes the same word: replays walk every slot's schedule with no host-written scalar; the host writes
 * step[s][0] only when it fills slot s.  Every pointer must be 4-byte aligned and no more (the int64 tables move as 32-bit words);
 * SEER_EINVAL otherwise, and for slots < 1, nsched < 1, reps outside {1, 2}, cond_f >= F_total, a NULL required pointer, one of a
 * pointer pair without the other. */
int seer_slot_step_begin(const float* x0_emb /* NULL iff f1 == 0 */, const float* x, const float* x_prov /* NULL with state */,
                         int32_t slots, int32_t reps, int32_t C, int32_t f1, int32_t F_pred, int32_t HW, const int64_t* t_table,
                         int32_t nsched, int32_t* step, int32_t* state /* NULL: no sampler per slot */, float* sample, int64_t* t_out,
                         void* stream);
int seer_slot_cfg_ddim_step(const float* eps, int32_t slots, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                            const float* scale, const float* coef, int32_t nsched, int32_t* step, const float* x,
                            const uint32_t* seeds /* NULL: eta = 0 */, const float* temperature /* NULL with seeds */, float* x_prev,
                            float* pred_x0, void* stream);

/* DDIM inversion (CompVis ldm/models/diffusion/ddim.py, encode(); eta = 0 by definition): the same CFG combine, then the update one
 * step UPWARD, fp32.  x is the latent at the level of a_prev, eps the model's output at the timestep of a_t:
 *   x0     = (x - sqrt(1-a_prev) e)/sqrt(a_prev)
 *   x_next = sqrt(a_t) x0 + sqrt(1-a_t) e          (sqrt(1-a_t) = column 3 of the row; sigma, column 2, is not read)
 * eps, coef and the shapes as in seer_cfg_ddim_step; x_next may be x; pred_x0 (= x0) may be NULL: it is then not written.
 *   host form    row `index` of coef; limit is NULL.
 *   device form  last kernel of a captured inversion step behind seer_ddim_step_begin: index = step[1], then step[0] = index + 1 --
 *                replays walk the schedule upwards.  limit: int32[1] in DEVICE memory, the number of rows the chain may use (the
 *                arguments of a replay are frozen, and the rows of a static table beyond the schedule hold a_prev = 0, which the
 *                update divides by).  For index < 0 or index >= limit[0] step[0] is written all the same, but no coefficient row is
 *                read and no element of x_next or pred_x0 written; limit[0] = 0 makes a launch write nothing but that word.
 * No kernel reads and writes the same word.  SEER_EINVAL for a NULL required pointer (eps, coef, x, x_next), an index source that
 * is neither form, limit without step or step without limit, b <= 0, non-positive extents, cond_f < 0 or >= F_total, a pointer
 * that is not 4-byte aligned, a grid beyond one dimension. */
int seer_cfg_ddim_invert_step(const float* eps, int32_t cfg, int32_t b, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                              float scale, const float* coef, int32_t index, int32_t* step, const int32_t* limit, const float* x,
                              float* x_next, float* pred_x0 /* NULL: not written */, void* stream);

/* ---- seeded noise: the DDIM step with eta > 0 and no noise tensor ------------------------------------------------------------
 * A counter-based generator, Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85), runs
 * inside the kernels: a clip's noise is a pure function of (seed, schedule index, element), whatever batch row or slot holds it.
 *   key      (seed & 0xffffffff, seed >> 32), one uint64 seed per clip; in device memory uint32 [rows][2] = (lo, hi), 4-byte aligned
 *   counter  (block, index, stream, 0); block = e >> 2 with e the element's linear index inside the clip's own [C, F_pred, HW]
 *            latent, and element e takes normal e & 3 of its block.  stream 0 = the start code (index 0), stream 1 = the noise of
 *            the step at schedule index `index`, stream 2 = the noise that re-noises given latents to the level of schedule index
 *            `index` ("given latents" below), streams >= 3 reserved
 *   uniform  u = float(2 * (w >> 9) + 1) * 2^-24, exact in fp32 and strictly inside (0, 1)
 *   normals  Box-Muller on the word pairs (w0, w1), (w2, w3): r = sqrtf(-2 logf(u_a)), (s, c) = sincospif(2 u_b), n_even = r c,
 *            n_odd = r s; |n| <= 5.7682
 * and the noise term of the update is sigma * (temperature * n), two rounded fp32 products.
 *   seer_philox_u32     diagnostic: out[4 (j - first_block) ..] = the four words of block j for first_block <= j < first_block +
 *                       n_blocks <= 2^32.  Its `stream` is 64 bits wide -- low word = counter word 2, high word = counter word 3 -- so
 *                       that any counter can be asked for; the samplers' streams have a zero high word.
 *   seer_philox_normal  out[0 .. n-1] = the first n normals of (seed, stream, index), 0 < n < 2^31; nothing is written past
 *                       out[n-1].  The start code of a seeded clip is stream 0, index 0.
 *   seer_cfg_ddim_step with `seeds` (one pair per batch row) and `temperature`, `noise` NULL
 *                       where row `index` of coef has sigma != 0, element e of row bi gets stream-1 noise of seeds[bi] at that
 *                       index -- the bits of the same call given noise = temperature * seer_philox_normal(seed, 1, index); where
 *                       sigma == 0 nothing is drawn and the bits are those of noise = NULL.  Either index source.
 *   seer_slot_cfg_ddim_step with `seeds` uint32 [slots][2] and `temperature` fp32 [slots] in device memory
 *                       sigma is column 2 of the slot's own coef rows.  An idle slot (index < 0 or >= nsched) writes nothing.
 * With seeds set, SEER_EINVAL also for a pointer that is not 4-byte aligned and for a clip of C * F_pred * HW >= 2^31 elements. */
int seer_philox_u32(uint64_t seed, uint64_t stream, uint32_t index, uint64_t first_block, int64_t n_blocks, uint32_t* out,
                    void* hip_stream);
int seer_philox_normal(uint64_t seed, uint32_t stream, uint32_t index, int64_t n, float* out, void* hip_stream);

/* ---- given latents: masked sampling and stochastic_encode (CompVis ldm/models/diffusion/ddim.py:144-147, 207-221) --------------
 * q(e) = sqrtf(a_t) * x0[e] + s1m * n[e]: the given latent x0 noised to the level of coefficient row `index` (a_t = column 0, s1m =
 * column 3).  n is a noise tensor shaped like x0, or -- with seeds uint32 [rows][2] as above -- normal e of Philox stream 2 of the
 * row's seed at that index, e counted in the clip's own [C, F_pred, HW] latent.  Exactly one of `noise` and `seeds` is non-NULL; the
 * seeded form gives the bits of the noise-tensor form fed seer_philox_normal(seed, 2, index).
 *   seer_q_sample          out[bi][e] = q with row index[bi] of coef (fp32 [nsched][4]); x0, noise, out fp32 [b][per_row], index int32
 *                          [b] in device memory.  A row whose index is outside 0 .. nsched - 1 is not written.
 *   seer_known_blend       the mask blend in front of one sampler step, on x [b, C, F_pred, HW] in place.  mask fp32 [b, F_pred, HW]
 *                          (broadcast over channels, values in [0, 1]), known fp32 shaped like x.  index = step[0] when `step` is
 *                          non-NULL (device memory, only read: the kernel runs in front of seer_ddim_step_begin), else the host's
 *                          `index`.  Per element: mask == 0 writes nothing and draws nothing (x keeps its bits); mask == 1 stores q,
 *                          whatever x holds; otherwise x = q * m + (1 - m) * x.  An index < 0 writes nothing.
 *   seer_slot_known_blend  the same over slots, seeded: mask [slots, F_pred, HW], known [slots, C, F_pred, HW], coef fp32
 *                          [slots][nsched][4], index = step[s][0], seeds [slots][2].  A slot whose index is < 0 or >= nsched, or
 *                          whose mask is all zero, is untouched.  It runs in front of seer_slot_step_begin.
 * None of the three writes a step word.  SEER_EINVAL for a NULL required pointer, both or neither of noise and seeds, non-positive
 * extents, a clip (a row of seer_q_sample) of >= 2^31 elements, a pointer that is not 4-byte aligned, a grid beyond one dimension. */
int seer_q_sample(const float* x0, int32_t b, int64_t per_row, const float* coef, int32_t nsched, const int32_t* index,
                  const float* noise, const uint32_t* seeds, float* out, void* stream);
int seer_known_blend(float* x, const float* mask, const float* known, int32_t b, int32_t C, int32_t F_pred, int32_t HW,
                     const float* coef, int32_t index, const int32_t* step, const float* noise, const uint32_t* seeds, void* stream);
int seer_slot_known_blend(float* x, const float* mask, const float* known, int32_t slots, int32_t C, int32_t F_pred, int32_t HW,
                          const float* coef, int32_t nsched, const int32_t* step, const uint32_t* seeds, void* stream);

/* CFG combine + PLMS update of PLMSSampler.p_sample_plms (ldm/models/diffusion/plms.py:199-236; eta = 0, so no noise term), fp32.
 * e is the CFG-combined eps of this evaluation as in seer_cfg_ddim_step (frames >= cond_f only); h1, h2, h3 are earlier e,
 * newest first, each [b, C, F_pred, HW].  e' by `order`:
 *   0: e                                   the first step's provisional DDIM update (plms.py:221)
 *   1: (h1 + e)/2                          the first step's final update: h1 = its first evaluation, e = the second (:223)
 *   2: (3e - h1)/2    3: (23e - 16h1 + 5h2)/12    4: (55e - 59h1 + 37h2 - 9h3)/24      (:226-232)
 * then x0 = (x - sqrt(1-a_t) e')/sqrt(a_t), x' = sqrt(a_prev) x0 + sqrt(1-a_prev-sigma^2) e' from coef row `index`.
 * Order k reads h1 for k >= 1, h2 for k >= 3, h3 for k == 4 and no other history pointer (NULL is allowed there; a slot that is
 * not read may hold anything, NaN included).  e_out (NULL: not written) receives e -- not e' (plms.py:160) -- for every order but
 * 1.  x may alias x_prev, and e_out may alias h1, h2 or h3: every thread reads its element before it writes it. */
int seer_cfg_plms_step(const float* eps, int32_t cfg, int32_t b, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                       float scale, const float* coef, int32_t index, int32_t order, const float* x, const float* h1,
                       const float* h2, const float* h3, float* x_prev, float* pred_x0, float* e_out, void* stream);

/* The same update for a step captured whole in one hipGraph (seer_ddim_step_begin -> UNet -> this kernel): index = step[1], then
 * step[0] = index - 1, as seer_cfg_ddim_step's device form.  The history is a ring of three slots, ring fp32 [3][b*C*F_pred*HW].
 * ring_state int32[4] = (valid, newest) for even indices, then (valid, newest) for odd ones: a step reads the pair of its own
 * index's parity -- valid in 0..3 earlier e, h1 = slot newest, h2 = slot (newest+2)%3, h3 = slot (newest+1)%3 -- runs order 0
 * for valid = 0 and order valid+1 otherwise, stores e into slot s = (newest+1)%3 (the oldest slot once all three are valid), and
 * one thread writes (min(valid+1, 3), s) into the pair of parity (index-1).  No kernel reads and writes the same word, so replays
 * walk the schedule and the ring with no host-written scalars; the host writes step[0] and the pair of the first index to start
 * a chain.  A pair outside those ranges is read as (0, 2).  x may alias x_prev.
 * step[1] < 0, as in seer_cfg_ddim_step: step[0] and the pair of parity (index-1) are written as above, no coefficient row is
 * read and no element of x_prev, pred_x0 or the ring is written. */
int seer_cfg_plms_step_dev(const float* eps, int32_t cfg, int32_t b, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                           float scale, const float* coef, int32_t* step, float* ring, int32_t* ring_state, const float* x,
                           float* x_prev, float* pred_x0, void* stream);

/* CFG combine + DPM-Solver++ update of DPMSolverSampler (Lu et al. 2022, "DPM-Solver++", the data-prediction multistep solver 2M and
 * its first-order form; eta = 0, nothing is drawn), fp32.  e is the CFG-combined eps as in seer_cfg_ddim_step (frames >= cond_f only).
 * The step goes from the level s of schedule entry `index` (abar_s = a_t of the DDIM table) to the level t of its a_prev; with
 * alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = log(alpha / sigma), h = lambda_t - lambda_s:
 *   D      = (x - sigma_s e) / alpha_s                                              the data prediction; pred_x0 receives it
 *   order 1: x_prev = (sigma_t / sigma_s) x - alpha_t (exp(-h) - 1) D               (algebraically the eta = 0 DDIM update)
 *   order 2: the same with D replaced by D + (D - d_prev) / (2 r), r = h_(index+1) / h_(index), d_prev = the D of entry index + 1
 * The kernel evaluates no exp and no log: coef is the DPM table, fp32 [nsched][6], computed on the host in float64, one row per entry:
 *   word 0  sigma_s          word 1  1 / alpha_s                                     D = (x - word0 e) word1
 *   word 2  c_x = sigma_t / sigma_s        word 3  c_D1 = -alpha_t (exp(-h) - 1)     order 1: x_prev = word2 x + word3 D
 *   word 4  c_D2 = c_D1 (1 + 1/(2r))       word 5  c_Dprev = -c_D1 / (2r)            order 2: x_prev = word2 x + word4 D + word5 d_prev
 * The top entry of a schedule has no entry above it, so no r: its words 4 and 5 are (c_D1, 0), and a chain never runs it at order 2.
 *   host form    row `index` and `order` (1 or 2); state is NULL.  d_prev is read at order 2 only (NULL or any contents, NaN
 *                included, at order 1).  x_prev may be x and pred_x0 (NULL: not written) may be d_prev: every thread reads its
 *                element of each before it writes it.
 *   device form  last kernel of a step captured whole in one hipGraph behind seer_ddim_step_begin: index = step[1], then step[0] =
 *                index - 1; `order` is not read and d_prev is NULL.  pred_x0 [b, C, F_pred, HW], required, is history and output at
 *                once: the D of the step before is read from it (order 2 only) and this step's D written over it.  state int32[4]
 *                in device memory = (history valid for an even index, history valid for an odd index, the sampler's order 1 or 2,
 *                nonzero when a schedule's final step -- index 0 -- is first order).  A step reads the valid word of its own
 *                index's parity and runs order 2 when that word is 1, state[2] is 2 and not (index == 0 and state[3] != 0), else
 *                order 1; one thread writes the valid word of parity (index - 1): 1 when this launch stored a D, 0 when it did
 *                not.  state[2] and state[3] are only read, so no kernel reads and writes the same word and replays walk a
 *                schedule with no host-written scalar: to start a chain the host writes step[0] and zeroes state[0..1];
 *                state[2..3] change with the sampler's settings and the schedule only.  An index outside 0 .. nsched - 1: the two
 *                words are written all the same, no table row is read and no element written.
 * SEER_EINVAL for a NULL required pointer (eps, x, coef, x_prev; d_prev at order 2; pred_x0 in the device form), an index source
 * that is neither form, state without step or step without state, d_prev in the device form, b <= 0, non-positive extents, cond_f
 * < 0 or >= F_total, nsched < 1, from the host an index >= nsched or an order other than 1 and 2, a pointer that is not 4-byte
 * aligned, a grid beyond one dimension. */
int seer_cfg_dpm_step(const float* eps, int32_t cfg, int32_t b, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW, float scale,
                      const float* x, const float* coef, int32_t nsched, int32_t index, int32_t order, int32_t* step, int32_t* state,
                      const float* d_prev, float* x_prev, float* pred_x0, void* stream);

/* The captured step over slots with a SAMPLER per slot: DDIM and PLMS clips side by side in one step (slots.py, plms=True).  The
 * buffers of the two slot entry points above, and per slot in device memory
 *   state   int32 [slots][8]: words 0..2 = (phase, valid, newest) of the slot's NEXT step, words 4..6 = the same three of the step
 *           IN FLIGHT, words 3 and 7 unused;
 *   ring    fp32 [slots][3][C*F_pred*HW]: earlier e of the slot, (valid, newest) read as in seer_cfg_plms_step_dev;
 *   x_prov  fp32 [slots][C*F_pred*HW]: the provisional latent of a PLMS clip's first step.
 * phase 0 = a DDIM clip, for all its steps; 1 = a PLMS clip's first step, first evaluation; 2 = its second evaluation; 3 = every
 * later PLMS step.  A clip of n schedule entries takes n calls of the pair with phase 0, n + 1 with PLMS.
 *   seer_slot_step_begin with x_prov and state
 *                              for every slot s as above, and the in-flight words of state[s] = its next words; in
 *                              phase 2 the sample rows come from x_prov[s] instead of x[s] and t_out is t_table[s][max(index - 1,
 *                              0)], the NEXT timestep (plms.py:145).  An idle slot is treated the same way (finite rows as long as
 *                              x, x0_emb and x_prov are).
 *   seer_slot_cfg_plms_step    for every slot s: index = step[s][1], (phase, valid, newest) = the in-flight words, e = the CFG
 *                              combination with scale[s], coefficient row `index` of coef[s].
 *                                phase 0: exactly seer_slot_cfg_ddim_step's update; step[s][0] = index - 1.
 *                                phase 1: x_prov[s] = seer_cfg_plms_step's order 0 of x[s]; e goes into ring entry 0; the next words
 *                                         become (2, 1, 0).  x_prev[s], pred_x0[s] and step[s][0] are NOT written.
 *                                phase 2: order 1 with h1 = ring entry `newest`, from x[s] into x_prev[s] and pred_x0[s]; e is not
 *                                         kept; step[s][0] = index - 1; the next phase becomes 3.
 *                                phase 3: order valid + 1 (order 0 for valid = 0) with h1, h2, h3 = ring entries newest,
 *                                         (newest+2)%3, (newest+1)%3; e goes into entry (newest+1)%3; step[s][0] = index - 1; the
 *                                         next (valid, newest) = (min(valid+1, 3), (newest+1)%3).
 *                              The arithmetic is the device code of seer_cfg_ddim_step / seer_cfg_plms_step, so an element gets
 *                              their bits.  A ring entry the order does not use is never read (it may hold NaN).  index < 0 or
 *                              >= nsched: nothing of that slot is written -- no latent, no ring entry, no word of step or state.
 *                              A phase outside 0..3 is read as 0; in phase 3 a (valid, newest) outside 0..3 x 0..2 is read as
 *                              (0, 2), in phase 2 a newest outside 0..2 as 0: no word found on the device indexes outside the ring.
 *                              x_prev may be x; pred_x0 may be NULL; x_prov may not be x.
 * No kernel reads and writes the same word: begin reads next words (and step[s][0]) and writes in-flight words (and step[s][1]),
 * the update reads in-flight words and writes next words.  The host writes step[s][0] and the next words of state[s] -- (1, 0, 2)
 * for PLMS, (0, 0, 2) for DDIM -- only when it fills slot s.  Every pointer must be 4-byte aligned and no more; SEER_EINVAL
 * otherwise, for everything the two entry points above refuse, for a NULL state, ring or x_prov, and for x_prov == x. */
int seer_slot_cfg_plms_step(const float* eps, int32_t slots, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                            const float* scale, const float* coef, int32_t nsched, int32_t* step, int32_t* state, float* ring,
                            const float* x, float* x_prov, float* x_prev, float* pred_x0, void* stream);

/* The captured step over slots with DDIM and DPM-Solver++ clips side by side (slots.py, dpm=True): the per-slot form of
 * seer_cfg_dpm_step's device form, as seer_slot_cfg_ddim_step is of seer_cfg_ddim_step's.  Its first kernel is seer_slot_step_begin,
 * unchanged: DPM-Solver++ needs no provisional latent and no second evaluation.  Per slot in device memory, beside scale[s],
 * coef[s] (fp32 [slots][nsched][4], the DDIM rows) and step[s][0..1] of seer_slot_cfg_ddim_step:
 *   dpm_coef  fp32 [slots][nsched][6]: a DPM table per slot, the six words per row of seer_cfg_dpm_step;
 *   state     int32 [slots][4]: word 0 = history valid for an even index, word 1 = history valid for an odd index, word 2 = the
 *             slot's sampler (0 DDIM, 1 DPM-Solver++ first order, 2 DPM-Solver++ 2M), word 3 = nonzero when the schedule's final
 *             step -- index 0 -- is first order;
 *   d_hist    fp32 [slots][C*F_pred*HW]: the slot's pred_x0 rows, history and output at once.
 * For every slot s: index = step[s][1], e = the CFG combination with scale[s].
 *   word 2 is 1 or 2:  order 2 when state[s][index & 1] == 1, word 2 == 2 and not (index == 0 and word 3 != 0), else order 1;
 *                      seer_cfg_dpm_step's update of that order with row `index` of dpm_coef[s], d_prev = d_hist[s] (read at order
 *                      2 only: at order 1 it may hold anything, NaN included), and this step's D written over d_hist[s].  The
 *                      slot's first thread writes step[s][0] = index - 1 and state[s][(index - 1) & 1] = 1.
 *   any other word 2:  exactly seer_slot_cfg_ddim_step's update with row `index` of coef[s], pred_x0 = d_hist[s]; step[s][0] =
 *                      index - 1; no state word is written.
 * Words 2 and 3 are only read and the valid word written is of the other parity than the one read: no kernel reads and writes the
 * same word.  The arithmetic is the device code of seer_cfg_ddim_step / seer_cfg_dpm_step, so an element gets their bits.
 * index < 0 or >= nsched: nothing of that slot is written -- no latent, no element of d_hist, no word of step or state.  The host
 * writes step[s][0] and state[s] = (0, 0, sampler, final-step rule) only when it fills slot s: a clip's first step is first order.
 * x_prev may be x; d_hist may be neither.  SEER_EINVAL, and nothing launched, for a NULL pointer (d_hist is required), slots
 * outside 1 .. 4, non-positive extents, cond_f outside 0 .. F_total - 1, nsched < 1, a pointer that is not 4-byte aligned, d_hist
 * == x or d_hist == x_prev, a grid beyond one dimension. */
int seer_slot_cfg_dpm_step(const float* eps, int32_t slots, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                           const float* scale, const float* coef, const float* dpm_coef, int32_t nsched, int32_t* step,
                           int32_t* state, const float* x, float* x_prev, float* d_hist, void* stream);

/* ---- v-prediction: the output of a model trained on the velocity target (train.py:373-374, diffusers get_velocity), as eps -------------
 * With x_t = sqrt(a) x0 + sqrt(1 - a) eps such a model gives v = sqrt(a) eps - sqrt(1 - a) x0, and a sampler needs
 *   eps = sqrtf(a_t) * v + s1m * x_t          a_t = coef[4 r], s1m = coef[4 r + 3] of the DDIM coefficient row r of seer_cfg_ddim_step
 * (rounded fp32 products, then the sum).  ONE elementwise launch in front of a step's last kernel, whichever sampler that is: the
 * conversion is affine in v with the same x_t for both rows of a CFG pair, so converting the rows and then CFG-combining them is the eps
 * of combining v first, and every update kernel above is unchanged.
 *   v, out  fp32 [reps * b, C, F_total, HW], reps 1 (no CFG) or 2 (uc rows, then c rows); only frames >= cond_f are read or written (the
 *           conditioning frames of a model output may hold anything, NaN included); out may be v;
 *   x       fp32 [b, C, F_total - cond_f, HW], the latent the model was evaluated at: output row r reads x[r mod b].
 *   seer_v_to_eps      host form: row `index`.  Device form, inside a captured step between seer_ddim_step_begin and the update:
 *                      index = step[1], the word the begin kernel latched.  It is only read -- this kernel writes NO counter word,
 *                      so "no kernel reads and writes the same word" holds for the step as before.  An index outside 0 .. nsched - 1
 *                      reads no row and writes no element.
 *   seer_slot_v_to_eps over slots, CFG on: rows s and slots + s read x[s], row step[s][1] of coef[s] (fp32 [slots][nsched][4]).  With
 *                      `state` (int32 [slots][8] of seer_slot_step_begin; x_prov then required, NULL both otherwise) a slot whose
 *                      IN-FLIGHT phase word (state[s][4]) is 2 was evaluated at x_prov[s] and t_table[max(index - 1, 0)]: it reads
 *                      x_prov[s] and row max(index - 1, 0).  An idle slot, or a counter outside the table, leaves its rows untouched.
 *                      No step or state word is written.
 * SEER_EINVAL, nothing launched: a NULL required pointer, reps outside {1, 2}, b <= 0, slots outside 1 .. 4, non-positive extents,
 * cond_f outside 0 .. F_total - 1, nsched < 1, an index source that is neither form, a host index >= nsched, state without x_prov or
 * the reverse, x_prov == x, a pointer that is not 4-byte aligned, a grid beyond one dimension. */
int seer_v_to_eps(const float* v, int32_t reps, int32_t b, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW, const float* coef,
                  int32_t nsched, int32_t index, const int32_t* step, const float* x, float* out, void* stream);
int seer_slot_v_to_eps(const float* v, int32_t slots, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW, const float* coef,
                       int32_t nsched, const int32_t* step, const int32_t* state /* NULL: no sampler per slot */, const float* x,
                       const float* x_prov /* NULL with state */, float* out, void* stream);

/* ---- guidance rescale: classifier-free guidance with the std of the conditional branch (Lin et al. 2023, "Common Diffusion Noise
 * Schedules and Sample Steps are Flawed", section 3.4; diffusers rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale)) --------
 * Guidance at scale s multiplies the std of the model output by a factor that grows with s.  Per CLIP, over the n = C (F_total - cond_f)
 * HW elements of its predicted frames (frames >= cond_f; the conditioning frames are never read or written and may hold NaN):
 *   c_i  the conditional row,      g_i = eu_i + scale * (c_i - eu_i), the fp32 value every update kernel above combines (one device
 *        function for all of them), so the moments are taken of exactly the numbers that get scaled;
 *   S1c = sum c, S2c = sum c c, S1g = sum g, S2g = sum g g       in double (every fp32 x fp32 product is exact there);
 *   q_c = max(n S2c - S1c^2, 0),   q_g = n S2g - S1g^2           (n^2 times the variance: exact on integer data, and the n - 1 of an
 *                                                                  unbiased std cancels in the ratio);
 *   m   = (float)(phi * sqrt(q_c / q_g) + (1 - phi))             in double, phi = `rescale` widened from float;
 *   out = m * g                                                   one fp32 product, written IN PLACE to the clip's uc row AND its c row.
 * That is rescale_noise_cfg with std over all non-batch dims (agreement in float64: 6e-15).  DEVIATION: where q_g <= 0 (a constant g;
 * n = 1) or the ratio is not finite, m = 1 and out = g; diffusers divides by the zero std and returns inf or NaN.
 * Both rows are overwritten because the update kernels are unchanged: they compute eu + scale * (ec - eu) with eu == ec, which is ec
 * again exactly for finite values (ec - eu = +0, scale * 0 = 0, eu + 0 = eu, with or without FMA contraction).  The node acts on the raw
 * model output -- for a v-model on v, IN FRONT of seer_v_to_eps, whose conversion is affine with the same x_t for both rows and keeps
 * them equal.
 * TWO launches over the same grid (P, clips), P = ceil(n / SEER_RESCALE_TILE), and no atomics, counters or waiting inside a launch:
 *   moments  block (p, clip) reduces elements [p TILE, min((p + 1) TILE, n)) to the four doubles in a fixed order -- per thread in index
 *            order, __shfl_xor across the wave64, the waves through LDS in wave order -- and stores them to ws[clip][p][4];
 *   apply    every block sums its clip's P partials in index order, makes m and writes m g to both rows of its tile (an element's two
 *            inputs are read before either is written); block p = 0 writes mult[clip] = m when mult != NULL.
 * The tiling depends on n alone -- not on b, the row or the slot -- so a clip's m and rows are the same bits in any batch or slot layout
 * and in every run.
 *   out   fp32 [2 b, C, F_total, HW], uc rows then c rows (slot form: b = slots, slot s owns rows s and slots + s);
 *   ws    double [clips][P][4], seer_cfg_rescale_ws_bytes(clips, ...) bytes, 8-byte aligned; it need not be zeroed;
 *   mult  fp32 [clips] or NULL: the multipliers, for a caller that wants to look at them.
 *   seer_cfg_rescale       `scale` and `rescale` from the host, for every clip.  rescale == 0: SEER_OK, nothing launched.
 *   seer_slot_cfg_rescale  slot s uses scale[s] and rescale[s] (device memory) and its in-flight index step[s][1].  A slot that is idle
 *                          (index < 0 or >= nsched) or has rescale[s] == 0 has NONE of its words written: neither rows, ws nor mult.
 *                          No step or state word is written by either kernel.  It does not read a PLMS phase: both evaluations of a
 *                          PLMS first step are rescaled alike.  rescale[s] is not clamped: the host validates it (SlotSampler.submit).
 * SEER_EINVAL, nothing launched: a NULL required pointer (mult may be NULL), b <= 0, slots outside 1 .. 4, non-positive extents, cond_f
 * outside 0 .. F_total - 1, nsched < 1, (solo form) rescale outside [0, 1] or not finite, a pointer that is not 4-byte (ws: 8-byte)
 * aligned, more than 65535 clips or 2^31 - 1 tiles.  seer_cfg_rescale_ws_bytes returns SEER_EINVAL for clips <= 0 or such extents. */
#define SEER_RESCALE_TILE 1024   /* elements of a clip per workgroup: 256 threads x 4; a multiple of 256 */
int64_t seer_cfg_rescale_ws_bytes(int32_t clips, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW);
int seer_cfg_rescale(float* out, int32_t b, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW, float scale, float rescale,
                     double* ws, float* mult /* [b] or NULL */, void* stream);
int seer_slot_cfg_rescale(float* out, int32_t slots, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW, const float* scale,
                          const float* rescale, int32_t nsched, const int32_t* step, double* ws, float* mult /* [slots] or NULL */,
                          void* stream);

/* decoded image post-process of ddim_sample (utils/ddim_sampling_utils.py:41): clamp((x+1)/2, 0, 1) in place */
int seer_clamp01(float* x, int64_t n, void* stream);

/* VAE encode, the step before the path: DiagonalGaussianDistribution.sample
 * (ldm/modules/distributions/distributions.py:24-37; diffusers AutoencoderKL.encode(x).latent_dist.sample(),
 * inference_img.py:168): moments fp32 [N, 2C, HW] = (mean | logvar) along channels ->
 *   out[n, c, i] = mean + exp(0.5 * clamp(logvar, -30, 20)) * noise[n, c, i]        (noise NULL: the mode) */
int seer_gaussian_sample(const float* moments, int32_t N, int32_t C, int32_t HW, const float* noise, float* out,
                         void* stream);

/* ---- training step (train.py:319-389) --------------------------------------------------------------
 * The backward pass reuses seer_gemm_bf16 for the input gradients and has one more MFMA kernel for the weight gradients:
 *   dX[M,K] = dY[M,N] W[N,K]       -> A = dY, W' = W^T ([K][N], a transposed copy of the weight: seer_transpose_bf16)
 *   dW[N,K] = dY^T[N,M] X[M,K]     -> seer_gemm_tn_f32 (both operands read as they are, fragments by transposed LDS reads)
 *   conv3x3 dX                     -> the CONV3X3 mode with the weight repacked as w'[ci][2-ky][2-kx][co]; a stride-2 conv
 *                                     first spreads dY with seer_zero_insert2x_bf16, a conv behind the nearest-2x upsample
 *                                     folds its dX with seer_sumpool2x_bf16
 * and seer_attn_bwd for attention.  The entry points below are the HBM-bound remainder.  Every reduction is two-stage through
 * a caller workspace (no float atomics). */

/* weight gradient without transposes: C[n*K + k] = sum_m A[m*lda + n] * B[m*ldb + k]   (dW[N,K] = dY[M,N]^T X[M,K]), bf16
 * operands in their token-major layout, fp32 result; colsum (optional) receives sum_m A[m][n] -- the bias gradient -- from
 * one more MFMA against a fragment of ones.  N, K, lda, ldb multiples of 8.  The contraction is split across blocks; slices
 * meet in `workspace` (seer_gemm_tn_workspace_bytes(M, N, K) bytes, 0 = not needed) and are added in slice order. */
int64_t seer_gemm_tn_workspace_bytes(int32_t M, int32_t N, int32_t K);
int seer_gemm_tn_f32(const void* A, int32_t lda, const void* B, int32_t ldb, int32_t M, int32_t N, int32_t K, float* C,
                     float* colsum, void* workspace, int64_t workspace_bytes, void* stream);

/* The weight gradients of MANY layers in one launch (ABI 24).  In the reference every trainable nn.Linear gets its `.grad` from
 * autograd's backward (train.py:382 `accelerator.backward(loss)`), one product per layer wherever the walk reaches it; none of them
 * depends on another and nothing reads them before the optimizer (train.py:383-386), so a backward pass may leave them to its end:
 * `items` is a HOST array (the launch carries its problem table in the kernel arguments, 48 problems per launch: a captured launch keeps
 * it), item i as seer_gemm_tn_f32's arguments.  A problem is split over ceil(M / group_rows) workgroups per tile (the group fills the chip by its number of problems);
 * slices meet in `workspace` (seer_gemm_tn_grouped_workspace_bytes) and one more launch adds them in slice order.  Results are
 * independent of how problems are grouped: a problem's bits depend on its own (M, N, K) and group_rows only -- on nothing else in the
 * group and on nothing in the process environment. */
typedef struct seer_tn_item {
    const void* A;          /* dY [M][N] bf16, row pitch lda */
    const void* B;          /* X  [M][K] bf16, row pitch ldb */
    float* C;               /* dW [N][K] fp32 */
    float* colsum;          /* [N] fp32 or NULL */
    int32_t lda, ldb, M, N, K;
    int32_t group_rows;     /* rows of the contraction per workgroup, rounded up to the tile height; 0 (or below a tile) = 16384.
                               (The field zero-initialised callers knew as `reserved`: same layout, same results.) */
} seer_tn_item;
int64_t seer_gemm_tn_grouped_workspace_bytes(const seer_tn_item* items /* host */, int32_t n_items);
int seer_gemm_tn_grouped_f32(const seer_tn_item* items /* host */, int32_t n_items, void* workspace, int64_t workspace_bytes,
                             void* stream);

/* y[c*ldy + r] = x[r*ldx + c]; columns rows..ldy-1 of y are zero filled */
int seer_transpose_bf16(const void* x, int64_t rows, int32_t cols, int32_t ldx, void* y, int64_t ldy, void* stream);

/* The same for many matrices in one launch (the W^T refresh of all trainable matrices after an optimizer step).  `items` is a
 * DEVICE array, read by the kernel: matrix i is x [rows, cols] with row pitch ldx -> y [cols, ldy], 64x64 tiles numbered
 * tile0 + (tile row) + tiles_r * (tile column), tiles_r = ldy / 64, tile0 = the running sum of tiles_r * ceil(cols / 64)
 * (ascending, items[0].tile0 = 0); total_tiles = that sum over all items.  Every item: cols % 8 == 0, ldx % 8 == 0,
 * ldy % 64 == 0, ldy >= rows, x and y 16-byte aligned (the caller checks: the table is not readable from the host side). */
typedef struct seer_transpose_item {
    const void* x;
    void* y;
    int64_t rows;
    int64_t ldy;
    int64_t tile0;
    int32_t cols;
    int32_t ldx;
    int32_t tiles_r;
    int32_t reserved;
} seer_transpose_item;
int seer_transpose_batched_bf16(const seer_transpose_item* items, int32_t n_items, int64_t total_tiles, void* stream);

/* out[c] = sum_r x[r][c] (bias gradients).  workspace: seer_colsum_workspace_floats(rows, cols) floats (the same size
 * serves seer_layernorm_bwd). */
int64_t seer_colsum_workspace_floats(int64_t rows, int32_t cols);
int seer_colsum_bf16(const void* x, int64_t rows, int32_t cols, int32_t ldx, float* out, float* workspace, void* stream);

/* nn.LayerNorm backward (attention.py:198-200,275-277): dx = rstd (g - mean(g) - xhat mean(g xhat)) (+ dres), g = dy gamma;
 * dgamma = sum_r dy xhat, dbeta = sum_r dy (both NULL for a frozen norm).  dres: gradient arriving on the residual path
 * that shares x (fused add), or NULL. */
int seer_layernorm_bwd(const void* x, const void* dy, int64_t rows, int32_t C, int32_t ldx, int32_t lddy, const float* gamma,
                       float eps, const void* dres, int32_t ldres, void* dx, int32_t lddx, float* dgamma, float* dbeta,
                       float* workspace, void* stream);
/* The same, leaving d gamma / d beta as partial slabs: workspace[slab][2][C] (v 0 = d beta, v 1 = d gamma), seer_layernorm_bwd_slabs(rows)
 * slabs; seer_colfinal_grouped adds the slabs of MANY norms in one launch (ABI 24: the finals of every LayerNorm a backward walk
 * passed, deferred to its end -- nothing reads them before the optimizer, train.py:383-386).  Bits as seer_layernorm_bwd's. */
int64_t seer_layernorm_bwd_slabs(int64_t rows);
int seer_layernorm_bwd_partials(const void* x, const void* dy, int64_t rows, int32_t C, int32_t ldx, int32_t lddy, const float* gamma,
                                float eps, const void* dres, int32_t ldres, void* dx, int32_t lddx, float* workspace, void* stream);
/* out_v[c] = sum over k < nblocks of ws[(k * NV + v) * C + c], k in a fixed order; `items` is a HOST array (64 per launch, by value) */
typedef struct seer_colfinal_item {
    const float* ws;
    float* out0;            /* v = 0, or NULL */
    float* out1;            /* v = 1, or NULL */
    int32_t nblocks, NV, C, reserved;
} seer_colfinal_item;
int seer_colfinal_grouped(const seer_colfinal_item* items /* host */, int32_t n_items, void* stream);

/* GroupNorm (+ optional SiLU) backward over (C/G, F, H, W) per (b, g); stats/count/eps/gamma/beta/silu as in the forward
 * pair seer_groupnorm_stats / seer_groupnorm_apply.  dy bf16 [rows, C1+C2]; dx1/dx2 are the gradients of the two concat
 * sources (+ dres1/dres2 when given). */
int64_t seer_groupnorm_bwd_workspace_floats(int32_t C, int32_t batch, int64_t rows_per_batch, int32_t groups);
int seer_groupnorm_bwd(const void* x1, int32_t C1, const void* x2, int32_t C2, int32_t batch, int64_t rows_per_batch,
                       int32_t groups, const float* stats, double count, float eps, const float* gamma, const float* beta,
                       int32_t silu, const void* dy, const void* dres1, const void* dres2, void* dx1, void* dx2,
                       float* dgamma, float* dbeta, float* workspace, void* stream);

/* GEGLU (attention.py:785-793) outside the GEMM epilogue, on the interleaved projection layout of SEER_EPI_GEGLU
 * (columns [32g, 32g+16) values, [32g+16, 32g+32) gates -> output columns [16g, 16g+16)): the training forward keeps the
 * pre-activation for the backward. */
int seer_geglu_fwd(const void* pre, int64_t rows, int32_t inner, int32_t ldp, void* out, int32_t ldo, void* stream);
int seer_geglu_bwd(const void* pre, const void* dout, int64_t rows, int32_t inner, int32_t ldp, int32_t lddo, void* dpre,
                   int32_t lddp, void* stream);

/* y = a + b on bf16 [rows, cols] views (gradient fan-in) */
int seer_add_bf16(const void* a, int32_t lda, const void* b, int32_t ldb, void* y, int32_t ldy, int64_t rows, int32_t cols,
                  void* stream);
/* backward of the nearest-2x upsample (resnet.py:39): dx[img,y,x,:] = sum of the 2x2 block of du [n_img, 2H, 2W, C] */
int seer_sumpool2x_bf16(const void* du, int32_t n_img, int32_t H, int32_t W, int32_t C, void* dx, void* stream);
/* z [n_img, 2H, 2W, C]: z[2y, 2x] = d[y, x], zero elsewhere (input-gradient of a stride-2 conv, resnet.py:52-57) */
int seer_zero_insert2x_bf16(const void* d, int32_t n_img, int32_t H, int32_t W, int32_t C, void* z, void* stream);

/* epsilon-MSE of train.py:380: loss = mean((pred[:, :, cond_f:] - target)^2) over [B, C, F_total - cond_f, HW];
 * dpred fp32 [B, C, F_total, HW] = d loss / d pred (zero on the conditioning frames).  workspace: 1024 floats. */
int seer_mse_loss_grad(const float* pred, const float* target, int32_t B, int32_t C, int32_t F_total, int32_t cond_f,
                       int32_t HW, float* loss, float* dpred, float* workspace, void* stream);
/* The same loss with Min-SNR-gamma weighting (Hang et al., "Efficient Diffusion Training via Min-SNR Weighting Strategy", ICCV 2023;
 * `--snr_gamma` of the diffusers training scripts): sample b carries the weight w_b of its timestep, inside the loss and inside dpred.
 *   pred, dpred     fp32 [B, C, F_total, HW];   target fp32 [B, C, F_total - cond_f, HW]
 *   timesteps       int64 [B], alphas_cumprod fp32 [T], BOTH IN DEVICE MEMORY (a captured step stays valid when the timesteps change);
 *                   a timestep outside [0, T) is clamped into the table, as in seer_velocity_target.  The table's values are the
 *                   caller's and are not checked: they lie in [0, 1].
 *   a = alphas_cumprod[t_b] and snr_gamma widened to double; each operation below one rounded double operation; w_b rounded once to fp32:
 *     v_prediction == 0 (eps-model):  w_b = fmin(1.0, snr_gamma * (1.0 - a) / a)     = min(SNR, gamma) / SNR;        a = 0: 1,  a = 1: 0
 *     v_prediction == 1 (v-model):    w_b = fmin(a, snr_gamma * (1.0 - a))           = min(SNR, gamma) / (SNR + 1);  a = 0: 0,  a = 1: 0
 *   weights[b]      = w_b                                                            (the bits of that float64 expression cast to fp32)
 *   sample_loss[b]  = mean over the n_s = C (F_total - cond_f) HW predicted elements of sample b of (pred - target)^2, UNweighted
 *   loss            = (1 / B) sum_b w_b sample_loss_b
 *   dpred[i]        = 2.0f * d * inv_n * w_b, the products in this order, d = pred - target and inv_n = (float)(1.0 / (B n_s)): the
 *                     expression of seer_mse_loss_grad times w_b (the same bits where w_b == 1); +0.0f on the conditioning frames.
 * Reproducible, no atomics.  Launch one, grid (nblk, B), nblk <= SEER_SNR_MSE_BLOCKS: a block strides over its sample, adds
 * (double)(d * d) (the fp32 product, widened), tree-reduces in LDS in a fixed order and stores one double at workspace[b * nblk + blk].
 * Launch two adds a sample's partials in index order (sum_b), writes sample_loss[b] = (float)(sum_b * (1.0 / n_s)), adds
 * (double)w_b * (sum_b / n_s) over b = 0 .. B-1 in order and writes loss = (float)(total / B).
 *   workspace       B * SEER_SNR_MSE_BLOCKS doubles, 8-byte aligned; it need not be zeroed.
 * 16-byte accesses when HW % 4 == 0 and pred, target and dpred are 16-byte aligned, a scalar path otherwise.
 * SEER_EINVAL, nothing launched: a NULL pointer; T, B, C, F_total or HW not positive; cond_f outside 0 .. F_total - 1; B above 65535 (the
 * launch grid) or more than 2^46 elements; snr_gamma not finite or not positive; v_prediction outside {0, 1}; a float pointer not
 * 4-byte aligned, timesteps or workspace not 8-byte aligned; dpred overlapping pred or target, or any two of the five outputs
 * (loss, sample_loss, weights, dpred, workspace) overlapping. */
#define SEER_SNR_MSE_BLOCKS 64
int seer_snr_mse_loss_grad(const float* pred, const float* target, const int64_t* timesteps, const float* alphas_cumprod, int32_t T,
                           float snr_gamma, int32_t v_prediction, int32_t B, int32_t C, int32_t F_total, int32_t cond_f, int32_t HW,
                           float* loss, float* sample_loss, float* weights, float* dpred, double* workspace, void* stream);
/* `--text_loss` of train.py:346-347 (the FSTextTransformer initialisation stage): loss = mean_{b,l,c} (mean_f y - target)^2
 * with y bf16 [b, F, LC] (FSTextTransformer output), target fp32 [b, LC] (the CLIP sequence); its gradient is ADDED to dy
 * (bf16 [b, F, LC], the gradient arriving from the UNet).  workspace: 1024 floats. */
int seer_text_loss_grad(const void* y, const float* target, int32_t b, int32_t F, int64_t LC, void* dy, float* loss,
                        float* workspace, void* stream);
/* input gradient of conv_out (frozen): dpred fp32 [B, Cout, F, H, W] -> dx bf16 [B*F, H*W, C0]; W fp32 [Cout][3][3][C0] */
int seer_conv_out_bwd(const float* dpred, int32_t B, int32_t C0, int32_t F, int32_t H, int32_t W, const float* Wt,
                      int32_t Cout, void* dx, void* stream);

/* y = beta*y + alpha*x on fp32 buffers (x may alias y), n % 4 == 0 (gradient accumulation over micro-batches: train.py:321
 * `accelerator.accumulate`, configs/train.yaml gradient_accumulation_steps) */
int seer_axpby_f32(float* y, const float* x, float alpha, float beta, int64_t n, void* stream);
/* out[0] = sum g^2 (workspace: 1024 floats) */
int seer_sumsq_f32(const float* g, int64_t n, float* out, float* workspace, void* stream);
/* torch.optim.AdamW step (train.py:226-232,385) on flat fp32 buffers; when grad_sumsq != NULL the gradient is first scaled
 * by min(1, max_norm / (sqrt(*grad_sumsq) + 1e-6)) (clip_grad_norm_, train.py:384).  step = 1, 2, ...; p_bf16 (optional)
 * receives the bf16 working copy of the updated parameters. */
int seer_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int32_t step, const float* grad_sumsq, float max_norm, void* p_bf16, void* stream);
/* The same step with 8-bit optimizer state (train.py:214-222 `use_8bit_adam`; block-wise dynamic quantisation after the 8-bit
 * optimizers paper; this project's own format, NOT interchangeable with bitsandbytes' state files).  A block is 256 consecutive
 * elements.  Per element two uint8 codes cm / cv, per block two fp32 scales absmax_m / absmax_v [n / 256]; qmap_m (signed) and
 * qmap_v (unsigned) are the code books, 256 ascending fp32 entries each.  Fresh state: cm = 127, cv = 0 (the zero codes), scales 0.
 * Per block, in fp32 and in the order of seer_adamw_step:
 *   m = qmap_m[cm] * absmax_m,  v = qmap_v[cv] * absmax_v;   m = b1 m + (1 - b1) g',  v = b2 v + (1 - b2) g' g'  (g' = clipped g)
 *   p = p (1 - lr wd) - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)          with the new m, v BEFORE they are quantised
 *   absmax_m' = max |m|, absmax_v' = max v over the block;  cm' / cv' = the code of the entry nearest to m / absmax_m', v / absmax_v'
 *   (a tie goes either way; the zero code when the block maximum is 0).
 * A non-finite moment stays out of the block maximum, so the scales remain finite; its own code is defined but meaningless.
 * p_bf16 (optional) as above.  SEER_EINVAL, nothing launched: a NULL required pointer, n <= 0, n % 256 != 0, step < 1, p or g not
 * 16-byte aligned, cm / cv / a float array not 4-byte aligned, p_bf16 not 8-byte aligned. */
int seer_adamw8_step(float* p, const float* g, uint8_t* cm, uint8_t* cv, float* absmax_m, float* absmax_v, const float* qmap_m,
                     const float* qmap_v, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                     int32_t step, const float* grad_sumsq, float max_norm, void* p_bf16, void* stream);
/* seer_adamw_step / seer_adamw8_step that also move an exponential moving average of the parameters (the CompVis tree's
 * ldm/modules/ema.py LitEma, diffusers' `--use_ema`) in the same launch, from the register that holds the new parameter p':
 *   ema' = ema - one_minus_decay * (ema - p')
 * LitEma.forward's `shadow.sub_(one_minus_decay * (shadow - param))`: three fp32 operations, each rounded on its own (a difference, a
 * product, a difference; never contracted into a fused multiply-add), so ema' has the bits of those three torch operations.  p, the
 * moments (codes, scales) and p_bf16 receive exactly what the plain entry point writes.  ema: fp32 [n] in BOTH optimizer modes: at
 * decay 0.9999 a step moves the average by 1e-4 of its distance to p', far below what an 8- or 16-bit state can hold.
 * The expression is taken literally: one_minus_decay = 1 does not always yield p' exactly (ema - (ema - p') rounds twice);
 * one_minus_decay = 0 leaves ema's bits untouched unless ema - p' is non-finite (0 * inf = NaN); a non-finite p' makes ema non-finite,
 * as in LitEma: there is no guard.
 * SEER_EINVAL, nothing launched: everything the plain entry point refuses; ema == NULL; one_minus_decay outside [0, 1] (a NaN
 * included); ema not 4-byte (seer_adamw_ema_step) or not 16-byte (seer_adamw8_ema_step) aligned; ema's n floats overlapping p, g, the
 * moments (m, v; cm, cv, absmax_m, absmax_v), p_bf16 or grad_sumsq. */
int seer_adamw_ema_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int32_t step, const float* grad_sumsq, float max_norm, void* p_bf16, void* stream,
                        float* ema, float one_minus_decay);
int seer_adamw8_ema_step(float* p, const float* g, uint8_t* cm, uint8_t* cv, float* absmax_m, float* absmax_v, const float* qmap_m,
                         const float* qmap_v, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                         int32_t step, const float* grad_sumsq, float max_norm, void* p_bf16, void* stream, float* ema,
                         float one_minus_decay);

/* The glue of train.py:349-365 between the VAE encoder and the UNet, in ONE launch: posterior sample, latent scale, DDPM add_noise
 * and the `(b f) c h w -> b c f h w` rearranges (train.py:353-354,365).
 *   moments        fp32 [b, F, 2C, HW]  encoder output of all F = f1 + f2 frames of every video, images in (b f) order, (mean | logvar)
 *   eps_post       fp32 [b, F, C, HW]   posterior noise, or NULL: the mean is taken
 *   noise          fp32 [b, C, f2, HW]  the DDPM noise (= the epsilon target of the loss)
 *   timesteps      int64 [b];  alphas_cumprod fp32 [T] (DDPMScheduler.alphas_cumprod)
 *   model_input    fp32 [b, C, F, HW]   cat[latents_x0, noisy_latents] along frames (train.py:365)
 *   latents        fp32 [b, C, f2, HW]  the clean scaled latents of the f2 frames, or NULL: not written
 * Per element, in fp32:  z = mean + exp(0.5 * clamp(logvar, -30, 20)) * eps  (the bits of seer_gaussian_sample),  lat = z * latent_scale;
 *   f <  f1:  model_input[b, c, f] = lat
 *   f >= f1:  model_input[b, c, f] = sqrt(a) * lat + sqrt(1 - a) * noise[b, c, f - f1],   a = alphas_cumprod[timesteps[b]]
 * A timestep outside [0, T) is clamped into the table by the kernel, never dereferenced (callers reject it beforehand).  16-byte
 * accesses along HW when HW % 4 == 0 and all five bases are 16-byte aligned, a scalar path otherwise: any HW > 0 is accepted.
 * SEER_EINVAL: a NULL required pointer, a non-positive extent, f2 < 1 (f1 = 0, no conditioning frame, is allowed), F or b*C above
 * 65535 (the launch grid). */
int seer_train_inputs(const float* moments, const float* eps_post, const float* noise, const int64_t* timesteps,
                      const float* alphas_cumprod, int32_t T, int32_t b, int32_t C, int32_t f1, int32_t f2, int32_t HW,
                      float latent_scale, float* model_input, float* latents, void* stream);

/* The loss target of a v-prediction model (train.py:373-374, `noise_scheduler.get_velocity(latents, noise, timesteps)`):
 *   target[bi, e] = sqrtf(a) * noise[bi, e] - sqrtf(1 - a) * latents[bi, e],   a = alphas_cumprod[timesteps[bi]]
 * latents, noise, target fp32 [b, per_row] (the clean scaled latents seer_train_inputs writes, and its noise); timesteps int64 [b];
 * alphas_cumprod fp32 [T].  A timestep outside [0, T) is clamped into the table, as in seer_train_inputs.  16-byte accesses when
 * per_row % 4 == 0 and the three bases are 16-byte aligned, a scalar path otherwise.  SEER_EINVAL: a NULL pointer, T, b or per_row not
 * positive, b above 65535 (the launch grid), a float pointer not 4-byte or timesteps not 8-byte aligned, a grid beyond its limit. */
int seer_velocity_target(const float* latents, const float* noise, const int64_t* timesteps, const float* alphas_cumprod, int32_t T,
                         int32_t b, int64_t per_row, float* target, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEER_HIP_H */
