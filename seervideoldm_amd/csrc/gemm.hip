// seer_gemm_bf16 (include/seer_hip.h): the launch planner, the host queries that read its plan, and the dispatch to the four
// kernels.  Host code only; no kernel in this unit:
//   the tile kernel        gemm_tile_kernel.h, emitted by the units gemm_tiles_<u>.hip (the tile table: gemm_tiles.h)
//   split-K second pass    gemm_reduce.hip
//   weight-stationary      gemm_ws.hip
//   256 x 320 tile         gemm_t320.hip
#include "gemm_tiles.h"

namespace {

// the kernel's `staged` condition, host side: column sums are taken from the staged bf16 tile
bool colsum_store_ok(const seer_gemm_desc& d) {
    return !(d.epilogue & (SEER_EPI_OUT_F32 | SEER_EPI_TRANS_OUT | SEER_EPI_GEGLU)) && d.ldc % 8 == 0 && d.N % 8 == 0 &&
           (reinterpret_cast<uintptr_t>(d.C) & 15) == 0 && (d.batch <= 1 || (d.strideC % 8) == 0);
}

// the argument checks of every launch; normalises K1 / lda2 / batch and the strides of the phase convs in place.  No decisions.
int validate(seer_gemm_desc& d) {
    if (d.M <= 0 || d.N <= 0 || d.K <= 0) return SEER_EINVAL;
    if (d.K % BK) return SEER_EINVAL;
    if (!d.A || !d.W || !d.C) return SEER_EINVAL;
    const bool geglu = (d.epilogue & SEER_EPI_GEGLU) != 0;
    if (d.N % (geglu ? 32 : 4)) return SEER_EINVAL;
    if (d.mode == SEER_GEMM_CONV3X3) {
        if (d.Cin <= 0 || d.Cin % BK) return SEER_EINVAL;
        if (d.Hin <= 0 || d.Win <= 0 || d.Hout <= 0 || d.Wout <= 0) return SEER_EINVAL;
        if (d.upsample == 2) {
            // four 2x2 phase convs as the four batch elements of one launch: same input, W[phase][N][4 Cin], rows scattered
            if (d.K != 4 * d.Cin || d.stride != 1 || d.pad_after_only || d.Hout != 2 * d.Hin || d.Wout != 2 * d.Win) return SEER_EINVAL;
            if (d.M % (d.Hin * d.Win) || d.residual || d.rowvec) return SEER_EINVAL;
            if (d.epilogue & (SEER_EPI_OUT_F32 | SEER_EPI_TRANS_OUT | SEER_EPI_ROTARY | SEER_EPI_GEGLU)) return SEER_EINVAL;
            d.batch = 4;
            d.strideA = 0;
            d.strideW = (int64_t)d.N * d.K;
            d.strideC = 0;
        } else {
            if (d.K != 9 * d.Cin) return SEER_EINVAL;
            if (d.stride != 1 && d.stride != 2) return SEER_EINVAL;
            if (d.M % (d.Hout * d.Wout)) return SEER_EINVAL;
        }
        d.K1 = d.K;
    } else if (d.mode == SEER_GEMM_PLAIN) {
        if (!d.A2) { d.K1 = d.K; d.lda2 = 0; }
        if (d.K1 % BK || d.K1 > d.K || d.lda % 8 || (d.A2 && d.lda2 % 8)) return SEER_EINVAL;
    } else {
        return SEER_EINVAL;
    }
    if (!(d.epilogue & SEER_EPI_TRANS_OUT) && (d.ldc % 4)) return SEER_EINVAL;
    if (d.residual && (d.ldr % 4)) return SEER_EINVAL;
    if (d.rowvec && d.rows_per_batch <= 0) return SEER_EINVAL;
    if ((d.epilogue & SEER_EPI_SILU) && (d.epilogue & SEER_EPI_QUICKGELU)) return SEER_EINVAL;      // one activation per launch
    if (d.epilogue & SEER_EPI_ROTARY) {
        if (!d.rot_table || d.rot_head_dim <= 0 || d.rot_head_dim % 4 || d.rot_dim <= 0 || d.rot_dim % 4 ||
            d.rot_dim > d.rot_head_dim || d.rot_tokens_per_batch <= 0 || d.rot_cols % d.rot_head_dim || geglu)
            return SEER_EINVAL;
    }
    if (d.epilogue & SEER_EPI_COLSCALE) {
        if (geglu || d.col_scale_cols <= 0 || d.col_scale_cols % 4 || d.col_scale_cols > d.N) return SEER_EINVAL;
    }
    if (d.batch <= 1) d.batch = 1;
    return SEER_OK;
}

// split-K decision for a validated descriptor whose d.tile names a tile kernel or AUTO: few output tiles and a long K loop
// (deep-level convs / linears, M = 384 .. 1536).  Returns the K slices (1: no split) and the tile that runs them.
struct split_choice { int splits, tile; };
split_choice choose_split(const seer_gemm_desc& d) {
    const bool geglu = (d.epilogue & SEER_EPI_GEGLU) != 0;
    int s = 1, tile = d.tile;
    const bool can_split = d.batch == 1 && !geglu && !(d.epilogue & (SEER_EPI_TRANS_OUT | SEER_EPI_ROTARY)) &&
                           (d.tile == SEER_TILE_AUTO || d.tile == SEER_TILE_64x64 || d.tile == SEER_TILE_G64x64_3 ||
                            d.tile == SEER_TILE_G128x128_2 || d.tile == SEER_TILE_G96x160_2) &&
                           d.splits != 1;
    if (can_split) {
        const int nk = d.K / BK;
        if (d.splits > 1) {
            s = d.splits < nk ? d.splits : nk;
        } else if (d.splits == 0) {
            // measured on MI355X (profiles/r01_splitk_sweep.log, r01_sweep_shapes.log): the reduce pass + second launch
            // cost ~4-5 us, so splitting pays only when a slice keeps >= ~11 K tiles and the unsplit grid leaves CUs idle.
            // Wide outputs (N a multiple of 128, >= 640): 128x128 tiles (half the L2->LDS bytes per FLOP of 64x64), K
            // sliced until the grid holds ~2 blocks per CU -- the 16x16-level convs at B*F = 24 (x2), the 8x8 level (x4),
            // the 4x4 level (x16) and, with fewer frames or one CFG half per rank, the same levels sliced deeper.
            const long t128 = (long)((d.M + 127) / 128) * ((d.N + 127) / 128);
            const long blocks64 = (long)((d.M + 63) / 64) * ((d.N + 63) / 64);
            // (the 8x8-level feed-forward output projection, 1536 x 1280 x 5120: 35.2 us on 128x128 x 4 slices + the reduce pass against
            // 40.0 unsplit on the 5-stage 64x64 ring: profiles/r04_ff2_tile_sweep.log)
            int s128 = 1;
            // (cold weights, r06_lab_cold_weights.log / r06_lab_cold_train.log: a PLAIN product is sliced to ONE round of the chip, not two
            //  -- 1536 x 1280 x 6400: 2 slices 41.3 against 43.3 us for 4; 768 x 1280 x 10240: 4 slices 37.0 against 45.3 for 8; 924 x 768 x
            //  6144: 4 slices 23.8 against 30.7 -- while the convs, whose slices are ten times longer, keep two)
            const long split_target = d.mode == SEER_GEMM_PLAIN ? 180 : 400, split_accept = d.mode == SEER_GEMM_PLAIN ? 180 : 200;
            if (d.N % 128 == 0 && d.N >= 640 && d.M >= 256 && t128 < 256 && nk >= 64)
                while (t128 * s128 < split_target && s128 < 16 && nk / (2 * s128) >= 11) s128 *= 2;
            // N = 320 on half the rows (one CFG half per rank: 12 288 rows = 256 tiles of 96x160, one lone workgroup per CU, which
            // runs a K tile no faster than two co-resident ones do): two K slices bring the second workgroup back.  3x3 convs only
            // (K >= 2880): 47.1 -> 44.9, 84.4 -> 76.8, 128.0 -> 103.5 us; the K = 1280 GEMM loses (profiles/r02_half_rows.log)
            const long t96160 = (long)((d.M + 95) / 96) * ((d.N + 159) / 160);
            // Round 6, COLD weights (profiles/r06_lab_cold_weights.log: each launch of a shape reads another weight tensor, >= 400 MB in
            // rotation, as inside the step, where a launch's weights were last touched 1.7 GB of other weights ago and come from HBM,
            // not from the 256 MB memory-side cache a back-to-back sweep over ONE tensor reads them from): cold, every launch costs
            // 3-15 us more, and the ranking moves towards FEWER workgroups re-reading a weight tile -- fewer K slices, wider tiles.
            //  * the 4x4-level convs (384 rows): 96x160 tiles x 8 slices = 256 workgroups, ONE round (29.5 / 44.6 us cold against 36.1 /
            //    48.2 for 128x128 x 16 slices; hot the two are level)
            //    (fewer rows -- a rank's share of the frames -- keep the one round: 256 / tiles slices, each >= 11 K tiles)
            if (d.tile == SEER_TILE_AUTO && d.mode == SEER_GEMM_CONV3X3 && d.M <= 384 && d.N % 160 == 0 && nk >= 160 && t96160 <= 32) {
                s = (int)(256 / t96160);
                while (s > 1 && nk / s < 11) s >>= 1;
                tile = SEER_TILE_G96x160_2;
            } else
            if (s128 > 1 && t128 * s128 >= split_accept && d.tile == SEER_TILE_AUTO) {
                s = s128;
                tile = SEER_TILE_G128x128_2;
            // (with COLD weights the 320 -> 320 conv, K = 2880, is faster unsplit -- 34.8 against 40.6 us -- and the longer ones keep their
            //  two slices: 60.9 against 63.7, 81.3 against 91.7; profiles/r06_lab_cold_train_convs.log)
            } else if (d.N == 320 && d.mode == SEER_GEMM_CONV3X3 && t96160 >= 128 && t96160 <= 256 && nk >= 80 &&
                       d.tile == SEER_TILE_AUTO) {
                s = 2;
                tile = SEER_TILE_G96x160_2;
            } else {
                if (blocks64 <= 160 && nk >= 160) s = blocks64 <= 40 ? 16 : 8;      // 4x4 / 8x8 level convs of a frame shard
                else if (blocks64 <= 160 && nk >= 40) s = nk / 20 < 8 ? nk / 20 : 8;
                else if (blocks64 <= 512 && nk >= 80) s = 4;
            }
        }
    }
    if (tile == SEER_TILE_AUTO) tile = SEER_TILE_G64x64_3;      // no tile rule above: the 64x64 ring runs the slices
    return {s, tile};
}

// the tile an unsplit, non-weight-stationary launch of `d` runs (d.tile, or the AUTO choice)
int resolve_tile(const seer_gemm_desc& d) {
    int tile = d.tile;
    if (tile == SEER_TILE_AUTO) {
        // from the MI355X sweep (profiles/r01_gemm_tile_sweep.log): LDS-direct 2-stage 128x128 wherever it fills the chip,
        // LDS-direct 3-stage 128x64 / 64x64 for narrow N or few rows once the K loop is long enough to amortise the ring
        // prologue, register-staged 64x64 for short K.
        const int nk = d.K / BK;
        const long t128 = (long)((d.M + 127) / 128) * ((d.N + 127) / 128) * d.batch;
        const long t12864 = (long)((d.M + 127) / 128) * ((d.N + 63) / 64) * d.batch;
        const int n128 = (d.N + 127) / 128 * 128;
        const bool n_fits_128 = (n128 - d.N) * 8 <= d.N;           // <= 12.5 % padded columns
        const long t128160 = (long)((d.M + 127) / 128) * ((d.N + 159) / 160) * d.batch;
        const long t96160 = (long)((d.M + 95) / 96) * ((d.N + 159) / 160) * d.batch;
        // (12 288 rows x 320 -- one CFG half, or the b = 1 fine-tuning step -- are 256 tiles of 96x160: one round; 16.2 / 28.6 / 12.9 us
        //  against 19.6 / 33.9 / 15.1 on 128x64 with cold weights, r06_lab_cold_train.log)
        if ((d.N == 320 || d.N == 960) && nk >= 5 && (t128160 >= 256 || (d.N == 320 && t96160 >= 224 && t96160 <= 256)) &&
            !(d.epilogue & SEER_EPI_GEGLU)) {
            // (with the fast epilogue the 160-wide tiles also win at K = 320 .. 960, where the register-staged 64x64 tile used to:
            //  projections of the 320-wide level 17.5 -> 15.6 / 14.4 -> 12.0 us, its 1x1 shortcuts 20.0 -> 16.2 / 26.5 -> 20.6, and
            //  its q|k|v projection, N = 960 = 6 x 160, 32.7 (weight-stationary) -> 26.4: profiles/r02_tile_sweep_fastepi.log)
            // N = 320 in two 160-wide tiles: no padded columns, 0.45x the L2->LDS traffic of 64x64.  Rows per tile: whichever
            // of 128 / 96 leaves the last round of tiles fuller -- 24 576 rows (the 32x32 level at CFG batch 2) are 384 tiles
            // of 128 rows (1.5 per CU) but 512 of 96 rows (2 per CU): +13 % on the 320->320 conv (profiles/r01_tile96.log)
            auto fill = [](long t) { return (double)t / (256.0 * (double)((t + 255) / 256)); };
            tile = fill(t96160) > fill(t128160) + 0.05 ? SEER_TILE_G96x160_2 : SEER_TILE_G128x160_2;
            // the rotary epilogue (temporal q|k|v) reads a (cos, sin) row per output row: fewer, taller tiles re-read less of the
            // table -- 24 576 x 960 x 320: 30.0 us on 128x160 against 34.8 on 96x160 (profiles/r03_tile_ab_rotary.log)
            if ((d.epilogue & SEER_EPI_ROTARY) && t128160 >= 256) tile = SEER_TILE_G128x160_2;
        }
        else if ((d.epilogue & SEER_EPI_ROTARY) && d.N == 1920 && nk >= 5 && (long)((d.M + 95) / 96) * 12 * d.batch >= 256)
            tile = SEER_TILE_G96x160_2;      // 6 144 x 1 920 x 640 rotary: 24.0 us against 26.8 on 128x128 (same log)
        // (cold weights, r06_lab_cold_weights.log: with a short K loop the fuller last round of 96-row tiles does not pay for their extra
        //  weight reads -- the 16x16-level q|k|v projection, 6144 x 1920 x 640: 21.5 us on 128x128 against 24.4 cold, 20.8 / 19.2 hot)
        else if (t128 >= 256 && n_fits_128 && d.N >= 640 && nk <= 10 && d.mode == SEER_GEMM_PLAIN && !(d.epilogue & SEER_EPI_GEGLU))
            tile = SEER_TILE_G128x128_2;
        else if (t128 >= 256 && n_fits_128 && d.N >= 640) {
            // 128x128, unless 96-row tiles leave the last round of resident workgroups (two per CU) clearly fuller: the q|k|v
            // projections of the 8x8 / 16x16 level are 360 / 720 tiles of 128 rows (0.70 of one / two rounds) but 480 / 960 of 96
            // rows (0.94): 22.0 -> 19.0, 23.1 -> 20.2 (rotary), 22.3 -> 20.9 us (profiles/r04_plain_tile_sweep.log)
            const long t96128 = (long)((d.M + 95) / 96) * ((d.N + 127) / 128) * d.batch;
            auto fill2 = [](long t) { return (double)t / (512.0 * (double)((t + 511) / 512)); };
            tile = (d.mode == SEER_GEMM_PLAIN && fill2(t96128) > fill2(t128) + 0.15) ? SEER_TILE_G96x128_2 : SEER_TILE_G128x128_2;
        }
        // a conv whose 128x128 grid just misses one round of the chip but whose 96x128 grid fills it (the 16x16-level 320 -> 640
        // conv: 240 / 320 tiles): 34.5 against 45.0 us on 128x64 (profiles/r04_conv_tile_sweep.log); plain GEMMs of those sizes stay
        // on 128x64 (ff.net.2 at that level: 34.0 against 31.5, r04_ff2_tile_sweep.log)
        // ... unless 96x160 tiles make exactly one round of the chip (that conv: 256 tiles; 35.0 against 41.7 us with cold weights,
        // r06_lab_cold_weights.log)
        else if (d.mode == SEER_GEMM_CONV3X3 && d.N % 160 == 0 && d.N >= 640 && nk >= 40 &&
                 (long)((d.M + 95) / 96) * (d.N / 160) * d.batch >= 224 && (long)((d.M + 95) / 96) * (d.N / 160) * d.batch <= 256)
            tile = SEER_TILE_G96x160_2;
        else if (d.mode == SEER_GEMM_CONV3X3 && n_fits_128 && d.N >= 640 && t128 >= 192 && nk >= 40 &&
                 (long)((d.M + 95) / 96) * ((d.N + 127) / 128) * d.batch >= 256)
            tile = SEER_TILE_G96x128_2;
        // cold weights (r06_lab_cold_weights.log): a 128x128 grid that almost fills one round (200-255 tiles: the 16x16-level projections,
        // shortcuts and ff.net.2 | proj_out, 6144 rows x 640) beats twice as many 128x64 tiles -- 10.2 / 16.5 / 22.0 / 34.1 us against 11.6 /
        // 19.2 / 26.5 / 38.7 (hot: level); and where the 128x64 grid itself is 200-255 tiles (the 8x8-level projections and shortcuts,
        // 1536 rows x 1280) it beats the 64x64 ring: 12.5 / 20.6 against 13.7 / 24.9
        else if (d.mode == SEER_GEMM_PLAIN && n_fits_128 && d.N >= 640 && t128 >= 200 && nk >= 10) tile = SEER_TILE_G128x128_2;
        else if (d.mode == SEER_GEMM_PLAIN && n_fits_128 && d.N >= 640 && t128 < 200 && nk >= 10 &&
                 (long)((d.M + 95) / 96) * ((d.N + 127) / 128) * d.batch >= 200 && (long)((d.M + 95) / 96) * ((d.N + 127) / 128) * d.batch <= 256)
            tile = SEER_TILE_G96x128_2;         // 768 x 3840 x 1280 (b = 1 step, 8x8 level): 240 tiles, 14.9 against 20.6 us cold on 128x64
        else if (d.mode == SEER_GEMM_PLAIN && t12864 >= 200 && t12864 < 256 && nk >= 10) tile = SEER_TILE_G128x64_3;   // (3072 x 640 x 640: 7.7 against 10.5)
        else if (t12864 >= 256 && nk >= 5) tile = SEER_TILE_G128x64_3;   // (K = 320 too: 8.9 vs 9.7 us on 12 288 x 320, r02_half_rows.log)
        else if (nk >= 64) tile = SEER_TILE_G64x64_5;        // long K on few tiles: deeper ring
        else if (nk >= 12) tile = SEER_TILE_G64x64_3;
        else tile = SEER_TILE_64x64;
    }
    return tile;
}

// The 256 x 320 tile kernel (gemm_t320.hip): 0 = this launch does not go there, else the number of K slices it runs with
// (reduced inside the launch; needs desc.workspace and desc.sync).
//
// AUTO takes it where a cost model calibrated on MI355X (profiles/r04_t320_*.log) puts it ahead of the smaller tiles:
//   t = rounds * (K tiles per slice * 1.9 us [2.0 conv] + 7 us of prologue / epilogue [12 GEGLU]) + slab bytes / 4.3 TB/s + 3 us
// rounds = ceil(tiles * S / 256 CUs); slab bytes = 2 * tiles * S * 320 KB when S > 1 -- the partial tiles of a split launch go
// through the fabric (write-through stores, sc1 loads) at HBM-like rates whatever the split, which is what keeps the big tile
// away from the few-tile shapes of a 32x32-latent step: 256 workgroups x 320 KB x 2 = 164 MB = 38 us per split launch.
// The smaller tiles are priced at the best rate they reach on these shape classes (0.78-1.1 PFLOP/s): the big tile is only
// chosen where it beats that optimistic figure.
double t320_model_us(const seer_gemm_desc& d, int S) {
    const int nb = (d.mode == SEER_GEMM_CONV3X3 && d.upsample == 2) ? 4 : (d.batch > 1 ? d.batch : 1);
    const int tiles = ((d.M + 255) / 256) * (d.N / 320) * nb, nk = d.K / BK;
    const int rounds = (tiles * S + 255) / 256;
    const double t_iter = d.mode == SEER_GEMM_CONV3X3 ? 2.0 : 1.9;
    const double slab = S > 1 ? 2.0 * tiles * S * 327680.0 / 4.3e6 : 0.0;
    const double fixed = (d.epilogue & SEER_EPI_GEGLU) ? 12.0 : 7.0;      // prologue + epilogue of a tile (the erf epilogue: +5 us)
    return rounds * (((nk + S - 1) / S) * t_iter + fixed) + slab + 3.0;
}
int t320_best_split(const seer_gemm_desc& d) {
    static const int cand[] = {1, 2, 3, 4, 5, 6, 8, 10, 12, 16};
    const int nk = d.K / BK;
    int best = 1;
    double tb = t320_model_us(d, 1);
    for (int S : cand) {
        if (S > nk / 4) break;                   // a slice keeps at least four K tiles
        const double t = t320_model_us(d, S);
        if (t < tb) { tb = t; best = S; }
    }
    return best;
}
int t320_plan(const seer_gemm_desc& d, bool assume_buffers) {
    if (d.rowstat || d.ln_rowstat) return 0;          // row statistics / folded LayerNorm live in the tile kernel
    if (d.tile != SEER_TILE_T256x320 && d.tile != SEER_TILE_AUTO) return 0;
    if (d.mode != SEER_GEMM_PLAIN && d.mode != SEER_GEMM_CONV3X3) return 0;
    if (!seer_gemm_t320_eligible(d)) return 0;
    const bool geglu = (d.epilogue & SEER_EPI_GEGLU) != 0;
    const bool phases = d.mode == SEER_GEMM_CONV3X3 && d.upsample == 2;
    const bool can_split = !geglu && d.batch <= 1 && !phases && d.splits != 1;
    if (d.tile == SEER_TILE_T256x320) {
        if (!can_split) return 1;
        const int nk = d.K / BK;
        int s = d.splits > 1 ? d.splits : t320_best_split(d);
        if (s > nk / 4) s = nk / 4;
        if (s > 16) s = 16;
        if (s < 1) s = 1;
        const bool room = d.workspace && d.workspace_bytes >= seer_gemm_t320_workspace_bytes(d, s) && d.sync &&
                          d.sync_bytes >= seer_gemm_t320_sync_bytes(d, s);
        return (!assume_buffers && s > 1 && !room) ? 1 : s;      // asked for by name without room to split: run it unsplit
    }
    // AUTO
    if (d.M % 256 || d.splits > 1) return 0;          // (ragged row tiles and explicit split requests stay with the smaller tiles)
    // AUTO never splits K on this kernel: the in-launch reduction waits for peer workgroups, which is only safe when this process
    // has the GPU to itself (gemm_t320.hip); ask for SEER_TILE_T256x320 + splits by name where that holds
    const double t = t320_model_us(d, 1);
    const double flops = 2.0 * d.M * d.N * (double)d.K * (phases ? 4 : d.batch > 1 ? d.batch : 1);
    // FLOP per us.  (Convs: since the small tiles' gather lost its address arithmetic they reach 1.0-1.2 PFLOP/s on long-K convs
    // with many rows -- profiles/r04_t320_recalibration.log -- and the big tile is rarely ahead there.)
    const double rate = d.mode == SEER_GEMM_CONV3X3 ? 1.10e9 : geglu ? 0.78e9 : 0.85e9;
    return t < flops / rate ? 1 : 0;
}

// what the plan has to know about a tile instantiation (bm == 0: not a tile code)
struct tile_traits { int bm, bn; bool colsum_ok, ln_ok; };
tile_traits traits_of(int tile) {
    switch (tile) {
#define SEER_ROW(code, BM, BN, NS, WM, WN, MAY_SPLIT, UNIT) \
    case code: return {BM, BN, TileShape<BM, BN, NS, WM, WN>::colsum_ok, TileShape<BM, BN, NS, WM, WN>::ln_ok};
        SEER_GEMM_TILES(SEER_ROW)
#undef SEER_ROW
        default: return {};
    }
}

// the launch of a tile code: its row's unit holds the kernels (split-K, d.splits > 1: the K slices)
int launch_tiles(int tile, bool f16, const seer_gemm_desc& d, hipStream_t st) {
    switch (tile) {
#define SEER_ROW(code, BM, BN, NS, WM, WN, MAY_SPLIT, UNIT)                                                    \
    case code:                                                                                                 \
        static_assert(UNIT >= 0 && UNIT < SEER_GEMM_TILE_UNITS && (!MAY_SPLIT || (WM == 2 && WN == 2)), #code); \
        return seer_gemm_tiles_launch<UNIT>(tile, f16, d, st);
        SEER_GEMM_TILES(SEER_ROW)
#undef SEER_ROW
        default: return SEER_EINVAL;
    }
}

// ---- folded LayerNorm (seer_gemm_desc::rowstat / ln_rowstat): such launches stay on the tile kernel, unsplit, with a staged
// bf16 output.  Can `tile` carry the row statistics `d` asks for?
bool ln_resolve(const seer_gemm_desc& d, const tile_traits& tile) {
    const bool geglu = (d.epilogue & SEER_EPI_GEGLU) != 0;
    if (d.mode != SEER_GEMM_PLAIN || d.batch > 1 || (d.epilogue & (SEER_EPI_OUT_F32 | SEER_EPI_TRANS_OUT | SEER_EPI_SILU | SEER_EPI_QUICKGELU)))
        return false;
    if (d.ldc % 8 || d.N % (geglu ? 16 : 8) || (reinterpret_cast<uintptr_t>(d.C) & 15)) return false;      // the kernel's `staged`
    if (d.rowstat && (geglu || d.colsum || d.colsum_fx)) return false;
    if (d.ln_rowstat && (d.A2 || !d.ln_wsum || (reinterpret_cast<uintptr_t>(d.ln_wsum) & 15))) return false;
    return tile.ln_ok;
}

// ---- the layout-invariant plan (SEER_TILE_AUTO_INVARIANT): the choices of choose_split() / resolve_tile() with the row count, the
// grid's fill and the device taken out.  What is left to decide on is mode, N, K, the epilogue flags, batch > 1 and the optional
// outputs asked, so rows 0 .. M-1 of a launch are the same bits whatever rows follow them.  One (N, K) class gets ONE choice for all
// the row counts it occurs with (the choice of the default plan at the step's CFG pair, or the one between pair and half); table in
// DESIGN.md.  No weight-stationary kernel, no 256 x 320 tile.
split_choice invariant_split(const seer_gemm_desc& d) {
    const int nk = d.K / BK;
    const bool can_split = d.batch == 1 && !(d.epilogue & (SEER_EPI_GEGLU | SEER_EPI_TRANS_OUT | SEER_EPI_ROTARY)) && d.splits != 1 &&
                           !d.rowstat && !d.ln_rowstat;
    if (!can_split) return {1, SEER_TILE_AUTO};
    if (d.splits > 1) return {d.splits < nk ? d.splits : nk, SEER_TILE_G64x64_3};      // slices asked for by number: the 64x64 ring, as AUTO
    const bool conv = d.mode == SEER_GEMM_CONV3X3;
    // the 8x8- and 4x4-level convs (N = 1280, K = 11 520 .. 23 040; 1536 / 384 rows at the CFG pair, 768 / 192 at one half): the
    // default plan runs 4 slices at 1536 rows and 8 at 384; four serve both
    if (conv && d.N % 160 == 0 && d.N >= 1024 && nk >= 88) return {4, SEER_TILE_G96x160_2};
    // the 16x16-level convs (N = 640) from K = 5760 up: unsplit at 6144 rows, 4 slices at 3072 today; two
    if (conv && d.N % 160 == 0 && d.N >= 512 && d.N < 1024 && nk >= 80) return {2, SEER_TILE_G96x160_2};
    // ff.net.2 | proj_out of the 8x8 level (N = 1280, K = 6400): 2 slices at 1536 rows, 4 at 768 today
    if (!conv && d.N % 128 == 0 && d.N >= 1024 && nk >= 88) return {4, SEER_TILE_G128x128_2};
    return {1, SEER_TILE_AUTO};
}

int invariant_tile(const seer_gemm_desc& d) {
    const int nk = d.K / BK;
    const bool geglu = (d.epilogue & SEER_EPI_GEGLU) != 0, rot = (d.epilogue & SEER_EPI_ROTARY) != 0;
    const int ring64 = nk >= 64 ? SEER_TILE_G64x64_5 : nk >= 12 ? SEER_TILE_G64x64_3 : SEER_TILE_64x64;
    const int n128 = (d.N + 127) / 128 * 128;
    const bool n_fits_128 = (n128 - d.N) * 8 <= d.N;
    int tile;
    if (d.mode == SEER_GEMM_CONV3X3) tile = d.N % 160 == 0 ? SEER_TILE_G96x160_2 : ring64;      // every conv of the UNet; conv_out (N = 4)
    else if (geglu) tile = SEER_TILE_G128x128_2;
    else if ((d.N == 320 || d.N == 960) && nk >= 5) tile = rot ? SEER_TILE_G128x160_2 : SEER_TILE_G96x160_2;     // the 32x32 level
    else if (d.N >= 1920 && n_fits_128) tile = (rot && d.N % 160 == 0) ? SEER_TILE_G96x160_2 : SEER_TILE_G128x128_2;   // q|k|v below it
    else if (d.N >= 512 && d.N < 1024 && d.N % 64 == 0 && nk >= 5) tile = SEER_TILE_G128x64_3;      // the 16x16 level's projections
    else tile = ring64;                                                                             // N = 1280: 8x8 and 4x4 level
    // an optional output the tile cannot carry moves the launch to the first tile that can (a function of what is asked, not of M)
    const int cand[] = {tile, SEER_TILE_G128x128_2, SEER_TILE_G128x64_3, SEER_TILE_G64x64_3, SEER_TILE_64x64};
    for (int c : cand) {
        const tile_traits t = traits_of(c);
        if (geglu && (t.bn / 32) % 2) continue;
        if ((d.rowstat || d.ln_rowstat) && !t.ln_ok) continue;
        if ((d.colsum || d.colsum_fx) && !t.colsum_ok) continue;
        return c;
    }
    return tile;
}

// ---- the launch plan: which kernel a descriptor gets, decided ONCE.  seer_gemm_bf16 launches it, the host queries read it.
struct gemm_plan {
    int status;                          // SEER_OK: seer_gemm_bf16 launches this plan; else the code it returns
    int kernel, tile, splits, reduce;    // SEER_GEMM_KERNEL_* (NONE: validate() refused, nothing else is set), the tile (under WS: the one
                                         // that runs if that launch hands back), K slices, SEER_GEMM_REDUCE_*; set whatever status says
    seer_gemm_desc d;                    // validated + normalised; d.tile: a tile kernel's code or AUTO; d.splits: still the request
    int colsum_rows, colsum_fx_rows;     // rows per partial of desc.colsum / desc.colsum_fx this launch leaves (0: it cannot)
    int tile_splits;                     // the K slices the smaller tiles would run this descriptor with (whichever kernel took it)
    bool ln_ok;                          // rowstat / ln_rowstat: asked for and carried
};

// assume_buffers: a size query -- plan as if workspace and sync will be provided; the launch plans with what it was given
gemm_plan plan_gemm(const seer_gemm_desc& in, bool assume_buffers) {
    gemm_plan p{};
    p.d = in;
    seer_gemm_desc& d = p.d;
    p.status = validate(d);
    if (p.status != SEER_OK) return p;
    const bool geglu = (d.epilogue & SEER_EPI_GEGLU) != 0, sums = d.colsum || d.colsum_fx, sums_stored = colsum_store_ok(d);
    const bool rows_ln = d.rowstat || d.ln_rowstat;       // row statistics / folded LayerNorm: tile kernel, unsplit
    // inv: the layout-invariant plan -- invariant_split() / invariant_tile() decide, nothing below looks at M or the workspace
    const bool inv = d.tile == SEER_TILE_AUTO_INVARIANT;
    const int s320 = inv ? 0 : t320_plan(d, assume_buffers);
    // an ineligible T256x320 request is AUTO; WS / AUTO_TILED are AUTO as far as tile and split-K selection go
    const int requested = d.tile == SEER_TILE_T256x320 ? SEER_TILE_AUTO : d.tile;
    d.tile = (requested == SEER_TILE_WS || requested == SEER_TILE_AUTO_TILED || inv) ? SEER_TILE_AUTO : requested;
    const split_choice sc = inv ? invariant_split(d) : choose_split(d);
    p.tile_splits = sc.splits;
    const bool room = d.workspace && d.workspace_bytes >= (int64_t)sc.splits * d.M * d.N * (int64_t)sizeof(float);
    // the smaller tiles slice K, and have the workspace for it (inv: sliced whatever was handed in; without room it is refused below)
    const bool slices = !s320 && sc.splits > 1 && (assume_buffers || room || inv);
    auto take = [&p](int kernel, int tile, int splits) { p.kernel = kernel; p.tile = tile; p.splits = splits; };
    tile_traits tile{};
    if (s320) {
        take(SEER_GEMM_KERNEL_T320, SEER_TILE_T256x320, s320);
    } else if (slices && !rows_ln) {
        take(SEER_GEMM_KERNEL_SPLITK, sc.tile, sc.splits);
        p.reduce = !d.colsum_fx ? (d.colsum ? SEER_GEMM_REDUCE_COLSUM : SEER_GEMM_REDUCE_PLAIN)
                 : splitk_fx_rows(d.M, inv) == 64 ? SEER_GEMM_REDUCE_COLSUM_FX64 : SEER_GEMM_REDUCE_COLSUM_FX32;
    } else {
        const bool ws = !sums && !rows_ln && seer_gemm_ws_eligible(d) &&
                        (requested == SEER_TILE_WS || (requested == SEER_TILE_AUTO && seer_gemm_ws_profitable(d)));
        take(ws ? SEER_GEMM_KERNEL_WS : SEER_GEMM_KERNEL_TILE, inv ? invariant_tile(d) : resolve_tile(d), 1);
        tile = traits_of(p.tile);
    }
    p.ln_ok = rows_ln && ln_resolve(d, tile);
    // rows per column-sum partial of this launch.  256 x 320: one per wave row (64 rows) unsplit, per 16-row fragment when K is split;
    // split-K: the strips of the reduce pass (the accumulating one owns bigger row blocks); else the tile's rows
    const bool split = p.kernel == SEER_GEMM_KERNEL_SPLITK;
    const int rows = !sums_stored ? 0 : s320 ? (d.M % 256 ? 0 : s320 > 1 ? 16 : 64)
                   : (p.kernel == SEER_GEMM_KERNEL_TILE && tile.colsum_ok) ? tile.bm : 0;
    // (slices && rows_ln: that launch stays unsplit and leaves TILE rows, but the queries have always answered with the strips there.
    //  No caller asks for both; kept as it was, to be changed with a fixture of its own.)
    p.colsum_rows = slices && sums_stored ? splitk_cs_rows(d.M, inv) : rows;
    p.colsum_fx_rows = slices && sums_stored ? splitk_fx_rows(d.M, inv) : rows;
    // what the launch cannot carry.  colsum_fx: no partial of this launch may straddle two batch elements
    const bool fx_bad = d.colsum_fx && (d.colsum || d.colsum_fx_reps < 1 || d.colsum_fx_rows <= 0 || d.M % d.colsum_fx_rows ||
                                        !p.colsum_fx_rows || d.colsum_fx_rows % p.colsum_fx_rows);
    const bool sums_bad = sums && (split ? (d.epilogue & (SEER_EPI_OUT_F32 | SEER_EPI_TRANS_OUT | SEER_EPI_GEGLU)) != 0 : !rows);
    // (tile / weight-stationary launches: a tile code; GEGLU has no conv form, and its value / gate n-tile pairs must sit in one wave)
    const bool tile_bad = !s320 && !split && (!tile.bm || (geglu && (d.mode == SEER_GEMM_CONV3X3 || (tile.bn / 32) % 2)));
    if (fx_bad || sums_bad || tile_bad || (rows_ln && !p.ln_ok)) p.status = SEER_EINVAL;
    if (inv) {
        if (split && !assume_buffers && !room) p.status = SEER_EINVAL;      // K slices without their workspace: an error, not an unsplit launch
        d.tile = SEER_TILE_AUTO_INVARIANT;                                  // the reduce pass reads the request (splitk_cs_rows)
    }
    return p;
}

}  // namespace

extern "C" int seer_gemm_plan(const seer_gemm_desc* desc, int32_t out[5]) {
    if (!desc || !out) return SEER_EINVAL;
    const gemm_plan p = plan_gemm(*desc, false);
    const bool ok = p.status == SEER_OK;          // a refused launch reports its status alone
    out[0] = p.status; out[1] = ok ? p.kernel : 0; out[2] = ok ? p.tile : 0; out[3] = ok ? p.splits : 0; out[4] = ok ? p.reduce : 0;
    return SEER_OK;
}

extern "C" int64_t seer_gemm_workspace_bytes(const seer_gemm_desc* desc) {
    if (!desc) return SEER_EINVAL;
    const gemm_plan p = plan_gemm(*desc, true);
    if (p.kernel == SEER_GEMM_KERNEL_NONE) return p.status;
    // (a launch that is planned for the 256 x 320 tile but arrives without `sync` falls back to the smaller tiles: room for both)
    const int s = p.tile_splits;
    const int64_t w320 = p.kernel == SEER_GEMM_KERNEL_T320 ? seer_gemm_t320_workspace_bytes(p.d, p.splits) : 0;
    const int64_t wold = s > 1 ? (int64_t)s * p.d.M * p.d.N * (int64_t)sizeof(float) : 0;
    return w320 > wold ? w320 : wold;
}

extern "C" int64_t seer_gemm_sync_bytes(const seer_gemm_desc* desc) {
    if (!desc) return SEER_EINVAL;
    const gemm_plan p = plan_gemm(*desc, true);
    return p.kernel == SEER_GEMM_KERNEL_T320 ? seer_gemm_t320_sync_bytes(p.d, p.splits) : 0;
}

// the three column-sum / row-statistics queries ask about the launch WITH that feature: address 16 stands for its buffer
extern "C" int32_t seer_gemm_colsum_rows(const seer_gemm_desc* desc) {
    if (!desc) return 0;
    seer_gemm_desc d = *desc;
    if (!d.colsum && !d.colsum_fx) d.colsum = reinterpret_cast<float*>(16);
    return plan_gemm(d, false).colsum_rows;
}

extern "C" int32_t seer_gemm_colsum_fx_layout(const seer_gemm_desc* desc, int32_t rows_per_batch, int32_t* reps) {
    if (reps) *reps = 1;
    if (!desc || rows_per_batch <= 0 || desc->M % rows_per_batch) return 0;
    seer_gemm_desc d = *desc;
    if (!d.colsum && !d.colsum_fx) d.colsum_fx = reinterpret_cast<int64_t*>(16);
    const int rows = plan_gemm(d, false).colsum_fx_rows;
    if (rows <= 0 || rows_per_batch % rows) return 0;
    const int adds = rows_per_batch / rows;       // adds per address and launch without replicas
    if (reps) *reps = adds <= 24 ? 1 : adds <= 48 ? 2 : adds <= 96 ? 4 : 8;
    return rows;
}

extern "C" int32_t seer_gemm_rowstat_ok(const seer_gemm_desc* desc) {
    if (!desc) return 0;
    seer_gemm_desc d = *desc;
    if (!d.rowstat) d.rowstat = reinterpret_cast<int64_t*>(16);
    return plan_gemm(d, false).ln_ok ? 1 : 0;
}

extern "C" int32_t seer_gemm_lnfold_ok(const seer_gemm_desc* desc) {
    if (!desc || !desc->ln_rowstat) return 0;
    // a launch AUTO gives to the weight-stationary kernel (the level-0 GEGLU projection) keeps LayerNorm + that kernel: faster
    // than the tile kernel with the fold (58.7 vs 65.5 us, profiles/r02_tile_sweep_fastepi.log, against 7.6 us of LayerNorm)
    seer_gemm_desc d = *desc;
    d.ln_rowstat = nullptr;
    if (d.tile == SEER_TILE_AUTO && plan_gemm(d, false).kernel == SEER_GEMM_KERNEL_WS) return 0;
    return plan_gemm(*desc, false).ln_ok ? 1 : 0;
}

extern "C" int seer_gemm_bf16(const seer_gemm_desc* desc, void* stream) {
    if (!desc) return SEER_EINVAL;
    gemm_plan p = plan_gemm(*desc, false);
    if (p.status != SEER_OK) return p.status;
    p.d.splits = p.splits;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool f16 = (p.d.epilogue & SEER_EPI_F16) != 0;
    switch (p.kernel) {
        case SEER_GEMM_KERNEL_T320: return seer_gemm_t320_launch(p.d, p.splits, st);
        case SEER_GEMM_KERNEL_SPLITK:
            if (const int rc = launch_tiles(p.tile, f16, p.d, st); rc != SEER_OK) return rc;
            return seer_gemm_reduce_launch(p.d, p.reduce, st);
        case SEER_GEMM_KERNEL_WS:
            if (const int rc = seer_gemm_ws_launch(p.d, st); rc != SEER_ENOSYS) return rc;
            [[fallthrough]];             // not on this device: the tile kernel takes it
        default:
            return launch_tiles(p.tile, f16, p.d, st);
    }
}
