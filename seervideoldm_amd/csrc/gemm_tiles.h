// The tile table of seer_gemm_bf16 and what the planner (gemm.hip), the tile kernel (gemm_tile_kernel.h), its build units
// (gemm_tile_units.inc) and the split-K reduce pass (gemm_reduce.hip) have to agree on.  No kernel in here: host code may include it.
#pragma once
#include "seer_common.h"

// ---- the tiles: one row per instantiation of seer_gemm_kernel.  A tile is added or retired by touching its row.
//   X(SEER_TILE_* code, BM, BN, NS, WM, WN, may_split, unit)
// NS == 0: register-staged double buffer (global_load -> VGPR -> ds_write), one barrier per K tile.
// NS >= 2: NS-stage ring filled by global_load_lds (16 B per lane straight into LDS, no VGPR / ds_write), NS-1 tiles in
//          flight across raw s_barriers behind counted s_waitcnt vmcnt(N).  Same LDS image either way.
// WM x WN: the wave grid.  WN = 2: WM = 2 -> 256 threads, 4 -> 512 threads (256-row tiles, same 64x64 wave tile).
// WM = 2, WN = 4 with a 256 x 256 tile is the 8-phase ping-pong kernel (TileShape::PP8): 128 x 64 wave tiles, its own main loop.
// may_split: the tile also exists in its split-K form (the four tiles choose_split() / invariant_split() hand out).
// unit: the translation unit gemm_tiles_<unit>.hip that emits the row's kernels, both storage types.  The units compile in
//       parallel, so the column balances compile time (the device assembly of a row is a fair measure: 25 000 lines for a 64 x 64
//       ring, 103 000 for the 256 x 256 tile; profiles/gemm_split.md), nothing else.
#define SEER_GEMM_TILES(X)                            \
    X(SEER_TILE_128x128, 128, 128, 0, 2, 2, false, 4)    \
    X(SEER_TILE_128x64, 128, 64, 0, 2, 2, false, 2)      \
    X(SEER_TILE_64x64, 64, 64, 0, 2, 2, true, 3)         \
    X(SEER_TILE_G128x128_2, 128, 128, 2, 2, 2, true, 1)  \
    X(SEER_TILE_G128x128_3, 128, 128, 3, 2, 2, false, 2) \
    X(SEER_TILE_G128x64_3, 128, 64, 3, 2, 2, false, 1)   \
    X(SEER_TILE_G64x64_3, 64, 64, 3, 2, 2, true, 5)      \
    X(SEER_TILE_G64x64_4, 64, 64, 4, 2, 2, false, 0)     \
    X(SEER_TILE_G64x64_5, 64, 64, 5, 2, 2, false, 4)     \
    X(SEER_TILE_G128x64_4, 128, 64, 4, 2, 2, false, 2)   \
    X(SEER_TILE_G128x160_2, 128, 160, 2, 2, 2, false, 5) \
    X(SEER_TILE_G64x160_3, 64, 160, 3, 2, 2, false, 1)   \
    X(SEER_TILE_G256x128_2, 256, 128, 2, 4, 2, false, 3) \
    X(SEER_TILE_G256x64_3, 256, 64, 3, 4, 2, false, 0)   \
    X(SEER_TILE_G256x256_2, 256, 256, 2, 2, 4, false, 0) \
    X(SEER_TILE_G96x160_2, 96, 160, 2, 2, 2, true, 5)    \
    X(SEER_TILE_G96x160_3, 96, 160, 3, 2, 2, false, 3)   \
    X(SEER_TILE_G96x128_2, 96, 128, 2, 2, 2, false, 4)
constexpr int SEER_GEMM_TILE_UNITS = 6;

// the launcher of unit U (gemm_tile_units.inc): the kernel behind `tile`, bf16 or IEEE-half storage; d.splits > 1: the K slices of
// the split-K form, whose second pass is seer_gemm_reduce_launch.  SEER_EINVAL for a tile (or form) the unit does not hold.
template <int U>
int seer_gemm_tiles_launch(int tile, bool f16, const seer_gemm_desc& d, hipStream_t st);
// gemm_reduce.hip: the second pass of a split-K launch, `reduce` = SEER_GEMM_REDUCE_*
int seer_gemm_reduce_launch(const seer_gemm_desc& d, int reduce, hipStream_t st);

bool seer_gemm_ws_eligible(const seer_gemm_desc& d);             // gemm_ws.hip: weight-stationary persistent kernel (short K)
bool seer_gemm_ws_profitable(const seer_gemm_desc& d);
int seer_gemm_ws_launch(const seer_gemm_desc& d, hipStream_t st);
bool seer_gemm_t320_eligible(const seer_gemm_desc& d);           // gemm_t320.hip: 256 x 320 tile, in-launch split-K
int64_t seer_gemm_t320_workspace_bytes(const seer_gemm_desc& d, int splits);
int64_t seer_gemm_t320_sync_bytes(const seer_gemm_desc& d, int splits);
int seer_gemm_t320_launch(const seer_gemm_desc& d, int splits, hipStream_t st);

// rows per partial of the split-K reduce passes with column sums (gemm_reduce.hip; the planner answers the host queries with them)
// (inv: the layout-invariant plan, SEER_TILE_AUTO_INVARIANT -- one row block whatever M; the launch hands the request on in desc.tile)
__host__ __device__ inline int splitk_cs_rows(int M, bool inv) { return (inv || M >= 2048) ? 16 : 4; }
__host__ inline int splitk_fx_rows(int M, bool inv) { return (!inv && M >= 1024) ? 64 : 32; }

namespace {

constexpr int BK = 64;

// The shape of one tile instantiation: its threads and its LDS layout, the only place their formulas are written.  The K-loop ring
// is [stage][A tile BM x 64 | B tile BN x 64] bf16; the epilogue stages the bf16 C tile over it (geglu: the GEGLU form, whose
// output tile is BN / 2 wide), then the column-sum scratch, then 4096 bytes on, the row statistics of a folded LayerNorm.
template <int BM_, int BN_, int NS_, int WM_ = 2, int WN_ = 2>
struct TileShape {
    static constexpr int BM = BM_, BN = BN_, NS = NS_, WM = WM_, WN = WN_;
    static constexpr int NT = 64 * WM * WN;                     // threads per block
    static constexpr int STAGE = (BM + BN) * BK;                // elements per stage
    static constexpr int RING_BYTES = (NS == 0 ? 2 : NS) * STAGE * (int)sizeof(bf16);
    static constexpr bool PP8 = WM == 2 && WN == 4 && BM == 256 && BN == 256;
    static constexpr bool GEGLU_OK = ((BN / 32) % 2) == 0;      // value / gate n-tile pairs must sit in one wave
    static constexpr int bno(bool geglu) { return geglu ? BN / 2 : BN; }      // output columns of the block tile
    // staged row pitch in bytes: 16 B of padding spreads the 16 rows a wave instruction writes over the banks; when the padded
    // tile does not fit (256 x 256 bf16 = the whole 128 KB ring) the rows are dense and the 16-byte chunk index is XORed with
    // the row instead
    static constexpr bool cswz(bool geglu) { return BM * (bno(geglu) * 2 + 16) > 2 * STAGE * (int)sizeof(bf16); }
    static constexpr int cpitch(bool geglu) { return bno(geglu) * 2 + (cswz(geglu) ? 0 : 16); }
    static constexpr int lnrow_off(bool geglu) { return BM * cpitch(geglu) + 4096; }
    // whether the tile can produce column sums (seer_gemm_desc::colsum): the staged C tile plus the row-segment partials have to
    // fit in the K-loop LDS, one thread per output column adds them
    static constexpr bool colsum_ok = !PP8 && BN <= NT && BM * cpitch(false) + (NT / (BN / 2)) * BN * 8 <= RING_BYTES;
    // whether the tile can take part in a folded LayerNorm (seer_gemm_desc::rowstat / ln_rowstat): the consumer parks
    // (mean * rstd, rstd) of its BM rows behind the staged C tile and the column-sum scratch
    static constexpr bool ln_ok = !PP8 && BM <= NT && lnrow_off(false) + BM * 8 <= RING_BYTES;
};

}  // namespace
