// One build unit of the tile kernel: the kernels of the rows of gemm_tiles.h whose unit is SEER_GEMM_TILE_UNIT, both storage types,
// and the unit's launcher.  gemm_tiles_<u>.hip are one define and this include each, so that every unit is a source of its own
// (the build keeps one object and one device assembly per source).  Without SEER_GEMM_TILE_UNIT (gemm_tiles_all.hip) every row
// is emitted into ONE unit: the measurement builds of scripts/ need that (SEER_GEMM_STAMPS writes __device__ arrays from inside
// the kernels, and the library is built without relocatable device code), linked in place of all the gemm_tiles_<u> objects.
#include "gemm_tile_kernel.h"

namespace {

template <int BM, int BN, int NS, int WM, int WN, bool MAY_SPLIT, bool F16>
int launch_row(const seer_gemm_desc& d, hipStream_t st) {
    if (d.splits <= 1) return launch_tile<BM, BN, NS, WM, WN, F16>(d, st);
    if constexpr (MAY_SPLIT) return launch_split_tile<BM, BN, NS, F16>(d, st);
    return SEER_EINVAL;
}

}  // namespace

template <int U>
int seer_gemm_tiles_launch(int tile, bool f16, const seer_gemm_desc& d, hipStream_t st) {
    switch (tile) {
#define SEER_ROW(code, BM, BN, NS, WM, WN, MAY_SPLIT, UNIT)                                                                   \
    case code:                                                                                                                \
        if constexpr (UNIT == U) return f16 ? launch_row<BM, BN, NS, WM, WN, MAY_SPLIT, true>(d, st)                          \
                                            : launch_row<BM, BN, NS, WM, WN, MAY_SPLIT, false>(d, st);                        \
        break;
        SEER_GEMM_TILES(SEER_ROW)
#undef SEER_ROW
    }
    return SEER_EINVAL;
}

#ifdef SEER_GEMM_TILE_UNIT
static_assert(SEER_GEMM_TILE_UNIT >= 0 && SEER_GEMM_TILE_UNIT < SEER_GEMM_TILE_UNITS, "no such unit in gemm_tiles.h");
template int seer_gemm_tiles_launch<SEER_GEMM_TILE_UNIT>(int, bool, const seer_gemm_desc&, hipStream_t);
#else
static_assert(SEER_GEMM_TILE_UNITS == 6, "one explicit instantiation per unit below");
template int seer_gemm_tiles_launch<0>(int, bool, const seer_gemm_desc&, hipStream_t);
template int seer_gemm_tiles_launch<1>(int, bool, const seer_gemm_desc&, hipStream_t);
template int seer_gemm_tiles_launch<2>(int, bool, const seer_gemm_desc&, hipStream_t);
template int seer_gemm_tiles_launch<3>(int, bool, const seer_gemm_desc&, hipStream_t);
template int seer_gemm_tiles_launch<4>(int, bool, const seer_gemm_desc&, hipStream_t);
template int seer_gemm_tiles_launch<5>(int, bool, const seer_gemm_desc&, hipStream_t);
#endif
