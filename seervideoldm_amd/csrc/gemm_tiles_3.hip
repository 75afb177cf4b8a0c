// unit 3 of the tile kernel: the rows of gemm_tiles.h marked 3 (see gemm_tile_units.inc)
#define SEER_GEMM_TILE_UNIT 3
#include "gemm_tile_units.inc"
