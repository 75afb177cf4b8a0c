// unit 4 of the tile kernel: the rows of gemm_tiles.h marked 4 (see gemm_tile_units.inc)
#define SEER_GEMM_TILE_UNIT 4
#include "gemm_tile_units.inc"
