// unit 1 of the tile kernel: the rows of gemm_tiles.h marked 1 (see gemm_tile_units.inc)
#define SEER_GEMM_TILE_UNIT 1
#include "gemm_tile_units.inc"
