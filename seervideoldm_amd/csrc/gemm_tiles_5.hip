// unit 5 of the tile kernel: the rows of gemm_tiles.h marked 5 (see gemm_tile_units.inc)
#define SEER_GEMM_TILE_UNIT 5
#include "gemm_tile_units.inc"
