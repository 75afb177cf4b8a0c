// unit 2 of the tile kernel: the rows of gemm_tiles.h marked 2 (see gemm_tile_units.inc)
#define SEER_GEMM_TILE_UNIT 2
#include "gemm_tile_units.inc"
