// unit 0 of the tile kernel: the rows of gemm_tiles.h marked 0 (see gemm_tile_units.inc)
#define SEER_GEMM_TILE_UNIT 0
#include "gemm_tile_units.inc"
