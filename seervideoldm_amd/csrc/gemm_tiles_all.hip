// every row of gemm_tiles.h in one unit: measurement builds only (scripts/), linked in place of gemm_tiles_0 .. 5; not in the library
#include "gemm_tile_units.inc"
