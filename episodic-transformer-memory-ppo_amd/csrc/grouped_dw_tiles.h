// The workgroup -> tile map of the grouped weight-gradient launches (grouped_dw.hip), callable from both sides: the kernels number
// their tiles with it and etm_grouped_dw_tile_map evaluates the same body on the host, so that a test can walk every tile count.
#pragma once
#include <hip/hip_runtime.h>

// Workgroup b runs on XCD b % 8 (the dispatcher deals consecutive workgroups round the eight dies, each with an L2 of its own), and the
// 9 - 12 tiles of one problem read the SAME two operands: dealt round the dies as they come, every tile pulls its operand columns
// through its die's L2 by itself (PMC rounds 5 / 6: 397 MB fetched per launch against 226 MB of operands even without any sharing).  So
// the tiles are renumbered: die x takes the contiguous run [x T / 8, (x + 1) T / 8) of the launch's tiles -- the tiles of a problem sit on
// one die (two at a run's ends) and walk the sample rows together through its L2.  A bijection for every T (tests/test_grouped_dw_host.py
// walks T = 1 .. 4096 through etm_grouped_dw_tile_map); the few blocks of a die that has one workgroup more than its run has tiles
// take the tiles left over on other dies.
__host__ __device__ __forceinline__ int gd_tile_of_block(int b, int n_tiles) {
  const int x = b & 7, slot = b >> 3;
  const int lo = (int)(((long long)x * n_tiles) >> 3), hi = (int)(((long long)(x + 1) * n_tiles) >> 3);      // this die's run
  const int full = n_tiles >> 3;
  const int wgs = full + (x < (n_tiles & 7) ? 1 : 0);        // workgroups the dispatcher gives die x
  const int run = hi - lo;
  if (slot < (run < wgs ? run : wgs)) return lo + slot;
  int k = 0;                                                 // index of this block among the leftover blocks
  for (int y = 0; y < x; ++y) {
    const int wy = full + (y < (n_tiles & 7) ? 1 : 0), ry = (int)(((long long)(y + 1) * n_tiles) >> 3) - (int)(((long long)y * n_tiles) >> 3);
    if (wy > ry) k += wy - ry;
  }
  k += slot - run;
  for (int y = 0; y < 8; ++y) {
    const int ly = (int)(((long long)y * n_tiles) >> 3), ry = (int)(((long long)(y + 1) * n_tiles) >> 3) - ly;
    const int wy = full + (y < (n_tiles & 7) ? 1 : 0);
    if (ry > wy) {
      if (k < ry - wy) return ly + wy + k;
      k -= ry - wy;
    }
  }
  return b;                                                  // (not reached: leftover blocks and leftover tiles are equally many)
}
