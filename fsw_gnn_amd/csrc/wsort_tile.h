// What the wave-sort kernels of diagonal mode share (k_embed_wsort: embed_wsort.hip, k_embed_wsort_bwd: embed_wsort_bwd.hip,
// k_embed_wsort_w_bwd: embed_w_sort_bwd.hip): a workgroup takes one row and walks its slices in groups of SC; the group's keys lie
// transposed in an LDS tile [SC][LINE], one line per slice, and one wavefront sorts and reads out one line.  gfx950.
// Here: the constants and the row mass.  The gather of a slice group is included text (wsort_gather.inc).  DESIGN.md, "Steps that the
// diagonal-mode kernels share", lists the steps that stay hand-kept copies because no shared form compiles to the same code.
#pragma once
#include "fsw_common.h"

namespace fsw {

constexpr int kWsSplitY = 4;   // workgroups sharing one row (grid.y; they take disjoint slice groups)

// LDS elements of one line of M elements per lane: one pad per M elements (lane l starts at l (M + 1)), odd stride
template <int M>
constexpr int ws_line() { return M * kWave + kWave + 1; }

// Slices per group: the float lines that fit an LDS budget beside `reserved_bytes` of other arrays (results, the row's weights,
// accumulators), in whole rounds of the four wavefronts, 64 at the most.  0: not even one line fits.
template <int M>
constexpr int ws_slices(int lds_bytes, int reserved_bytes) {
  const int lines = (lds_bytes - reserved_bytes) / 4 / ws_line<M>();
  return lines >= 64 ? 64 : (lines >= 4 ? (lines & ~3) : lines);
}

// The row mass in float64 from the four wavefronts' partial sums (msum[wave], written before the caller's barrier)
__device__ __forceinline__ double ws_row_mass(const double* msum) { return msum[0] + msum[1] + msum[2] + msum[3]; }

}  // namespace fsw
