// Cartesian slice x frequency mode, unit weights, rows above FSW_HUB_MAX_DEG: the backward of k_cart_giant_bwd<false>
// (embed_giant_cart_bwd.hip) with ONE (row, slice) line split over many workgroups.  gfx950.
//
// k_cart_giant_bwd gives a line to one workgroup of four wavefronts, which sorts its runs, merges them level by level and walks the
// sorted line tile by tile: one point cloud at S = 16 keeps 16 CUs busy, and the time is the latency of that chain.  Here every phase
// is a launch of its own whose grid covers (line, piece), from the same building blocks (wave_sort.h, merge_path64.h, fourier_coef.h):
//   k_split_bwd_runs    (group of four runs, line): a run per wavefront into the line's ping region (sorted_run.inc) -- phase A of
//                       k_cart_giant_bwd
//   k_split_bwd_level   one launch per level R = 2048, 4096, ..: (span of tile slots, line): the span's boundaries by binary search in
//                       the level's source region, its tiles merged into the other region, its share of the run without a partner
//                       copied (merge_path64_span.h).  After k levels the line lies in ping (k even) or pong (k odd)     -- phase B
//   k_split_bwd_walk    (tile of 256 threads x 16 consecutive ranks, line): phase C with the text k_cart_giant_bwd<false> runs
//                       (walk_unit.inc) and its order of accumulation -- a unit line needs no carry between tiles, c_t = t / D --,
//                       so gkey is bit-identical to it.  gkey is stored straight from the walk by entry index; the frequency gradients of a
//                       tile go to partial[line][tile][f] (no float atomic per tile)
//   k_split_bwd_finish  (frequency): the partial sums of all lines and tiles in a fixed order, one atomic per frequency into gfreq
// Consecutive launches in the caller's stream are the only synchronisation between workgroups: no spin barrier, no cooperative launch,
// no flag in memory.  The grids are sized by the longest row; a workgroup whose run, level, span or tile does not exist for ITS line
// leaves at once (workgroup-uniform, before any barrier), so a line runs exactly the levels of its own length and its output depends on
// the line only: not on the other rows, S, the grid or what the scratch held.  Every line owns its region of the scratch.
// The scratch and its query: embed_cart.h (CartSplitBwdPlan), include/fsw_hip.h (fsw_embed_cart_split_backward_scratch_bytes).
#include <algorithm>
#include "embed_cart.h"
#include "embed_launch.h"
#include "fourier_coef.h"
#include "merge_path64_span.h"
#include "sortnet.h"
#include "wave_sort.h"

namespace fsw {

namespace {

constexpr int kSbVT = 16;                           // the walk: consecutive ranks per thread, kGbVT[0] of k_cart_giant_bwd
constexpr int kSbFinishNT = 256;
constexpr int64_t kSbLevelWorkgroups = 512;         // a level's grid aims at this many workgroups (two resident per CU)
static_assert(kMp64Run == kCartMaxLine && kMp64NT == 4 * kWave && kMp64NT * kSbVT == kCartSplitBwdWalk && kCartMaxLine % kSbVT == 0,
              "a run is one wavefront's chunk; a thread's ranks end with the line");

struct CartSplitBwd {
  const int32_t* rowptr;
  const int32_t* col;
  const int32_t* perm;
  const int32_t* bin_start;
  const float* Xp;
  int64_t ldp;
  const float* freqs;
  int S, F;
  const float* g;
  int64_t ldg;
  int gcol0;
  float out_scale;
  float* gkey;
  int64_t ldk;
  float* gfreq;
  mp64_t* scratch;          // [nlines][2][line_cap]: ping, pong; line = (row within the class's bins) * S + s
  int64_t line_cap;         // words of a region: a multiple of kCartMaxLine, >= the longest row
  float* partial;           // [nlines][ntmax][F]
  int ntmax;                // walk tiles of the longest row
  int64_t nlines;
  int bin, min_degree;      // the rows: perm[bin_start[bin] ..] with at least min_degree neighbours
};

struct SbLine { int node, s, start, D, total; };
// the line's row (embed_cart.h: cart_row_at) with its slice and its whole runs; false for a row that k_cart_giant_bwd skips too
__device__ __forceinline__ bool sb_line(const CartSplitBwd& a, int64_t line, SbLine& l) {
  const int pbeg = a.bin_start[a.bin];
  cart_row_at(a, pbeg + (int)(line / a.S), l);
  l.s = (int)(line % a.S);
  const int64_t total64 = ((int64_t)l.D + kCartMaxLine - 1) / kCartMaxLine * kCartMaxLine;
  l.total = (int)total64;
  return l.D >= a.min_degree && total64 <= a.line_cap;
}
// where the line lies after k levels
__device__ __forceinline__ mp64_t* sb_region(const CartSplitBwd& a, int64_t line, int k) { return a.scratch + (2 * line + (k & 1)) * a.line_cap; }

// grid (ceil(runs of the longest row / 4), nlines): wavefront w sorts run 4 blockIdx.x + w
__global__ void __launch_bounds__(kMp64NT, 2) k_split_bwd_runs(const CartSplitBwd a) {
  constexpr int M = kCartLongM, CAP = kCartMaxLine;
  const int64_t line = blockIdx.y;
  const int lane = lane_id();
  SbLine l;
  if (!sb_line(a, line, l)) return;
  const int64_t c64 = ((int64_t)blockIdx.x * 4 + wave_id()) * CAP;
  if (c64 >= l.total) return;                                // no barrier in this kernel: a wavefront may leave alone
  const int c0 = (int)c64, D = l.D;
  const int32_t* colrow = a.col + l.start;
  const float* xs = a.Xp + l.s;
  {
    constexpr bool RUN_PAD = false;
    unsigned long long* const run_line = sb_region(a, line, 0);
#include "sorted_run.inc"
  }
}

// grid (ceil(tile slots of the longest row / span), nlines): span blockIdx.x of level k, runs of kMp64Run << k words
__global__ void __launch_bounds__(kMp64NT, 2) k_split_bwd_level(const CartSplitBwd a, int k, int span) {
  __shared__ mp64_t tk[kMp64TileLds];
  __shared__ int part[kMp64MaxSpan + 1];
  const int64_t line = blockIdx.y;
  SbLine l;
  if (!sb_line(a, line, l)) return;
  const int64_t R64 = mp64_level_run(k);
  if (R64 >= (int64_t)l.total) return;                       // not a level of this line
  const Mp64Level lv = mp64_level(l.total, (int)R64);
  Mp64Span sp;
  if (!mp64_span(l.total, lv, span, (int)blockIdx.x, sp)) return;
  const mp64_t* src = sb_region(a, line, k);
  mp64_t* dst = sb_region(a, line, k + 1);
  if (sp.nt > 0) mp64_merge_tiles(src, dst, l.total, lv, sp.t0, sp.nt, tk, part);
  mp64_copy_run(src, dst, sp.c0, sp.c1, (int)threadIdx.x);
}

// grid (ntmax, nlines): tile blockIdx.x of the sorted line, which lies where levels = mp64_num_levels(total) left it
__global__ void __launch_bounds__(kMp64NT, 2) k_split_bwd_walk(const CartSplitBwd a) {
  constexpr int VT = kSbVT, TILE = kMp64NT * VT, NW = 4;
  __shared__ float red[NW][kWave];
  const int64_t line = blockIdx.y;
  SbLine l;
  if (!sb_line(a, line, l)) return;
  const int t0 = (int)blockIdx.x * TILE;
  const int D = l.D, total = l.total, F = a.F;
  if (t0 >= D) return;
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const mp64_t* se = sb_region(a, line, mp64_num_levels(total));
  const double inv = 1.0 / (double)D;
  const float* grow = a.g + (int64_t)l.node * a.ldg + a.gcol0 + (int64_t)l.s * F;
  float* gk = a.gkey + (int64_t)l.start * a.ldk + l.s;
  float* prow = a.partial + ((int64_t)line * a.ntmax + blockIdx.x) * F;
  const int r0 = t0 + tid * VT;
  const bool live = t0 + w * kWave * VT < D;                 // this wavefront's ranks hold elements of the line (wave-uniform)
  float key[VT];
  int idx[VT];
#pragma unroll
  for (int j = 0; j < VT; ++j) {
    const mp64_t e = r0 < total ? se[r0 + j] : ~0ull;        // total is a multiple of VT: a thread's ranks lie in the line or past it
    key[j] = r0 + j < D ? from_orderable_bits((unsigned int)(e >> 32)) : 0.f;   // fill elements: no inf in the frequency sums
    idx[j] = (int)((unsigned int)e & 0x7fffffffu);
  }
  for (int fb = 0; fb < F; fb += kWave) {
    const int nf = min(kWave, F - fb);
    float gfl = 0.f;                                         // lane q: this wavefront's gfreq sum of frequency fb + q
    float G[VT];
#pragma unroll
    for (int j = 0; j < VT; ++j) G[j] = 0.f;
    if (live) {
      for (int q = 0; q < nf; ++q) {
#include "walk_unit.inc"
      }
    }
    // blocks of 64 frequencies add up in block order, as in k_cart_giant_bwd: the same thread wrote the entry in the block before
#pragma unroll
    for (int j = 0; j < VT; ++j) {
      if (idx[j] < D) {
        float* p = gk + (int64_t)idx[j] * a.ldk;
        *p = fb == 0 ? G[j] : *p + G[j];
      }
    }
    if (a.gfreq) {                                           // the tile's sums: wavefronts in order
      red[w][lane] = gfl;
      __syncthreads();
      if (tid < nf) prow[fb + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
      __syncthreads();                                       // red is rewritten by the next block of frequencies
    }
  }
}

// grid (F): frequency blockIdx.x; thread i sums the (line, tile) pairs i, i + 256, .. in that order, then lanes and wavefronts in order
__global__ void __launch_bounds__(kSbFinishNT) k_split_bwd_finish(const CartSplitBwd a) {
  __shared__ float red[kSbFinishNT / kWave];
  const int f = blockIdx.x, tid = threadIdx.x;
  const int64_t items = a.nlines * a.ntmax;
  float sum = 0.f;
  for (int64_t i = tid; i < items; i += kSbFinishNT) {
    const int64_t line = i / a.ntmax;
    const int tile = (int)(i - line * a.ntmax);
    SbLine l;
    if (sb_line(a, line, l) && (int64_t)tile * kCartSplitBwdWalk < l.D) sum += a.partial[i * a.F + f];
  }
  sum = wave_sum(sum);
  if (lane_id() == 0) red[wave_id()] = sum;
  __syncthreads();
  if (tid == 0) {
    float tot = 0.f;
#pragma unroll
    for (int u = 0; u < kSbFinishNT / kWave; ++u) tot += red[u];
    atomicAdd(a.gfreq + f, tot);
  }
}

}  // namespace

// unit weights with tau <= 1: the rows of the giant class of kCartLong[0], every line in its own region of c->scratch
int launch_cart_split_bwd(const fsw_cart_args* c, const CartSplitBwdPlan& p, hipStream_t stream) {
  const CartLongMode& m = kCartLong[0];
  if (p.lines <= 0) return 0;
  CartSplitBwd t;
  cart_fill_inputs(t, c);
  cart_fill_grads(t, c);
  t.scratch = (mp64_t*)c->scratch; t.line_cap = (int64_t)(p.line_bytes / kCartGiantBwdElemBytes);
  t.partial = (float*)((char*)c->scratch + p.partial_offset); t.ntmax = p.ntmax; t.nlines = p.lines;
  t.bin = m.giant_bin; t.min_degree = m.giant_min_degree;
  // lines <= 2 GiB / (two runs of the shortest row) = 3855 and line_cap <= 2 GiB / 16: every grid dimension fits
  const int64_t nruns = t.line_cap / kCartMaxLine;             // runs = tile slots of the longest row
  k_split_bwd_runs<<<dim3((unsigned)ceil_div(nruns, (int64_t)4), (unsigned)p.lines), kMp64NT, 0, stream>>>(t);
  FSW_LAUNCH_CHECK();
  // tile slots per workgroup of a level: about kSbLevelWorkgroups workgroups per launch.  The result does not depend on it
  const int span = (int)std::min<int64_t>(std::max<int64_t>(ceil_div(p.lines * nruns, kSbLevelWorkgroups), 1), kMp64MaxSpan);
  const dim3 spans((unsigned)ceil_div(nruns, (int64_t)span), (unsigned)p.lines);
  for (int k = 0; mp64_level_run(k) < t.line_cap; ++k) {
    k_split_bwd_level<<<spans, kMp64NT, 0, stream>>>(t, k, span);
    FSW_LAUNCH_CHECK();
  }
  k_split_bwd_walk<<<dim3((unsigned)p.ntmax, (unsigned)p.lines), kMp64NT, 0, stream>>>(t);
  FSW_LAUNCH_CHECK();
  if (t.gfreq) {
    k_split_bwd_finish<<<(unsigned)c->F, kSbFinishNT, 0, stream>>>(t);
    FSW_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace fsw
