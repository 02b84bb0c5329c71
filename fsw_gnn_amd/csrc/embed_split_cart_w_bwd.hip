// Cartesian slice x frequency mode, general weights (w != NULL or tau > 1), rows of FSW_CART_W_MAX_LINE neighbours and more: the backward
// of k_cart_giant_bwd<true> (embed_giant_cart_bwd.hip) with ONE (row, slice) line split over many workgroups.  gfx950.
//
// k_cart_giant_bwd<true> gives a line of D + 1 elements (the neighbours and the reference's pad element) to one workgroup of four
// wavefronts, which sorts its runs, merges them level by level and walks the sorted line tile by tile: one weighted point cloud at S = 16
// keeps 16 CUs busy.  Here every phase is a launch of its own whose grid covers (line, piece), from the same building blocks
// (wave_sort.h, merge_path64.h, merge_path64_span.h, fourier_coef.h):
//   k_splitw_bwd_mass    (run, row): the float64 sum of the weights of the entries [2048 p, 2048 p + 2048) into mass[row][p]; the row's
//                        mass m is the sum of its pieces in piece order (w == NULL: every weight is 1).  m does not depend on the slice;
//                        the walk needs it for the pad element's weight max(tau - m, 0) and for 1 / max(m, tau)
//   k_splitw_bwd_runs    (group of four runs, line): phase A -- a run per wavefront into the line's ping region (sorted_run.inc, with
//                        the pad element)
//   k_splitw_bwd_level   one launch per level R = 2048, 4096, ..: (span of tile slots, line), as k_split_bwd_level of the unit form:
//                        mp64_span, mp64_merge_tiles, mp64_copy_run.  After k levels the line lies in ping (k even) or pong (k odd)
//   k_splitw_bwd_tsum    (walk tile, line): the float64 sum of the weights of the tile's 2048 ranks into tsum[line][tile]; the weights are
//                        re-read by entry index (w[start + idx], the pad weight for idx == D, 0 for fill)
//   k_splitw_bwd_walk    (tile of 256 threads x 8 consecutive ranks, line): the cumulative weight before the tile is the sum of the
//                        earlier tiles' tsum in tile order (float64); inside the tile phase C of k_cart_giant_bwd<true>: wave scan +
//                        wavefront offsets in float64, then the text that kernel runs per frequency (walk_weighted.inc).  gkey is
//                        stored straight from the walk by entry index (pad and fill elements store nothing); the frequency gradients of
//                        a tile go to partial[line][tile][f], the four wavefronts' sums added in wavefront order (no float atomic per tile).
//                        More than 64 frequencies: blocks of 64, the sums of a gkey entry added in block order by the thread that owns it
//   k_splitw_bwd_finish  (frequency): the partial sums of all lines and tiles in a fixed order, one atomic per frequency into gfreq
// Consecutive launches in the caller's stream are the only synchronisation between workgroups: no spin barrier, no cooperative launch,
// no flag in memory.  The grids are sized by the longest row; a workgroup whose run, level, span or tile does not exist for ITS line
// leaves at once (workgroup-uniform, before any barrier), and so does one whose row belongs to the class below, which shares the degree
// bin (k_cart_hub_w_bwd has written that row).  Every line owns its regions of the scratch and every word a phase reads was written by
// an earlier phase of the same call, so gkey of a line depends on the line only: not on S, the other rows, the grids, the span or what
// the scratch held.
// NOT bit-identical to k_cart_giant_bwd<true>: that kernel sums the row mass per wavefront over the chunks w, w + 4, .. and carries the
// cumulative weight from tile to tile as a running float64 sum of wavefront totals; here the mass is the sum of per-run pieces and the
// carry the sum of per-tile sums.  A last-bit change of 1 / max(m, tau) or of a cumulative weight can move a float32 gradient; both forms
// are within the project's bounds of the float64 backward (tests/test_hip_cart_split_w_bwd.py prints the difference; measured on its
// two graphs with random weights at 4 x 8: no entry differs, which is not asserted).
// The scratch and its query: embed_cart.h (CartSplitWBwdPlan), include/fsw_hip.h (fsw_embed_cart_split_w_backward_scratch_bytes).
#include <algorithm>
#include "embed_cart.h"
#include "embed_launch.h"
#include "fourier_coef.h"
#include "merge_path64_span.h"
#include "sortnet.h"
#include "wave_sort.h"

namespace fsw {

namespace {

constexpr int kSwbVT = 8;                            // the walk: consecutive ranks per thread, kGbVT[1] of k_cart_giant_bwd
constexpr int kSwbFinishNT = 256;
constexpr int64_t kSwbLevelWorkgroups = 512;         // a level's grid aims at this many workgroups (two resident per CU)
static_assert(kMp64Run == kCartMaxLine && kMp64NT == 4 * kWave && kMp64NT * kSwbVT == kCartSplitWBwdWalk && kCartMaxLine % kSwbVT == 0,
              "a run is one wavefront's chunk and one tile of the walk");

struct CartSplitWBwd {
  const int32_t* rowptr;
  const int32_t* col;
  const float* w;           // null with tau > 1: every weight is 1
  const int32_t* perm;
  const int32_t* bin_start;
  const float* Xp;
  int64_t ldp;
  const float* freqs;
  int S, F;
  float tau;
  const float* g;
  int64_t ldg;
  int gcol0;
  float out_scale;
  float* gkey;
  int64_t ldk;
  float* gfreq;
  mp64_t* scratch;          // [nlines][2][line_cap]: ping, pong; line = (row within the class's bins) * S + s
  int64_t line_cap;         // words of a region: a multiple of kCartMaxLine, > the longest row
  double* mass;             // [rows][tiles]
  double* tsum;             // [nlines][tiles]
  float* partial;           // [nlines][tiles][F]
  int tiles;                // runs = walk tiles of the longest line
  int64_t nlines;
  int bin, min_degree;      // the rows: perm[bin_start[bin] ..] with at least min_degree neighbours
};

struct SwbRow { int node, start, D, total; };
// the row (embed_cart.h: cart_row_at) with its line of D + 1 elements in whole runs; false for a row that k_cart_giant_bwd<true> skips too
__device__ __forceinline__ bool swb_row(const CartSplitWBwd& a, int64_t row, SwbRow& l) {
  cart_row_at(a, a.bin_start[a.bin] + (int)row, l);
  const int64_t total64 = ((int64_t)l.D + 1 + kCartMaxLine - 1) / kCartMaxLine * kCartMaxLine;
  l.total = (int)total64;
  return l.D >= a.min_degree && total64 <= a.line_cap;
}
// where the line lies after k levels
__device__ __forceinline__ mp64_t* swb_region(const CartSplitWBwd& a, int64_t line, int k) { return a.scratch + (2 * line + (k & 1)) * a.line_cap; }
// the row's mass: its pieces in piece order
__device__ __forceinline__ double swb_mass(const CartSplitWBwd& a, int64_t row, int total) {
  const double* p = a.mass + row * a.tiles;
  double m = 0.0;
  for (int q = 0; q < total / kCartMaxLine; ++q) m += p[q];
  return m;
}
// the weight of the element with entry index idx: a neighbour, the pad element, fill
__device__ __forceinline__ float swb_weight(const float* wrow, int idx, int D, float padw) {
  return idx < D ? (wrow ? wrow[idx] : 1.f) : (idx == D ? padw : 0.f);
}
// the same in float64 with the pad weight unrounded, for the float64 sums of the cumulative weight (fsw_common.h: pad_residual)
__device__ __forceinline__ double swb_weight_f64(const float* wrow, int idx, int D, double padw) {
  return idx < D ? (double)(wrow ? wrow[idx] : 1.f) : (idx == D ? padw : 0.0);
}

// grid (tiles, rows): piece blockIdx.x of the row
__global__ void __launch_bounds__(kMp64NT) k_splitw_bwd_mass(const CartSplitWBwd a) {
  __shared__ double redd[kMp64NT / kWave];
  const int64_t row = blockIdx.y;
  SwbRow l;
  if (!swb_row(a, row, l)) return;
  const int64_t t064 = (int64_t)blockIdx.x * kCartMaxLine;
  if (t064 >= l.total) return;
  const int t0 = (int)t064, n = max(0, min(l.D - t0, kCartMaxLine));
  double* dst = a.mass + row * a.tiles + blockIdx.x;
  if (!a.w) {                                                // kernel-uniform
    if (threadIdx.x == 0) *dst = (double)n;
    return;
  }
  const float* wr = a.w + l.start + t0;
  double pm = 0.0;
#pragma unroll
  for (int i = 0; i < kCartMaxLine / kMp64NT; ++i) {
    const int t = i * kMp64NT + (int)threadIdx.x;
    pm += t < n ? (double)wr[t] : 0.0;
  }
  pm = wave_sum(pm);
  if (lane_id() == 0) redd[wave_id()] = pm;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = 0.0;
#pragma unroll
    for (int q = 0; q < kMp64NT / kWave; ++q) m += redd[q];
    *dst = m;
  }
}

// grid (ceil(tiles / 4), nlines): wavefront w sorts run 4 blockIdx.x + w
__global__ void __launch_bounds__(kMp64NT, 2) k_splitw_bwd_runs(const CartSplitWBwd a) {
  constexpr int M = kCartLongM, CAP = kCartMaxLine;
  const int64_t line = blockIdx.y;
  const int lane = lane_id();
  SwbRow l;
  if (!swb_row(a, line / a.S, l)) return;
  const int s = (int)(line % a.S);
  const int64_t c64 = ((int64_t)blockIdx.x * 4 + wave_id()) * CAP;
  if (c64 >= l.total) return;                                // no barrier in this kernel: a wavefront may leave alone
  const int c0 = (int)c64, D = l.D;
  const int32_t* colrow = a.col + l.start;
  const float* xs = a.Xp + s;
  {
    constexpr bool RUN_PAD = true;
    unsigned long long* const run_line = swb_region(a, line, 0);
#include "sorted_run.inc"
  }
}

// grid (ceil(tiles / span), nlines): span blockIdx.x of level k, runs of kMp64Run << k words
__global__ void __launch_bounds__(kMp64NT, 2) k_splitw_bwd_level(const CartSplitWBwd a, int k, int span) {
  __shared__ mp64_t tk[kMp64TileLds];
  __shared__ int part[kMp64MaxSpan + 1];
  const int64_t line = blockIdx.y;
  SwbRow l;
  if (!swb_row(a, line / a.S, l)) return;
  const int64_t R64 = mp64_level_run(k);
  if (R64 >= (int64_t)l.total) return;                       // not a level of this line
  const Mp64Level lv = mp64_level(l.total, (int)R64);
  Mp64Span sp;
  if (!mp64_span(l.total, lv, span, (int)blockIdx.x, sp)) return;
  const mp64_t* src = swb_region(a, line, k);
  mp64_t* dst = swb_region(a, line, k + 1);
  if (sp.nt > 0) mp64_merge_tiles(src, dst, l.total, lv, sp.t0, sp.nt, tk, part);
  mp64_copy_run(src, dst, sp.c0, sp.c1, (int)threadIdx.x);
}

// grid (tiles, nlines): tile blockIdx.x of the sorted line, which lies where levels = mp64_num_levels(total) left it
__global__ void __launch_bounds__(kMp64NT) k_splitw_bwd_tsum(const CartSplitWBwd a) {
  constexpr int VT = kSwbVT, TILE = kMp64NT * VT;
  __shared__ double redd[kMp64NT / kWave];
  const int64_t line = blockIdx.y, row = line / a.S;
  SwbRow l;
  if (!swb_row(a, row, l)) return;
  const int64_t t064 = (int64_t)blockIdx.x * TILE;
  if (t064 > l.D) return;                                    // the tiles beyond element D hold fill elements only
  const int D = l.D;
  const float* wrow = a.w ? a.w + l.start : nullptr;
  const double padw = fmax((double)a.tau - swb_mass(a, row, l.total), 0.0);
  const mp64_t* se = swb_region(a, line, mp64_num_levels(l.total)) + t064 + (int)threadIdx.x * VT;   // total is a multiple of TILE
  double pre = 0.0;
#pragma unroll
  for (int j = 0; j < VT; ++j) pre += swb_weight_f64(wrow, (int)((unsigned int)se[j] & 0x7fffffffu), D, padw);
  pre = wave_sum(pre);
  if (lane_id() == 0) redd[wave_id()] = pre;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
#pragma unroll
    for (int q = 0; q < kMp64NT / kWave; ++q) tot += redd[q];
    a.tsum[line * a.tiles + blockIdx.x] = tot;
  }
}

// grid (tiles, nlines): tile blockIdx.x of the sorted line
__global__ void __launch_bounds__(kMp64NT, 2) k_splitw_bwd_walk(const CartSplitWBwd a) {
  constexpr int VT = kSwbVT, TILE = kMp64NT * VT, NW = 4;
  __shared__ float red[NW][kWave];
  __shared__ double redd[NW];
  const int64_t line = blockIdx.y, row = line / a.S;
  SwbRow l;
  if (!swb_row(a, row, l)) return;
  const int64_t t064 = (int64_t)blockIdx.x * TILE;
  if (t064 > l.D) return;                                    // the tiles beyond element D hold fill elements only
  const int t0 = (int)t064, D = l.D, L = D + 1, F = a.F, s = (int)(line % a.S);
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const float* wrow = a.w ? a.w + l.start : nullptr;
  const double taud = (double)a.tau, m = swb_mass(a, row, l.total);
  const double inv = 1.0 / fmax(m, taud);
  const float padw = (float)fmax(taud - m, 0.0);
  const double rho = pad_residual(taud - m, padw);           // what the float wt[] loses of the pad weight: added where the walk passes the pad
  const double* ts = a.tsum + line * a.tiles;
  double carry = 0.0;                                        // the cumulative weight before the tile
  for (int q = 0; q < (int)blockIdx.x; ++q) carry += ts[q];
  const mp64_t* se = swb_region(a, line, mp64_num_levels(l.total));
  const float* grow = a.g + (int64_t)l.node * a.ldg + a.gcol0 + (int64_t)s * F;
  float* gk = a.gkey + (int64_t)l.start * a.ldk + s;
  float* prow = a.partial + ((int64_t)line * a.tiles + blockIdx.x) * F;
  const int r0 = t0 + tid * VT;                              // total is a multiple of TILE: the tile lies in the line's region
  const bool live = t0 + w * kWave * VT < L;                 // this wavefront's ranks hold elements of the line (wave-uniform)
  float key[VT], wt[VT];
  int idx[VT];
  double pre = 0.0;
#pragma unroll
  for (int j = 0; j < VT; ++j) {
    const mp64_t e = se[r0 + j];
    key[j] = r0 + j < L ? from_orderable_bits((unsigned int)(e >> 32)) : 0.f;   // fill elements: no inf in the frequency sums
    idx[j] = (int)((unsigned int)e & 0x7fffffffu);
    wt[j] = swb_weight(wrow, idx[j], D, padw);
    pre += (double)wt[j] + (idx[j] == D ? rho : 0.0);
  }
  double cw0 = wave_exclusive_scan_f64(pre);
  const double wtot = __shfl(cw0 + pre, kWave - 1);          // this wavefront's total
  if (lane == 0) redd[w] = wtot;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < NW; ++q)
    if (q < w) cw0 += redd[q];
  cw0 += carry;
  for (int fb = 0; fb < F; fb += kWave) {
    const int nf = min(kWave, F - fb);
    float gfl = 0.f;                                         // lane q: this wavefront's gfreq sum of frequency fb + q
    float G[VT];
#pragma unroll
    for (int j = 0; j < VT; ++j) G[j] = 0.f;
    if (live) {
      for (int q = 0; q < nf; ++q) {
#include "walk_weighted.inc"
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
__global__ void __launch_bounds__(kSwbFinishNT) k_splitw_bwd_finish(const CartSplitWBwd a) {
  __shared__ float red[kSwbFinishNT / kWave];
  const int f = blockIdx.x, tid = threadIdx.x;
  const int64_t items = a.nlines * a.tiles;
  float sum = 0.f;
  for (int64_t i = tid; i < items; i += kSwbFinishNT) {
    const int64_t line = i / a.tiles;
    const int tile = (int)(i - line * a.tiles);
    SwbRow l;
    if (swb_row(a, line / a.S, l) && (int64_t)tile * kCartSplitWBwdWalk <= l.D) sum += a.partial[i * a.F + f];
  }
  sum = wave_sum(sum);
  if (lane_id() == 0) red[wave_id()] = sum;
  __syncthreads();
  if (tid == 0) {
    float tot = 0.f;
#pragma unroll
    for (int u = 0; u < kSwbFinishNT / kWave; ++u) tot += red[u];
    atomicAdd(a.gfreq + f, tot);
  }
}

}  // namespace

// general weights: the rows of the giant class of kCartLong[1], every line in its own regions of c->scratch
int launch_cart_split_w_bwd(const fsw_cart_args* c, const CartSplitWBwdPlan& p, hipStream_t stream) {
  const CartLongMode& m = kCartLong[1];
  if (p.lines <= 0) return 0;
  CartSplitWBwd t;
  cart_fill_inputs_w(t, c);
  cart_fill_grads(t, c);
  t.scratch = (mp64_t*)c->scratch; t.line_cap = p.words;
  t.mass = (double*)((char*)c->scratch + p.mass_offset);
  t.tsum = (double*)((char*)c->scratch + p.tsum_offset);
  t.partial = (float*)((char*)c->scratch + p.partial_offset);
  t.tiles = p.tiles; t.nlines = p.lines;
  t.bin = m.giant_bin; t.min_degree = m.giant_min_degree;
  // lines <= 2 GiB / (the 9 runs of the shortest row x 16 B) = 7281 and tiles <= 2 GiB / (2048 x 16 B) = 65536: every grid dimension fits
  const int64_t nruns = p.tiles;                               // runs = tile slots = walk tiles of the longest row
  k_splitw_bwd_mass<<<dim3((unsigned)nruns, (unsigned)p.rows), kMp64NT, 0, stream>>>(t);
  FSW_LAUNCH_CHECK();
  k_splitw_bwd_runs<<<dim3((unsigned)ceil_div(nruns, (int64_t)4), (unsigned)p.lines), kMp64NT, 0, stream>>>(t);
  FSW_LAUNCH_CHECK();
  // tile slots per workgroup of a level: about kSwbLevelWorkgroups workgroups per launch.  The result does not depend on it
  const int span = (int)std::min<int64_t>(std::max<int64_t>(ceil_div(p.lines * nruns, kSwbLevelWorkgroups), 1), kMp64MaxSpan);
  const dim3 spans((unsigned)ceil_div(nruns, (int64_t)span), (unsigned)p.lines);
  for (int k = 0; mp64_level_run(k) < t.line_cap; ++k) {
    k_splitw_bwd_level<<<spans, kMp64NT, 0, stream>>>(t, k, span);
    FSW_LAUNCH_CHECK();
  }
  const dim3 walk((unsigned)nruns, (unsigned)p.lines);
  k_splitw_bwd_tsum<<<walk, kMp64NT, 0, stream>>>(t);
  FSW_LAUNCH_CHECK();
  k_splitw_bwd_walk<<<walk, kMp64NT, 0, stream>>>(t);
  FSW_LAUNCH_CHECK();
  if (t.gfreq) {
    k_splitw_bwd_finish<<<(unsigned)c->F, kSwbFinishNT, 0, stream>>>(t);
    FSW_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace fsw

using namespace fsw;

// host values only (embed_cart.h: cart_split_w_bwd_plan)
extern "C" size_t fsw_embed_cart_split_w_backward_scratch_bytes(const fsw_cart_args* c) { return cart_split_w_bwd_plan(c).bytes; }
extern "C" int64_t fsw_embed_cart_split_w_backward_lines(const fsw_cart_args* c) { return cart_split_w_bwd_plan(c).lines; }
extern "C" int64_t fsw_embed_cart_split_w_backward_max_lines(void) { return kCartSplitWBwdMaxLines; }
