// Cartesian slice x frequency mode, unit weights, rows above FSW_HUB_MAX_DEG: the forward of k_cart_giant (embed_giant_cart.hip) with ONE
// (row, slice) line split over many workgroups.  gfx950.
//
// k_cart_giant gives a line to one workgroup, which walks the line's blocks of kCartGiantBlk keys one after the other through eleven
// (150 000 keys) to twenty-two (1 000 000 keys) fence-separated passes: one point cloud at S = 16 keeps 16 CUs busy.  Here every pass is
// a launch of its own whose grid covers (line, block), from the same building blocks (hub_line.h, wave_sort.h):
//   k_split_sort    (line, block): phase A of k_cart_giant for one block, parked at rank order b * BLK + w * CAP + lane * M + j
//   k_split_sweep   one launch per exchange of a merge level size = 2, 4, .., pow2ceil(nb): the flip, then the strides size / 4 .. 1
//                   (hub_line.h: sweep_block_pair), every pair cut into kSplitCut workgroups.  Pairs whose upper block holds only
//                   +inf are skipped
//   k_split_tail    (line, block): fetch, workgroup_merge_block; below the line's last level: park.  At the line's LAST level the block
//                   stays in registers and is read out at all F frequencies in batches of kFB (unit_readout) -- lane, wavefront,
//                   workgroup -- into partial[line][b][f]
//   k_split_finish  (line, f): the partial sums of blocks 0 .. nb - 1 in block order, bias, out_scale; the mass column for s == 0
// Consecutive launches in the caller's stream are the only synchronisation between workgroups: no spin barrier, no cooperative launch,
// no flag in memory, no float atomic, so nothing waits on a partly resident grid and the order of summation is fixed.  The grids are sized
// by the longest row (nbmax blocks); a workgroup whose block, pair or level does not exist for ITS line leaves at once (workgroup-uniform,
// before any barrier), so a line runs exactly the levels of its own length and its output depends on the line only: not on the other
// rows, S, the grid or what the scratch held.  Every line owns its region of the scratch; blocks b >= nb of a region are never read.
// The scratch and its query: embed_cart.h (CartSplitPlan), include/fsw_hip.h (fsw_embed_cart_split_scratch_bytes).
#include <algorithm>
#include "embed_cart.h"
#include "embed_launch.h"
#include "hub_line.h"
#include "sortnet.h"
#include "wave_sort.h"

namespace fsw {

namespace {

constexpr int kSplitCut = 16;                  // workgroups per pair of blocks of a sweep: 5 blocks x 16 lines leave >= 256 in every launch
constexpr int kSplitSweepNT = 256;             // threads of a sweep workgroup: kCartGiantBlk / kSplitCut / 4 / 256 = 2 accesses of 16 bytes each
constexpr int kSplitFinishNT = 256;
static_assert(kCartGiantBlk % (kSplitCut * kSplitSweepNT * 4) == 0, "a sweep workgroup's part of a block in whole 16-byte accesses");

struct CartSplit {
  const int32_t* rowptr;
  const int32_t* col;
  const int32_t* perm;
  const int32_t* bin_start;
  const float* Xp;
  int64_t ldp;
  const float* freqs;
  int S, F;
  float* out;
  int64_t ldo;
  const float* bias;
  float out_scale;
  int has_mass, mass_fn;
  float mass_scale;
  float* scratch;           // [nlines][line_floats]: line = (row within the class's bins) * S + s
  int64_t line_floats;      // a multiple of kCartGiantBlk, >= the longest row
  float* partial;           // [nlines][nbmax][F]
  int nbmax;                // line_floats / kCartGiantBlk
  int64_t nlines;
  int bin, min_degree;      // the rows: perm[bin_start[bin] ..] with at least min_degree neighbours
};

struct SplitLine { int node, s, start, D, nb; };
// the line's row (embed_cart.h: cart_row_at) with its slice and its blocks; false for a row that k_cart_giant skips too
__device__ __forceinline__ bool split_line(const CartSplit& a, int64_t line, SplitLine& l) {
  const int pbeg = a.bin_start[a.bin];
  cart_row_at(a, pbeg + (int)(line / a.S), l);
  l.s = (int)(line % a.S);
  l.nb = (l.D + kCartGiantBlk - 1) / kCartGiantBlk;
  return l.D >= a.min_degree && (int64_t)l.nb * kCartGiantBlk <= a.line_floats;
}

// grid (nbmax, nlines)
__global__ void __launch_bounds__(kCartGiantNW* kWave, 4) k_split_sort(const CartSplit a) {
  constexpr int NW = kCartGiantNW, M = kCartLongM, CAP = M * kWave, BLK = kCartGiantBlk;
  static_assert(NW * CAP == BLK, "one block across the workgroup's registers");
  __shared__ float xbuf[NW * CAP];
  const int b = blockIdx.x;
  const int64_t line = blockIdx.y;
  SplitLine l;
  if (!split_line(a, line, l) || b >= l.nb) return;
  const int lane = lane_id(), w = wave_id();
  WaveLine<M, false> ln;
  gather_chunk<M>(ln, a.col + l.start, b * BLK + w * CAP, l.D, a.Xp, a.ldp, l.s, lane);
  ln.sort();
  workgroup_merge_levels<NW, M>(ln, xbuf, w, lane);
  park_keys<M>(ln, a.scratch + line * a.line_floats + (int64_t)b * BLK + w * CAP + lane * M);
}

// grid (pow2ceil(nbmax) / 2 * kSplitCut, nlines): pair p of the exchange (flip: st == 0) of level `size`, part blockIdx.x % kSplitCut
__global__ void __launch_bounds__(kSplitSweepNT) k_split_sweep(const CartSplit a, int size, int st) {
  constexpr int BLK = kCartGiantBlk, PART = BLK / kSplitCut;
  const int p = blockIdx.x / kSplitCut, part = blockIdx.x % kSplitCut;
  const int64_t line = blockIdx.y;
  const bool flip = st == 0;
  const int half = flip ? size >> 1 : st;                    // the pairs' lower blocks: `half` consecutive ones out of every 2 * half
  const int b = (p / half) * (half << 1) + (p % half);
  const int b2 = flip ? (b ^ (size - 1)) : (b + st);
  SplitLine l;
  if (!split_line(a, line, l) || b2 >= l.nb || size > (int)pow2ceil((uint32_t)l.nb)) return;   // all-+inf partner: no-op; not a level of this line
  float* lo = a.scratch + line * a.line_floats + (int64_t)b * BLK;
  float* hi = a.scratch + line * a.line_floats + (int64_t)b2 * BLK;
#pragma unroll
  for (int i = 0; i < PART / (kSplitSweepNT * 4); ++i) {
    sweep_block_pair<BLK>(lo, hi, part * PART + (i * kSplitSweepNT + (int)threadIdx.x) * 4, flip);
  }
}

// grid (nbmax, nlines): the in-block tail of level `size`; at the line's last level the readout of the block instead of parking it
__global__ void __launch_bounds__(kCartGiantNW* kWave, 4) k_split_tail(const CartSplit a, int size) {
  constexpr int NW = kCartGiantNW, M = kCartLongM, CAP = M * kWave, BLK = kCartGiantBlk;
  static_assert(NW <= kFB, "wavefront 0 sums a batch's wave sums");
  __shared__ float xbuf[NW * CAP];
  __shared__ float red[2][kFB][NW];       // wave sums of a batch of frequencies, double-buffered
  const int b = blockIdx.x;
  const int64_t line = blockIdx.y;
  SplitLine l;
  if (!split_line(a, line, l) || b >= l.nb) return;
  const int nbp = (int)pow2ceil((uint32_t)l.nb);
  if (size > nbp) return;                                    // not a level of this line
  const int lane = lane_id(), w = wave_id();
  float* mine = a.scratch + line * a.line_floats + (int64_t)b * BLK + w * CAP + lane * M;
  WaveLine<M, false> ln;
  fetch_keys<M>(ln, mine);
  workgroup_merge_block<NW, M>(ln, xbuf, w, lane);
  if (size < nbp) {
    park_keys<M>(ln, mine);
    return;
  }
  // the line is sorted: the lane's keys have ranks r0 .. r0 + M - 1
  const int F = a.F;
  const int r0 = b * BLK + w * CAP + lane * M;
  const bool live = b * BLK + w * CAP < l.D;                 // else the wavefront's keys are all +inf: it contributes 0
  float* prow = a.partial + (line * a.nbmax + b) * (int64_t)F;
  int buf = 0;
  for (int f0 = 0; f0 < F; f0 += kFB, buf ^= 1) {
    const int nf = min(kFB, F - f0);
    float acc[kFB];
#pragma unroll
    for (int q = 0; q < kFB; ++q) acc[q] = 0.f;
    if (live) {
#pragma unroll
      for (int q = 0; q < kFB; ++q)
        if (q < nf) acc[q] = unit_readout<M>(ln, r0, l.D, a.freqs[f0 + q]);
    }
#pragma unroll
    for (int q = 0; q < kFB; ++q) {
      if (q < nf) {
        const float tot = wave_sum(acc[q]);
        if (lane == 0) red[buf][q][w] = tot;
      }
    }
    __syncthreads();
    // the batch before the previous one used this buffer: every wavefront has passed a barrier since wavefront 0 read it
    if (w == 0 && lane < nf) {
      float val = 0.f;
#pragma unroll
      for (int u = 0; u < NW; ++u) val += red[buf][lane][u];
      prow[f0 + lane] = val;
    }
  }
}

// one thread per (line, f)
__global__ void __launch_bounds__(kSplitFinishNT) k_split_finish(const CartSplit a) {
  const int64_t i = (int64_t)blockIdx.x * kSplitFinishNT + threadIdx.x;
  if (i >= a.nlines * a.F) return;
  const int64_t line = i / a.F;
  const int f = (int)(i - line * a.F);
  SplitLine l;
  if (!split_line(a, line, l)) return;
  const float* p = a.partial + line * a.nbmax * (int64_t)a.F + f;
  float sum = 0.f;
  for (int b = 0; b < l.nb; ++b) sum += p[(int64_t)b * a.F];
  float* orow = a.out + (int64_t)l.node * a.ldo;
  const int64_t c = (int64_t)a.has_mass + (int64_t)l.s * a.F + f;
  orow[c] = a.out_scale * (sum + (a.bias ? a.bias[c] : 0.f));
  if (a.has_mass && l.s == 0 && f == 0) orow[0] = mass_column((float)l.D, a.mass_fn, a.mass_scale, a.bias, a.out_scale);
}

}  // namespace

// unit weights with tau <= 1: the rows of the giant class of kCartLong[0], every line in its own region of c->scratch
int launch_cart_split(const fsw_cart_args* c, const CartSplitPlan& p, hipStream_t stream) {
  const CartLongMode& m = kCartLong[0];
  if (p.lines <= 0) return 0;
  CartSplit t;
  cart_fill_inputs(t, c);
  cart_fill_outputs(t, c);
  t.scratch = (float*)c->scratch; t.line_floats = (int64_t)(p.line_bytes / sizeof(float));
  t.partial = (float*)((char*)c->scratch + p.partial_offset); t.nbmax = p.nbmax; t.nlines = p.lines;
  t.bin = m.giant_bin; t.min_degree = m.giant_min_degree;
  // lines <= 2 GiB / (two blocks) = 8192 and lines * nbmax <= 2 GiB / (one block) = 16384: every grid dimension fits
  const dim3 blocks((unsigned)p.nbmax, (unsigned)p.lines);
  const int nbp = (int)pow2ceil((uint32_t)p.nbmax);
  const dim3 pairs((unsigned)(nbp / 2 * kSplitCut), (unsigned)p.lines);
  k_split_sort<<<blocks, kCartGiantNW * kWave, 0, stream>>>(t);
  FSW_LAUNCH_CHECK();
  for (int size = 2; size <= nbp; size <<= 1) {
    k_split_sweep<<<pairs, kSplitSweepNT, 0, stream>>>(t, size, 0);
    FSW_LAUNCH_CHECK();
    for (int st = size >> 2; st >= 1; st >>= 1) {
      k_split_sweep<<<pairs, kSplitSweepNT, 0, stream>>>(t, size, st);
      FSW_LAUNCH_CHECK();
    }
    k_split_tail<<<blocks, kCartGiantNW * kWave, 0, stream>>>(t, size);
    FSW_LAUNCH_CHECK();
  }
  k_split_finish<<<(unsigned)ceil_div(p.lines * c->F, kSplitFinishNT), kSplitFinishNT, 0, stream>>>(t);
  FSW_LAUNCH_CHECK();
  return 0;
}

}  // namespace fsw
