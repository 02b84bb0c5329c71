// Cartesian slice x frequency mode, unit weights, rows above FSW_HUB_MAX_DEG (any length): forward.  gfx950.
//
// The composition of the diagonal k_embed_giant (embed_hub.hip) with the readout of k_cart_hub (embed_cart_hub.hip), from the same
// building blocks (hub_line.h, wave_sort.h).  One workgroup of kCartGiantNW = 16 wavefronts takes ONE (recipient row, slice) line at a
// time (persistent, XCD-aware line loop).  The line is cut into blocks of kCartGiantBlk keys -- 16 wavefronts x 2048, the line of the
// largest hub class --, every block is gathered and sorted in the workgroup's registers and parked in the workgroup's scratch line
// (global memory, 4 bytes per key).  The bitonic merge levels above one block are element-wise min / max sweeps over pairs of blocks
// (coalesced, all 1024 threads) followed by the in-workgroup tail of the level (workgroup_merge_block) on every block; pairs whose
// upper block holds only +inf are skipped.  Synchronisation between the phases: a workgroup-scope fence and a barrier, as in
// k_embed_giant (an agent-scope fence measured 3x the kernel time there).
// The sort is paid once per slice.  The last level parks its blocks too, and the sorted line is then read out at all F frequencies in
// batches of kFB: every lane walks ITS keys of every block (the places it stored itself) and keeps kFB sums over all blocks
// (unit_readout: one float64 FMA per key and frequency), then the wave sums go into the double-buffered LDS table of k_cart_hub, ONE
// barrier, and lanes 0 .. kFB - 1 of wavefront 0 store a contiguous run of outputs.  The order of summation of a line is fixed -- lane,
// wavefront, block --, so the output does not depend on how many workgroups share the rows.
// General weights: embed_giant_cart_w.hip.  The classes and the scratch line: embed_cart.h.
#include <algorithm>
#include "embed_cart.h"
#include "embed_launch.h"
#include "hub_line.h"
#include "sortnet.h"
#include "wave_sort.h"

namespace fsw {

namespace {

struct CartGiant {
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
  float* scratch;
  int64_t line_floats;      // floats of a workgroup's scratch line: a multiple of kCartGiantBlk, >= the longest row
  int bin, min_degree;      // the rows: perm[bin_start[bin] ..] with at least min_degree neighbours
};

__global__ void __launch_bounds__(kCartGiantNW* kWave, 4) k_cart_giant(const CartGiant a) {
  constexpr int NW = kCartGiantNW, M = kCartLongM, CAP = M * kWave, BLK = kCartGiantBlk, NT = NW * kWave;
  static_assert(NW <= kFB && NW * CAP == BLK, "one block across the workgroup's registers");
  __shared__ float xbuf[NW * CAP];        // exchange buffer of the merge levels inside a block
  __shared__ float red[2][kFB][NW];       // wave sums of a batch of frequencies, double-buffered
  const int pbeg = a.bin_start[a.bin], nrows = a.bin_start[FSW_NUM_BINS] - pbeg;
  const int lane = lane_id(), w = wave_id();
  const int S = a.S, F = a.F;
  const int blk = xcd_first_line();
  float* sl = a.scratch + (int64_t)blk * a.line_floats;
  const int64_t nlines = (int64_t)nrows * S;
  // every wavefront's scratch stores performed, then a barrier.  Workgroup scope is enough: the wavefronts of a workgroup share their
  // CU's L1, which the CU's own stores write through
  auto sync_scratch = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();
  };
  for (int64_t line = blk; line < nlines; line += gridDim.x) {
    const int node = a.perm[pbeg + (int)(line / S)], s = (int)(line % S);
    const int start = a.rowptr[node];
    const int D = a.rowptr[node + 1] - start;
    const int nb = (D + BLK - 1) / BLK;                   // blocks that hold keys
    // a row of another class in this bin, or one longer than the host's max_degree, which sized the line (workgroup-uniform)
    if (D < a.min_degree || (int64_t)nb * BLK > a.line_floats) continue;
    const int nbp = (int)pow2ceil((uint32_t)nb);
    float* mine = sl + w * CAP + lane * M;                // the lane's M keys of block 0; block b: + b * BLK
    WaveLine<M, false> ln;
    // A. blocks: gather, sort in the workgroup's registers, park in the scratch line
#pragma unroll 1
    for (int b = 0; b < nb; ++b) {
      gather_chunk<M>(ln, a.col + start, b * BLK + w * CAP, D, a.Xp, a.ldp, s, lane);
      ln.sort();
      workgroup_merge_levels<NW, M>(ln, xbuf, w, lane);
      park_keys<M>(ln, mine + (int64_t)b * BLK);
    }
    sync_scratch();
    // B. merge levels above one block
#pragma unroll 1
    for (int size = 2; size <= nbp; size <<= 1) {
      // element-wise exchanges between blocks: the flip (b against b ^ (size - 1), mirrored), then strides size / 4 .. 1
      auto sweep = [&](bool flip, int st) {
#pragma unroll 1
        for (int b = 0; b < nb; ++b) {
          const int b2 = flip ? (b ^ (size - 1)) : (b ^ st);
          if (b2 <= b || b2 >= nb) continue;              // each pair once, from its lower block; all-+inf partners: no-op
          float* lo = sl + (int64_t)b * BLK;
          float* hi = sl + (int64_t)b2 * BLK;
#pragma unroll 2
          for (int e = threadIdx.x * 4; e < BLK; e += NT * 4) sweep_block_pair<BLK>(lo, hi, e, flip);
        }
        sync_scratch();
      };
      sweep(true, 0);
      for (int st = size >> 2; st >= 1; st >>= 1) sweep(false, st);
#pragma unroll 1
      for (int b = 0; b < nb; ++b) {
        fetch_keys<M>(ln, mine + (int64_t)b * BLK);
        workgroup_merge_block<NW, M>(ln, xbuf, w, lane);
        park_keys<M>(ln, mine + (int64_t)b * BLK);
      }
      sync_scratch();
    }
    // C. readout: a lane reads back the places it parked itself, rank b * BLK + w * CAP + lane * M + j
    float* orow = a.out + (int64_t)node * a.ldo;
    const int64_t c0 = (int64_t)a.has_mass + (int64_t)s * F;
    int buf = 0;
    for (int f0 = 0; f0 < F; f0 += kFB, buf ^= 1) {
      const int nf = min(kFB, F - f0);
      float acc[kFB];
#pragma unroll
      for (int q = 0; q < kFB; ++q) acc[q] = 0.f;
#pragma unroll 1
      for (int b = 0; b < nb; ++b) {
        const int r0 = b * BLK + w * CAP + lane * M;
        if (b * BLK + w * CAP >= D) break;                  // the wavefront's keys of this and the later blocks: all +inf
        fetch_keys<M>(ln, mine + (int64_t)b * BLK);
#pragma unroll
        for (int q = 0; q < kFB; ++q)
          if (q < nf) acc[q] += unit_readout<M>(ln, r0, D, a.freqs[f0 + q]);
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
        const int64_t c = c0 + f0 + lane;
        orow[c] = a.out_scale * (val + (a.bias ? a.bias[c] : 0.f));
      }
    }
    if (a.has_mass && s == 0 && w == 0 && lane == 0) orow[0] = mass_column((float)D, a.mass_fn, a.mass_scale, a.bias, a.out_scale);
    // the next line's exchanges and scratch barriers separate its first batch from this line's last two; its blocks are parked by the
    // lanes that read these places here
  }
}

}  // namespace

// unit weights with tau <= 1: the rows of the giant class of kCartLong[0], as many workgroups as c->scratch holds lines
int launch_cart_giant(const fsw_cart_args* c, hipStream_t stream) {
  const CartLongMode& m = kCartLong[0];
  int64_t nwg;
  size_t line_bytes;
  if (const int rc = cart_giant_plan(c, m, &nwg, &line_bytes)) return rc;
  if (nwg == 0) return 0;
  CartGiant t;
  cart_fill_inputs(t, c);
  cart_fill_outputs(t, c);
  t.scratch = (float*)c->scratch; t.line_floats = (int64_t)(line_bytes / sizeof(float));
  t.bin = m.giant_bin; t.min_degree = m.giant_min_degree;
  k_cart_giant<<<(unsigned)nwg, kCartGiantNW * kWave, 0, stream>>>(t);
  FSW_LAUNCH_CHECK();
  return 0;
}

}  // namespace fsw
