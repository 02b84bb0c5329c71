// Cartesian slice x frequency mode, the longest rows -- unit weights: above FSW_HUB_MAX_DEG neighbours; general weights (w != NULL or
// tau > 1): lines of more than FSW_CART_W_MAX_LINE elements; any length --: backward with respect to the keys and the frequencies.
// gfx950.  The forward: embed_giant_cart.hip, embed_giant_cart_w.hip; the classes below: embed_cart_hub_bwd.hip, embed_cart_hub_w_bwd.hip.
// One line split over many workgroups, a launch per phase: embed_split_cart_bwd.hip (unit weights), embed_split_cart_w_bwd.hip (general).
//
// k_cart_giant_bwd<WEIGHTED>: one workgroup of four wavefronts takes ONE (recipient row, slice) line at a time (the forward's
// persistent, XCD-aware line loop) in its own scratch line: two lines of packed (key, entry index) words (ping, pong), the line
// rounded up to whole runs of kCartMaxLine words.
//   A. every wavefront sorts the runs w, w + 4, .. into the ping line (sorted_run.inc).  General weights: the reference's pad element
//      has weight max(tau - m, 0); the row mass m is summed in float64 as the chunks load and reduced over the workgroup;
//   B. the levels above one run are merge-path passes between ping and pong (merge_path64.h: one unsigned 64-bit compare, no ties:
//      equal keys keep entry order, the pad element sorts last among the zeros -- the project's rule and the generic kernel's);
//   C. the workgroup walks the sorted line in tiles of 256 threads x kGbVT (16 | 8) consecutive ranks; every tile is read out at all F
//      frequencies (g_f and xi_f wave-uniform) with the arithmetic of the long-row kernels:
//        unit weights     walk_unit.inc;
//        general weights  the weights re-read by entry index (w[start + idx], the pad weight for idx == D, 0 for fill), the float64
//                         cumulative weight by wave scan + wavefront offsets + a carry from tile to tile (as k_cart_mergepath_w's
//                         readout), then walk_weighted.inc;
//        gkey[e, s]  = sum_f out_scale g[r, s F + f] (F_f(c_rank) - F_f(c_{rank-1}))          stored for every entry
//        gfreq[f]   += out_scale g[r, s F + f] sum_t (dF_f(c_t) - dF_f(c_{t-1})) p_(t)         one float atomic per (wavefront, line, frequency)
//      The key gradients accumulate in registers over the frequencies and pass through the line that the last level left free, in
//      entry order (sc[idx]), so that the stores to gkey walk the entries; pad and fill elements store nothing.  Lane f of every
//      wavefront carries its gfreq sum of frequency f; more than 64 frequencies take another walk per 64, the same thread adding into
//      the place it wrote before.
// The order of summation inside a line is fixed -- thread, tile --, so gkey does not depend on how many workgroups share the rows.
// Scratch: 16 bytes per word of the rounded line and workgroup (embed_cart.h: cart_giant_bwd_line_bytes).
#include <algorithm>
#include "embed_cart.h"
#include "embed_launch.h"
#include "fourier_coef.h"
#include "hub_line.h"
#include "merge_path64.h"
#include "sortnet.h"
#include "wave_sort.h"

namespace fsw {

namespace {

struct CartGiantBwd {
  const int32_t* rowptr;
  const int32_t* col;
  const float* w;                 // null: every weight is 1
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
  char* scratch;
  int64_t line_cap;         // words of each of a workgroup's two scratch lines: a multiple of kCartMaxLine, >= the longest line
  int bin, min_degree;      // the rows: perm[bin_start[bin] ..] with at least min_degree neighbours
};

// the walk: consecutive ranks per thread and tile, unit | general weights.  16 ranks with their weights next to the float64 chain of
// F_dF need 291 vector registers (one workgroup per CU); 8 need 228, and two workgroups share a CU
constexpr int kGbVT[2] = {16, 8};
static_assert(kMp64Run == kCartMaxLine && kMp64NT == 4 * kWave, "a run of merge_path64.h is one wavefront's chunk");
static_assert(kCartGiantBwdElemBytes == 2 * sizeof(mp64_t) && kCartMaxLine % kGbVT[0] == 0 && kCartMaxLine % kGbVT[1] == 0, "ping and pong; a thread's ranks end with the line");

template <bool WEIGHTED>
__global__ void __launch_bounds__(kMp64NT, 2) k_cart_giant_bwd(const CartGiantBwd a) {
  constexpr int NW = 4, M = kCartLongM, CAP = kCartMaxLine, VT = kGbVT[WEIGHTED ? 1 : 0], TILE = kMp64NT * VT;
  __shared__ mp64_t tk[kMp64TileLds];       // a staged tile of the merge levels
  __shared__ int part[kMp64Parts + 1];      // their tile boundaries
  __shared__ double redm[NW], redd[NW];     // wavefront sums: the row mass | the weights of a tile of the walk
  const int pbeg = a.bin_start[a.bin], nrows = a.bin_start[FSW_NUM_BINS] - pbeg;
  const int tid = threadIdx.x, lane = lane_id(), w = wave_id();
  const int S = a.S, F = a.F;
  const int blk = xcd_first_line();
  mp64_t* ping = reinterpret_cast<mp64_t*>(a.scratch + (int64_t)blk * a.line_cap * kCartGiantBwdElemBytes);
  mp64_t* pong = ping + a.line_cap;
  const int64_t nlines = (int64_t)nrows * S;
  const double taud = (double)a.tau;
  for (int64_t line = blk; line < nlines; line += gridDim.x) {
    // workgroup-uniform values, kept in scalar registers: the sort network leaves no vector register for them
    const int node = __builtin_amdgcn_readfirstlane(a.perm[pbeg + (int)(line / S)]), s = (int)(line % S);
    const int start = __builtin_amdgcn_readfirstlane(a.rowptr[node]);
    const int D = __builtin_amdgcn_readfirstlane(a.rowptr[node + 1]) - start;
    const int L = D + (WEIGHTED ? 1 : 0);                    // with the pad element
    const int64_t total64 = ((int64_t)L + CAP - 1) / CAP * CAP;
    // a row of another class in this bin, or one longer than the host's max_degree, which sized the lines (workgroup-uniform)
    if (D < a.min_degree || total64 > a.line_cap) continue;
    const int total = (int)total64;
    const int32_t* colrow = a.col + start;
    const float* wrow = (WEIGHTED && a.w) ? a.w + start : nullptr;
    const float* xs = a.Xp + s;
    // A. runs: gather (striped: lane-contiguous col and weight reads; the entry index travels with the key), sort, park
    double mpart = 0.0;
    for (int c0 = w * CAP; c0 < total; c0 += NW * CAP) {
      if constexpr (WEIGHTED) {                              // the chunk's weights first: their registers are free again for the gather
        if (wrow) {
#pragma unroll
          for (int j = 0; j < M; ++j) {
            const int t = c0 + j * kWave + lane;
            mpart += (double)(t < D ? wrow[t] : 0.f);
          }
        } else {
          mpart += (double)max(0, min(D - c0 - lane + kWave - 1, M * kWave) / kWave);   // entries t = c0 + j * 64 + lane < D, j < M
        }
      }
      {
        constexpr bool RUN_PAD = WEIGHTED;
        unsigned long long* const run_line = ping;
#include "sorted_run.inc"
      }
    }
    double inv = 1.0 / (double)D;
    float padw = 0.f;
    double rho = 0.0;                                        // what the float wt[] loses of the pad weight: added where the walk passes the pad (fsw_common.h)
    if constexpr (WEIGHTED) {
      mpart = wave_sum(mpart);
      if (lane == 0) redm[w] = mpart;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();
    if constexpr (WEIGHTED) {
      double m = 0.0;
#pragma unroll
      for (int q = 0; q < NW; ++q) m += redm[q];             // rewritten after the barriers of the next line's phase C at the earliest
      inv = 1.0 / fmax(m, taud);
      padw = (float)fmax(taud - m, 0.0);
      rho = pad_residual(taud - m, padw);
    }
    // B. merge-path levels between ping and pong
    const mp64_t* se = merge_path64_levels(ping, pong, total, tk, part);
    float* sc = reinterpret_cast<float*>(se == ping ? pong : ping);   // key gradients in entry order: the line the last level left free
    // C. walk: the thread's ranks r0 .. r0 + VT - 1 of every tile at all frequencies
    const float* grow = a.g + (int64_t)node * a.ldg + a.gcol0 + (int64_t)s * F;
    for (int fb = 0; fb < F; fb += kWave) {
      const int nf = min(kWave, F - fb);
      float gfl = 0.f;                                       // lane q: this wavefront's gfreq sum of frequency fb + q
      double carry = 0.0;                                    // general weights: the cumulative weight before the tile
      for (int t0 = 0; t0 < L; t0 += TILE) {
        const int r0 = t0 + tid * VT;
        const bool live = t0 + w * kWave * VT < L;           // this wavefront's ranks hold elements of the line (wave-uniform)
        float key[VT], G[VT], wt[WEIGHTED ? VT : 1];
        int idx[VT];
#pragma unroll
        for (int j = 0; j < VT; ++j) {
          const mp64_t e = r0 < total ? se[r0 + j] : ~0ull;   // total is a multiple of VT: a thread's ranks lie in the line or past it
          key[j] = r0 + j < L ? from_orderable_bits((unsigned int)(e >> 32)) : 0.f;   // fill elements: no inf in the frequency sums
          idx[j] = (int)((unsigned int)e & 0x7fffffffu);
          G[j] = 0.f;
        }
        if constexpr (WEIGHTED) {
          double pre = 0.0;
#pragma unroll
          for (int j = 0; j < VT; ++j) {
            wt[j] = idx[j] < D ? (wrow ? wrow[idx[j]] : 1.f) : (idx[j] == D ? padw : 0.f);
            pre += (double)wt[j] + (idx[j] == D ? rho : 0.0);
          }
          double cw0 = wave_exclusive_scan_f64(pre);
          const double wtot = __shfl(cw0 + pre, kWave - 1);  // this wavefront's total
          if (lane == 0) redd[w] = wtot;
          __syncthreads();
          double tot = 0.0;
#pragma unroll
          for (int q = 0; q < NW; ++q) {
            if (q < w) cw0 += redd[q];
            tot += redd[q];
          }
          __syncthreads();                                   // redd is rewritten by the next tile
          cw0 += carry;
          carry += tot;
          if (live) {
            for (int q = 0; q < nf; ++q) {
#include "walk_weighted.inc"
            }
          }
        } else {
          if (live) {
            for (int q = 0; q < nf; ++q) {
#include "walk_unit.inc"
            }
          }
        }
#pragma unroll
        for (int j = 0; j < VT; ++j) {
          if (idx[j] < D) sc[idx[j]] = fb == 0 ? G[j] : sc[idx[j]] + G[j];   // the same thread wrote sc[idx] in the walk before
        }
      }
      if (a.gfreq && lane < nf) atomicAdd(a.gfreq + fb + lane, gfl);
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();
    for (int t = tid; t < D; t += kMp64NT) a.gkey[(int64_t)(start + t) * a.ldk + s] = sc[t];
    // the next line's runs overwrite the scratch lines that other threads still read
    __syncthreads();
  }
}

}  // namespace

// the rows of the giant class of the call's mode, as many workgroups as c->scratch holds lines (a multiple of 8 from 8 on)
int launch_cart_giant_bwd(const fsw_cart_args* c, hipStream_t stream) {
  const bool unit_fast = cart_unit_fast(c);
  const CartLongMode& m = cart_long_mode(unit_fast);
  const int64_t rows = cart_giant_rows(c, m);
  if (rows <= 0) return 0;
  FSW_REQUIRE(c->scratch && ((uintptr_t)c->scratch & 15) == 0,
              "fsw_embed_cart_backward_keys_f32: rows of the longest class need a 16-byte aligned scratch buffer "
              "(fsw_embed_cart_backward_keys_scratch_bytes)");
  const size_t line_bytes = cart_giant_bwd_line_bytes(m, c->max_degree);
  const int64_t nwg = cart_giant_bwd_workgroups(m, (int64_t)(c->scratch_bytes / line_bytes), rows * c->S);
  FSW_REQUIRE(nwg >= 1, "fsw_embed_cart_backward_keys_f32: scratch buffer too small for one line of the longest class "
                        "(need fsw_embed_cart_backward_keys_scratch_bytes)");
  CartGiantBwd t;
  cart_fill_inputs_w(t, c);
  cart_fill_grads(t, c);
  t.scratch = reinterpret_cast<char*>(c->scratch); t.line_cap = (int64_t)(line_bytes / kCartGiantBwdElemBytes);
  t.bin = m.giant_bin; t.min_degree = m.giant_min_degree;
  if (unit_fast) k_cart_giant_bwd<false><<<(unsigned)nwg, kMp64NT, 0, stream>>>(t);
  else k_cart_giant_bwd<true><<<(unsigned)nwg, kMp64NT, 0, stream>>>(t);
  FSW_LAUNCH_CHECK();
  return 0;
}

}  // namespace fsw
