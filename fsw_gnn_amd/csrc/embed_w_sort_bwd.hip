// Backward of the fused neighbourhood kernel WITH the gradient of the weights, rows of kWRegMaxDeg + 1 .. kWSortMaxDeg neighbours,
// wave-sort form.  gfx950.
//
// The structure is that of k_embed_wsort_bwd<M, true> (embed_wsort_bwd.hip): the neighbourhood transposed through LDS, four
// (row, slice) lines per workgroup, one per wavefront, held across the lanes' registers as packed (key, element index) words and
// sorted without a workgroup barrier, ties by element index; the pad element (key 0, weight max(tau - m, 0) in float64) is element
// D of the line.  Lane l owns the ranks l M .. l M + M - 1.  gkey and gfreq come from F and dF/dxi on the cumulative weight (in-lane
// prefix + float64 wave scan) with the expressions of that kernel.  On top of that walk, the gradient of the weights in the sorted
// order (embed_generic.hip, embed_w_bwd.hip): with h(c) = 2 (1 + xi) cos(2 pi xi c), c1_t = cum_t / M, c0_t = c1_{t-1},
//     q_t     = (h(c1_t) - h(c0_t)) key_t
//     R(t)    = h(c1_t) key_t + sum_{v > t} q_v                  (in-lane suffix + reverse float64 wave scan of the lanes' sums)
//     HC      = sum_t (h(c1_t) c1_t - h(c0_t) c0_t) key_t        (wave sum)
//     gw_j(s) = out_scale g[row, s] (R(rank_j) - [m <= tau] R(rank_pad) - [m >= tau] HC) / M
// R(rank_pad) is broadcast from the lane that holds element D.  The lane keeps h(c1_t) of its M ranks from the forward walk (the
// only per-element float64 array; R overwrites it on the way back), so the cosine of a rank is evaluated once.
// The class ends at 1024 neighbours: the instance of 64 ranks per lane (1025 .. 2048) spills 1.4 - 1.9 KB per lane in this form, 1.4 KB
// with a second walk that evaluates h again in place of the array, and 0.9 KB with the lane's constant part of R added in a second
// round of LDS atomics (k_embed_wsort_bwd<64, true> alone stands at 504 of 512 registers); those rows stay on the generic kernel.
// The weights are staged in LDS as (double)w + (double)w_lo (w_lo nullable: include/fsw_hip.h, fsw_embed_backward_w_lo_f32); the
// row mass, 1 / max(m, tau) and every cumulative weight come from these float64 values.
// Sum over slices: a [LINE] float64 accumulator in LDS takes every line's contributions with LDS float64 atomics, over all the
// slice groups the workgroup visits for the row; the workgroup then issues ONE float32 atomic per entry to consecutive addresses
// of gw (none for an exactly zero sum).  An entry receives min(gridDim.y, ceil(S / SC)) float32 adds.
// A line whose output gradient is zero writes zeros to its gkey column and adds nothing to gfreq or gw.
// Shared with k_embed_wsort and k_embed_wsort_bwd: the line length, the slices per group, the workgroups per row and the row mass
// (wsort_tile.h), the gather of a slice group (wsort_gather.inc) and the float64 wave scans (fsw_common.h).  The packed line load, the
// lane's weight sum and the forward walk are copies of those of k_embed_wsort_bwd and walk_line<M, true>: DESIGN.md, "Steps that the
// diagonal-mode kernels share", open work.
#include <algorithm>
#include "embed_launch.h"
#include "sortnet.h"
#include "wave_sort.h"
#include "weighted_coef.h"
#include "wsort_tile.h"

#define FSW_WS_GATHER_EDGE 0   // wsort_gather.inc: no edge features here

namespace fsw {

// as k_embed_wsort_bwd: two workgroups per CU
template <int M>
constexpr int ws_lds_bytes() { return 69 * 1024; }
// slices per group (wsort_tile.h): the float tile next to the two float64 lines (weights, accumulator)
template <int M>
constexpr int wsw_slices() { return ws_slices<M>(ws_lds_bytes<M>(), 2 * 8 * ws_line<M>()); }

template <int M>
__global__ void __launch_bounds__(256, (M <= 8 ? 2 : 1)) k_embed_wsort_w_bwd(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ w, const float* __restrict__ w_lo,
    const int32_t* __restrict__ perm, const int32_t* __restrict__ bin_start, int bin_lo, int bin_hi, const float* __restrict__ Xp,
    int64_t ldp, int S, const float* __restrict__ freqs, float tau, const float* __restrict__ g, int64_t ldg, int gcol0,
    float out_scale, float* __restrict__ gfreq, float* __restrict__ gkey, int64_t ldk, float* __restrict__ gw) {
  constexpr int CAP = M * kWave;
  constexpr int LINE = ws_line<M>();
  constexpr int SC = wsw_slices<M>();
  static_assert(SC >= 1, "a line must fit the LDS budget");
  static_assert((2 * 8 + 4 * SC) * LINE + 64 <= 160 * 1024, "LDS of one workgroup");
  extern __shared__ __attribute__((aligned(16))) double smem_d[];
  double* wrow = smem_d;                                  // [LINE] w + w_lo of the row, padded like a line
  double* gacc = smem_d + LINE;                           // [LINE] sum over the slices of the row's weight gradients
  float* tile = reinterpret_cast<float*>(smem_d + 2 * LINE);   // [SC][LINE]
  __shared__ double msum[4];
  const int pbeg = bin_start[bin_lo], pend = bin_start[bin_hi + 1];
  const int lane = lane_id(), wv = wave_id();
  const int ngroups = (S + SC - 1) / SC;
  if ((int)blockIdx.y >= ngroups) return;                 // the whole workgroup
  const double taud = (double)tau;

  for (int p = pbeg + blockIdx.x; p < pend; p += gridDim.x) {
    const int node = perm[p];
    const int start = rowptr[node];
    const int D = rowptr[node + 1] - start;
    const int Dtot = D + 1;
    if (Dtot > CAP) continue;                             // not a row of this instance's bins (the launcher never sends one)
    double part = 0.0;
    for (int t = threadIdx.x; t < D; t += blockDim.x) {
      const double wt = (double)w[start + t] + (w_lo ? (double)w_lo[start + t] : 0.0);
      wrow[t + t / M] = wt;
      gacc[t + t / M] = 0.0;
      part += wt;
    }
    part = wave_sum(part);
    if (lane == 0) msum[wv] = part;
    __syncthreads();
    const double m = ws_row_mass(msum);
    const double inv = 1.0 / fmax(m, taud);
    const double padd = fmax(taud - m, 0.0);              // the pad weight in float64 (fsw_common.h: pad_residual)
    auto weight_of = [&](int id) -> double { return id == D ? padd : wrow[id + id / M]; };

    for (int grp = blockIdx.y; grp < ngroups; grp += gridDim.y) {
      const int k0 = grp * SC;
#include "wsort_gather.inc"
      __syncthreads();                                    // the tile, and (first group) the row's weights and zeroed sums
      for (int kk = wv; kk < SC; kk += 4) {
        const int k = k0 + kk;
        if (k >= S) break;
        float* line = tile + kk * LINE;
        const float graw = g[(int64_t)node * ldg + gcol0 + k];
        const float gi = out_scale * graw;
        if (graw == 0.f) {                                // zero key gradients, nothing else (wave-uniform)
#pragma unroll
          for (int j = 0; j < M; ++j) {
            const int t = lane * M + j;
            if (t < D) line[t + t / M] = 0.f;
          }
          continue;
        }
        WaveLine64<M> ln;
#pragma unroll
        for (int j = 0; j < M; ++j) {
          const int t = lane * M + j;
          ln.e[j] = pack_key_index(t < Dtot ? line[lane * (M + 1) + j] : __builtin_inff(), t);
        }
        ln.sort();
        const double xi = (double)freqs[k];
        double lanew = 0.0;   // (a copy of the loop in k_embed_wsort_bwd)
#pragma unroll
        for (int j = 0; j < M; ++j) lanew += (lane * M + j < Dtot) ? weight_of(ln.index(j)) : 0.0;
        const double cstart = wave_exclusive_scan_f64(lanew);
        // forward over the lane's ranks: gkey into the element's place of the line (every lane has read its keys: the line is free),
        // gfreq, the lane's sums of q and of the HC terms, and h(c1) of every rank
        const double gd = (double)out_scale * (double)graw * inv;
        double c = cstart, c0 = c * inv, Fp, dFp, hstart;
        F_dF_h(xi, c0, Fp, dFp, hstart);
        double h1[M];
        double gf = 0.0, HC = 0.0, Q = 0.0, hp = hstart;
#pragma unroll
        for (int j = 0; j < M; ++j) {
          const int id = ln.index(j);
          const bool valid = lane * M + j < Dtot;
          c += valid ? weight_of(id) : 0.0;
          const double c1 = c * inv;
          double F, dF, h;
          F_dF_h(xi, c1, F, dF, h);
          const double kd = valid ? (double)ln.key(j) : 0.0;   // the +inf fillers beyond the line: weight 0, key taken as 0
          if (valid) {
            if (id < D) line[id + id / M] = gi * (float)(F - Fp);   // the pad element (id == D) has no source row
            gf = fma((double)gi * (dF - dFp), kd, gf);
          }
          Q += (h - hp) * kd;
          HC += (h * c1 - hp * c0) * kd;
          h1[j] = h;
          Fp = F;
          dFp = dF;
          hp = h;
          c0 = c1;
        }
        gf = wave_sum(gf);
        if (lane == 0 && gfreq) atomicAdd(gfreq + k, (float)gf);
        // R(t) = h(c1_t) key_t + sum of q over the ranks after t: the lanes above, then the lane's own suffix
        const double above = wave_reverse_exclusive_scan_f64(Q);
        HC = wave_sum(HC);
        double suf = above, rpad = 0.0;
#pragma unroll
        for (int j = M - 1; j >= 0; --j) {               // back over the lane's ranks; R overwrites h
          const int id = ln.index(j);
          const bool valid = lane * M + j < Dtot;
          const double kd = valid ? (double)ln.key(j) : 0.0;
          const double hprev = j > 0 ? h1[j > 0 ? j - 1 : 0] : hstart;
          const double q = (h1[j] - hprev) * kd;
          const double R = h1[j] * kd + suf;
          suf += q;
          if (valid && id == D) rpad = R;
          h1[j] = R;
        }
        const double Rpad = wave_sum(rpad);              // one lane holds element D
        const double corr = (m <= taud ? Rpad : 0.0) + (m >= taud ? HC : 0.0);
#pragma unroll
        for (int j = 0; j < M; ++j) {
          const int id = ln.index(j);
          const double v = gd * (h1[j] - corr);
          if (lane * M + j < Dtot && id < D && v != 0.0) atomicAdd(gacc + id + id / M, v);
        }
      }
      __syncthreads();
      for (int i = threadIdx.x; i < D * SC; i += blockDim.x) {
        const int kk = i % SC, t = i / SC;
        if (k0 + kk < S) gkey[(int64_t)(start + t) * ldk + k0 + kk] = tile[kk * LINE + t + t / M];
      }
      __syncthreads();
    }
    // every group's barrier lies behind: the sums are complete
    for (int t = threadIdx.x; t < D; t += blockDim.x) {
      const double v = gacc[t + t / M];
      if (v != 0.0) atomicAdd(gw + start + t, (float)v);
    }
    __syncthreads();                                      // the next row zeroes the sums
  }
}

template <int M>
static int launch_wsort_w_bwd(const fsw_embed_args& a, const float* w_lo, int bin_lo, int bin_hi, const float* g, int64_t ldg, float* gkey,
                              int64_t ldk, float* gfreq, float* gw, hipStream_t stream) {
  const int64_t rows = bin_rows_or(a, bin_lo, bin_hi, a.num_rows);
  if (rows <= 0) return 0;
  constexpr int bytes = (2 * 8 + 4 * wsw_slices<M>()) * ws_line<M>();
  static_assert(bytes <= ws_lds_bytes<M>(), "the tile and the two float64 lines fit the instance's LDS");
  FSW_SET_MAX_LDS_ONCE((k_embed_wsort_w_bwd<M>), bytes);
  dim3 grid((unsigned)std::min<int64_t>(rows, 1 << 14), (unsigned)std::min<int64_t>(kWsSplitY, ceil_div(a.S, wsw_slices<M>())));
  k_embed_wsort_w_bwd<M><<<grid, 256, bytes, stream>>>(a.rowptr, a.col, a.w, w_lo, a.perm, a.bin_start, bin_lo, bin_hi, a.Xp, a.ldp, a.S, a.freqs,
                                                       a.tau, g, ldg, a.has_mass, a.out_scale, gfreq, gkey, ldk, gw);
  FSW_LAUNCH_CHECK();
  return 0;
}

// rows of kWRegMaxDeg + 1 = 25 .. kWSortMaxDeg neighbours: a line of D + 1 elements fits 64 M
int launch_embed_wsort_w_bwd(const fsw_embed_args& a, const float* w_lo, const float* g, int64_t ldg, float* gkey, int64_t ldk, float* gfreq,
                             float* gw, hipStream_t stream) {
  static_assert(kWSortMaxDeg == 1024 && kWSortLastBin == FSW_BIN_LDS0 + 1, "the class ends with the LDS bin of 513 .. 1024 neighbours");
  int rc;
#define FSW_WSW(M, LO, HI) \
  if ((rc = launch_wsort_w_bwd<M>(a, w_lo, LO, HI, g, ldg, gkey, ldk, gfreq, gw, stream))) return rc
  FSW_WSW(32, FSW_BIN_LDS0 + 1, FSW_BIN_LDS0 + 1);         // 513 .. 1024, long rows first
  FSW_WSW(16, FSW_BIN_LDS0, FSW_BIN_LDS0);                 // 257 .. 512
  FSW_WSW(8, FSW_BIN_LDS0 - 1, FSW_BIN_LDS0 - 1);          // 193 .. 256
  FSW_WSW(4, kWRegMaxDeg + 1, FSW_BIN_LDS0 - 2);                       // 25 .. 192: the exact bins 25 .. 32 and the mid bins up to 192
#undef FSW_WSW
  return 0;
}

}  // namespace fsw
