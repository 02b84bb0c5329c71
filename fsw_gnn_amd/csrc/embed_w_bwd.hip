// Backward of the fused neighbourhood kernel WITH the gradient of the weights, register path, general weights.  gfx950.
//
// k_embed_reg_weighted_bwd (embed_bwd.hip) treats the weights as constants; the only kernel that differentiates them is the generic
// one (embed_generic.hip: a 256-thread workgroup per row, a float64 bitonic sort in LDS per slice).  This file adds gw to the register
// form for rows of 1 .. kWRegMaxDeg neighbours: one wavefront per (row tile, 64-slice chunk), lane = slice, the row's keys in
// registers, the pad element (key 0) as element D, cumulative weights from D(D+1)/2 compares with ties by element index,
// coefficients in float64.  With (embed_generic.hip)
//     H_t = h(c_t) (p_(t) - p_(t+1)),  h(c) = 2 (1 + xi) cos(2 pi xi c),  R(r) = sum_{t >= r} H_t
//     d out / d a_j = [ R(rank_j) - [m <= tau] R(rank_pad) - [m >= tau] sum_t H_t c_t ] / M
// summation by parts removes the sort and the successor key: for element u with key_u, c1_u = cum_u / M, c0_u = (cum_u - w_u) / M,
//     q_u = (h(c1_u) - h(c0_u)) key_u
//     R(rank_u)   = h(c1_u) key_u + sum_{v sorted after u} q_v          (a second compare pass of the shape of the one for cum)
//     sum_t H_t c_t = sum_u (h(c1_u) c1_u - h(c0_u) c0_u) key_u
// The pad element has key 0: q_pad = 0, it adds to no other element, and R(rank_pad) = sum of q_u over the keys > 0 (the pad is the
// last element, so it sorts after every other zero key).
// The per-slice contributions of an entry are summed in float64 over the wave's 64 lanes (a reduce-scatter: log2 P halving steps on
// the P = 2^ceil(log2 D) values, then an all-reduce over the remaining lane bits -- about P + 6 shuffles instead of 6 D), and lanes
// 0 .. P - 1 issue ONE float32 atomic each to D consecutive floats of gw.  gkey and gfreq come out of the same pass with the
// expressions of k_embed_reg_weighted_bwd.
// w_lo (nullable): the float32 remainder of weights the host holds in float64; w + w_lo is summed in float64 where the weights are
// loaded (d out / d w at frequency xi feels a weight's rounding times 2 pi xi: include/fsw_hip.h, fsw_embed_backward_w_lo_f32).
#include "embed_launch.h"
#include "weighted_coef.h"

namespace fsw {

constexpr int kWBwdRows = 32;
// Rows above kWRegMaxDeg (embed_launch.h) go to the wave-sort kernels of embed_w_sort_bwd.hip, rows above kWSortMaxDeg to the
// scratch-line kernels of embed_w_long_bwd.hip.  24, not FSW_REG_MAX_DEG: the form below
// for 25 .. 32 neighbours (key, cum / R and q of 32 elements live at once) spills 244 - 324 bytes per lane at 512 registers; DESIGN.md
// has the table.
static_assert(kWRegMaxDeg <= FSW_REG_MAX_DEG, "the degree bins are exact up to FSW_REG_MAX_DEG only");

constexpr int w_pow2(int d) { int p = 1; while (p < d) p <<= 1; return p; }
constexpr int w_log2(int p) { int l = 0; while ((1 << l) < p) ++l; return l; }

// v[0 .. N-1] per lane -> the sum over all 64 lanes of ONE of them: lane l < P ends with entry bitreverse(l) (log2 P bits)
template <int N>
__device__ __forceinline__ double wave_reduce_scatter(double* v, int lane, int off) {
  if constexpr (N == 1) {
    double r = v[0];
    for (; off < kWave; off <<= 1) r += __shfl_xor(r, off);
    return r;
  } else {
    const bool hi = (lane & off) != 0;
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
      const double send = hi ? v[i] : v[i + N / 2];
      const double keep = hi ? v[i + N / 2] : v[i];
      v[i] = keep + __shfl_xor(send, off);
    }
    return wave_reduce_scatter<N / 2>(v, lane, off << 1);
  }
}

template <int DEG>
__device__ __forceinline__ void w_bwd_rows(int p, int pe, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                           const float* __restrict__ w, const float* __restrict__ w_lo,
                                           const int32_t* __restrict__ perm,
                                           const float* __restrict__ Xp, int64_t ldp, const float* __restrict__ freqs, float tau,
                                           const float* __restrict__ g, int64_t ldg, int gcol0, float out_scale,
                                           float* __restrict__ gfreq, int k, int kc, bool kvalid, float* __restrict__ gkey,
                                           int64_t ldk, float* __restrict__ gw) {
  constexpr int P = w_pow2(DEG), L = w_log2(P);
  const int lane = lane_id();
  int myj = 0;                                    // the entry whose sum this lane ends up with
  if constexpr (L > 0) myj = (int)(__brev((unsigned)lane) >> (32 - L));
  const double xi = (double)freqs[kc];
  const double taud = (double)tau;
  float gf = 0.f;
  for (; p < pe; ++p) {
    const int node = perm[p];
    const int start = rowptr[node];
    const float graw = kvalid ? g[(int64_t)node * ldg + gcol0 + k] : 0.f;
    const float gi = out_scale * graw;
    float key[DEG];
    double wr[DEG];                               // w + w_lo: the weight in float64 (wave-uniform)
    double m = 0.0;
#pragma unroll
    for (int t = 0; t < DEG; ++t) {
      key[t] = Xp[(int64_t)col[start + t] * ldp + kc];
      wr[t] = (double)w[start + t] + (w_lo ? (double)w_lo[start + t] : 0.0);
      m += wr[t];
    }
    const double inv = 1.0 / fmax(m, taud);
    const double padd = fmax(taud - m, 0.0);      // the pad weight in float64, as in the forward (fsw_common.h: pad_residual)
    double cum[DEG];
#pragma unroll
    for (int t = 0; t < DEG; ++t) cum[t] = wr[t] + (0.f < key[t] ? padd : 0.0);   // the pad element sorts ahead of keys > 0
#pragma unroll
    for (int u = 0; u < DEG; ++u)
#pragma unroll
      for (int t = u + 1; t < DEG; ++t) {
        const bool before = key[t] < key[u];      // ties keep element order, like a stable sort
        cum[u] += before ? wr[t] : 0.0;
        cum[t] += before ? 0.0 : wr[u];
      }
    // coefficients: gkey and gfreq as in k_embed_reg_weighted_bwd; q and the head term of R for the weights
    double q[DEG], R[P];
    double HC = 0.0, Rpad = 0.0;
#pragma unroll
    for (int t = 0; t < DEG; ++t) {
      const double c1 = cum[t] * inv, c0 = (cum[t] - wr[t]) * inv;
      double F1, dF1, h1, F0, dF0, h0;
      F_dF_h(xi, c1, F1, dF1, h1);
      F_dF_h(xi, c0, F0, dF0, h0);
      gf = fmaf(gi * (float)(dF1 - dF0), key[t], gf);
      if (kvalid) gkey[(int64_t)(start + t) * ldk + k] = gi * (float)(F1 - F0);
      const double kd = (double)key[t];
      q[t] = (h1 - h0) * kd;
      R[t] = h1 * kd;
      HC += (h1 * c1 - h0 * c0) * kd;
      Rpad += 0.f < key[t] ? q[t] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < DEG; ++u)
#pragma unroll
      for (int t = u + 1; t < DEG; ++t) {
        const bool before = key[t] < key[u];      // t sorts ahead of u: u is among the elements after t
        R[t] += before ? q[u] : 0.0;
        R[u] += before ? 0.0 : q[t];
      }
    const double corr = (m <= taud ? Rpad : 0.0) + (m >= taud ? HC : 0.0);
    const double gd = (double)out_scale * (double)graw * inv;
#pragma unroll
    for (int t = 0; t < DEG; ++t) R[t] = gd * (R[t] - corr);
#pragma unroll
    for (int t = DEG; t < P; ++t) R[t] = 0.0;
    const double sum = wave_reduce_scatter<P>(R, lane, 1);
    if (lane < P && myj < DEG && sum != 0.0) atomicAdd(gw + start + myj, (float)sum);
  }
  if (kvalid && gfreq) atomicAdd(gfreq + k, gf);
}

// one kernel per degree range: the register budget is that of the range's longest row
template <int DLO, int DHI>
__global__ void __launch_bounds__(256) k_embed_reg_w_bwd(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         const float* __restrict__ w, const float* __restrict__ w_lo,
                                                         const int32_t* __restrict__ perm,
                                                         const int32_t* __restrict__ bin_start, const float* __restrict__ Xp,
                                                         int64_t ldp, int S, const float* __restrict__ freqs, float tau,
                                                         const float* __restrict__ g, int64_t ldg, int gcol0, float out_scale,
                                                         float* __restrict__ gfreq, float* __restrict__ gkey, int64_t ldk,
                                                         float* __restrict__ gw) {
#include "slice_chunk.inc"   // chunk, k, kvalid, kc; a wavefront behind the last slice returns
  int D, p = 0, pe = 0;
  if (!find_degree_tile<kWBwdRows>(bin_start, DLO, DHI, (int)blockIdx.x, D, p, pe)) return;
  switch (D) {
#define X(d)                                                                                                                    \
  case d:                                                                                                                       \
    if constexpr (d >= DLO && d <= DHI)                                                                                         \
      w_bwd_rows<d>(p, pe, rowptr, col, w, w_lo, perm, Xp, ldp, freqs, tau, g, ldg, gcol0, out_scale, gfreq, k, kc, kvalid, gkey, ldk, \
                    gw);                                                                                                        \
    break;
    FSW_CASES_1_32(X)   // fsw_common.h; the cases above kWRegMaxDeg are empty
#undef X
    default:
      break;
  }
}

template <int DLO, int DHI>
static int launch_w_bwd(const fsw_embed_args& a, const float* w_lo, int64_t nreg, const float* g, int64_t ldg, float* gkey, int64_t ldk, float* gfreq,
                        float* gw, hipStream_t stream) {
  int64_t tiles = ceil_div(nreg, kWBwdRows) + (DHI - DLO + 1);   // every bin ends with at most one partial tile
  if (a.bin_start_host) {
    tiles = 0;
    for (int d = DLO; d <= DHI; ++d) tiles += ceil_div((int64_t)(a.bin_start_host[d + 1] - a.bin_start_host[d]), kWBwdRows);
  }
  if (tiles == 0) return 0;
  dim3 grid((unsigned)tiles, (unsigned)ceil_div(a.S, 4 * kWave));
  k_embed_reg_w_bwd<DLO, DHI><<<grid, 256, 0, stream>>>(a.rowptr, a.col, a.w, w_lo, a.perm, a.bin_start, a.Xp, a.ldp, a.S, a.freqs, a.tau, g,
                                                        ldg, a.has_mass, a.out_scale, gfreq, gkey, ldk, gw);
  FSW_LAUNCH_CHECK();
  return 0;
}

}  // namespace fsw

using namespace fsw;

// an upper bound since the rows of 25 .. kWSortMaxDeg neighbours left the generic kernel: what it returned before, for every input
// (36 bytes per element of the padded line for at least one workgroup: embed_w_long_bwd.hip takes 20 per wavefront)
extern "C" size_t fsw_embed_backward_w_scratch_bytes(int64_t max_degree, int64_t num_rows) {
  return max_degree > kWRegMaxDeg ? fsw_embed_generic_scratch_bytes(max_degree, num_rows) : 0;
}

// the largest degree that needs no scratch
extern "C" int fsw_embed_backward_w_tuned_max_degree(void) { return kWSortMaxDeg; }

static int embed_backward_w(const fsw_embed_args* args, const float* w_lo, int64_t max_degree, const float* g, int64_t ldg,
                            float* gkey, int64_t ldk, float* gfreq, float* gw, void* scratch, size_t scratch_bytes,
                            hipStream_t stream) {
  FSW_REQUIRE(args && g && gkey && gw, "fsw_embed_backward_w_f32: null pointer");
  const fsw_embed_args& a = *args;
  FSW_REQUIRE(a.rowptr && a.col && a.w && a.perm && a.bin_start && a.Xp && a.freqs,
              "fsw_embed_backward_w_f32: null pointer in args (the weights w are required)");
  FSW_REQUIRE(!a.efeat, "fsw_embed_backward_w_f32: edge features are not supported");
  FSW_REQUIRE(a.S >= 1 && a.ldp >= a.S && ldg >= a.S + a.has_mass && ldk >= a.S && a.tau > 0.f && max_degree >= 0,
              "fsw_embed_backward_w_f32: bad sizes");
  if (a.num_rows <= 0) return 0;
  const int64_t nreg = a.num_reg_rows < 0 ? a.num_rows : a.num_reg_rows;
  int rc;
  // rows above kWSortMaxDeg neighbours: one wavefront per (row, kWLongSlices slices) on a scratch line (embed_w_long_bwd.hip), every bin
  // that has rows.  The longest rows first; it is also the only launcher that can refuse the buffer, before anything is launched.
  bool longer = max_degree > kWSortMaxDeg;
  if (longer && a.bin_start_host) longer = a.bin_start_host[FSW_NUM_BINS] > a.bin_start_host[kWSortLastBin + 1];
  else if (longer) longer = a.num_lds_rows != 0 || a.num_global_rows != 0;   // -1: unknown
  if (longer) {
    FSW_REQUIRE(scratch, "fsw_embed_backward_w_f32: rows above %d neighbours need scratch (fsw_embed_backward_w_scratch_bytes)",
                kWSortMaxDeg);
    if ((rc = launch_embed_w_long_bwd(a, w_lo, max_degree, g, ldg, gkey, ldk, gfreq, gw, scratch, scratch_bytes, stream))) return rc;
  }
  if (nreg > 0) {
    // long rows first
    if ((rc = launch_w_bwd<17, 24>(a, w_lo, nreg, g, ldg, gkey, ldk, gfreq, gw, stream))) return rc;
    if ((rc = launch_w_bwd<9, 16>(a, w_lo, nreg, g, ldg, gkey, ldk, gfreq, gw, stream))) return rc;
    if ((rc = launch_w_bwd<1, 8>(a, w_lo, nreg, g, ldg, gkey, ldk, gfreq, gw, stream))) return rc;
  }
  // 25 .. kWSortMaxDeg neighbours: one (row, slice) line per wavefront (embed_w_sort_bwd.hip), every bin that has rows
  if (max_degree > kWRegMaxDeg && (rc = launch_embed_wsort_w_bwd(a, w_lo, g, ldg, gkey, ldk, gfreq, gw, stream))) return rc;
  return 0;
}

extern "C" int fsw_embed_backward_w_long_slices(void) { return kWLongSlices; }

extern "C" int fsw_embed_backward_w_f32(const fsw_embed_args* args, int64_t max_degree, const float* g, int64_t ldg, float* gkey,
                                        int64_t ldk, float* gfreq, float* gw, void* scratch, size_t scratch_bytes,
                                        fsw_stream_t stream) {
  return embed_backward_w(args, nullptr, max_degree, g, ldg, gkey, ldk, gfreq, gw, scratch, scratch_bytes,
                          reinterpret_cast<hipStream_t>(stream));
}

extern "C" int fsw_embed_backward_w_lo_f32(const fsw_embed_args* args, const float* w_lo, int64_t max_degree, const float* g,
                                           int64_t ldg, float* gkey, int64_t ldk, float* gfreq, float* gw, void* scratch,
                                           size_t scratch_bytes, fsw_stream_t stream) {
  return embed_backward_w(args, w_lo, max_degree, g, ldg, gkey, ldk, gfreq, gw, scratch, scratch_bytes,
                          reinterpret_cast<hipStream_t>(stream));
}
