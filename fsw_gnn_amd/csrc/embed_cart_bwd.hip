// Backward of the tuned float32 Cartesian forward (embed_cart.hip) with respect to the keys and the frequencies.  gfx950.
//
//   out[r, s F + f] = out_scale sum_t C_f(t) p_(t),   C_f(t) = F(xi_f; c_t) - F(xi_f; c_{t-1})      (fourier_coef.h)
//   gkey[e, s]  = out_scale sum_f g[r, s F + f] C_f(rank_s(e))                          stored for every entry e of the graph
//   gfreq[f]   += out_scale sum_{r, s} g[r, s F + f] sum_t dC_f(t)/dxi p_(t)
// The degree classes are the forward's, on the same degree bins, so that the two stay in step; every line is sorted ONCE with its
// entry indices (equal keys keep entry order, as in the generic kernel: the project's rule) and read out at all F frequencies:
//   1 <= D <= 32     one lane per (row, slice).  Unit weights with tau <= 1: the coefficient rows of fsw_unit_coeff_table and
//                    fsw_unit_dcoeff_table are wave-uniform and come through the constant address space, kFC frequencies per step;
//                    the lanes' kFC frequency partials are summed across the wavefront by a transposing butterfly (kFC + 2 lane
//                    exchanges instead of 6 kFC).  General weights: float64 cumulative weights, one F / dF evaluation per
//                    (element, frequency) -- the value at c_t is the lower bound of element t + 1.  The key gradients go through
//                    a lane-private LDS row indexed by the entry, so that the stores are runs of S floats per entry.
//   33 <= L <= 2048  one wavefront per (row, slice), the line sorted across it as 64-bit (key, index) words (wave_sort.h); every
//                    lane keeps its M sorted elements and accumulates their gradients over the frequency loop (g_f and xi_f
//                    wave-uniform); the lower bound of a lane's first element comes from its neighbour lane.
//   2049 <= D <= 32768, unit weights with tau <= 1: one wavefront per (row, slice) in a scratch line of packed words
//                    (embed_cart_hub_bwd.hip: k_cart_bwd_long), 12 bytes of scratch per element of the padded line and wavefront.
//   2049 <= L <= 16384, general weights: one wavefront per (row, slice) in a scratch line of packed words, the weights re-read by
//                    entry index (embed_cart_hub_w_bwd.hip: k_cart_bwd_long_w), 12 bytes of scratch per element of the padded line.
//   longer lines     (general weights above 16384 elements, any row above 32768; any length) one workgroup of four wavefronts per
//                    (row, slice): the packed words in sorted runs in a scratch line, merge path above a run
//                    (embed_giant_cart_bwd.hip: k_cart_giant_bwd), 16 bytes of scratch per element of the line and workgroup.
//                    With args->flags & FSW_CART_SPLIT_BWD_LINES (unit weights: embed_split_cart_bwd.hip) or FSW_CART_SPLIT_W_BWD_LINES
//                    (general weights: embed_split_cart_w_bwd.hip) one line is split over the workgroups of a launch per phase.
// No float32 row runs on the generic kernel (k_embed_generic, embed_generic.hip).
// gfreq: the register class sums a workgroup's partials in LDS, the wavefront class across the wavefront; one float atomic per
// (workgroup resp. wavefront, frequency).
#include <algorithm>
#include "embed_cart.h"
#include "embed_launch.h"
#include "fourier_coef.h"
#include "sortnet.h"
#include "wave_sort.h"

namespace fsw {

namespace {

constexpr int kFC = 8;            // frequencies per step of the unit-weight register path
constexpr int kGfLds = 2048;      // up to this many frequencies a workgroup sums its gfreq partials in LDS (above: one atomic per wavefront)
constexpr int kRegLd = FSW_REG_MAX_DEG + 1;   // floats per lane of the transposing LDS rows (odd: conflict-free)

struct CartBwd {
  const int32_t* rowptr;
  const int32_t* col;
  const float* w;
  const int32_t* perm;
  const int32_t* bin_start;
  const float* Xp;
  int64_t ldp;
  const float* freqs;
  int S, F;
  float tau;
  const float* table;
  const float* dtable;
  int64_t ldt, lddt;
  const float* g;
  int64_t ldg;
  int gcol0;
  float out_scale;
  float* gkey;
  int64_t ldk;
  float* gfreq;
};

// one lane adds a wavefront's partial sum of frequency f
__device__ __forceinline__ void add_gfreq(const CartBwd& a, float* sgf, int f, float v) {
  if (!a.gfreq) return;
  if (a.F <= kGfLds) atomicAdd(sgf + f, v);
  else atomicAdd(a.gfreq + f, v);
}

// part[j], j < kFC, of every lane -> sums over the wavefront: each exchange halves the values a lane carries (the lane keeps the half
// its bit selects and adds the partner's), then three plain steps.  Afterwards lane l < kFC holds the sum of value bitrev3(l) in part[0].
__device__ __forceinline__ void transpose_sum(float (&part)[kFC], int lane) {
  static_assert(kFC == 8, "three halving steps");
  {
    const bool hi = lane & 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float keep = hi ? part[j + 4] : part[j], send = hi ? part[j] : part[j + 4];
      part[j] = keep + xor_lane<1>(send);
    }
  }
  {
    const bool hi = lane & 2;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float keep = hi ? part[j + 2] : part[j], send = hi ? part[j] : part[j + 2];
      part[j] = keep + xor_lane<2>(send);
    }
  }
  {
    const bool hi = lane & 4;
    const float keep = hi ? part[1] : part[0], send = hi ? part[0] : part[1];
    part[0] = keep + xor_lane<4>(send);
  }
  part[0] += xor_lane<8>(part[0]);
  part[0] += xor_lane<16>(part[0]);
  part[0] += xor_lane<32>(part[0]);
}

// VEC: 16-byte coefficient loads (F % kFC == 0, 16-byte aligned table rows: launch condition on the host)
template <int D, bool VEC>
__device__ __forceinline__ void cart_bwd_reg_unit(const CartBwd& a, int p, int pe, float* sgf, float* tr) {
  const int items = (pe - p) * a.S;
  const int lane = lane_id();
  ConstAS<float>* tab = as_const(a.table + (int64_t)(D * (D - 1) / 2) * a.ldt);
  ConstAS<float>* dtab = as_const(a.dtable + (int64_t)(D * (D - 1) / 2) * a.lddt);
  float* mine = tr + threadIdx.x * kRegLd;
  for (int i0 = 0; i0 < items; i0 += blockDim.x) {      // every lane takes part in the wavefront sums: idle ones carry g = 0
    const int i = i0 + threadIdx.x;
    const bool valid = i < items;
    const int ic = valid ? i : items - 1;
    const int r = ic / a.S, s = ic - r * a.S;
    const int node = a.perm[p + r];
    const int start = a.rowptr[node];
    IndexedNet<D> net;
#pragma unroll
    for (int t = 0; t < D; ++t) {
      net.k[t] = a.Xp[(int64_t)a.col[start + t] * a.ldp + s];
      net.w[t] = __int_as_float(t);
    }
    sort_network<D>(net);
    float G[D];
#pragma unroll
    for (int t = 0; t < D; ++t) G[t] = 0.f;
    const float* grow = a.g + (int64_t)node * a.ldg + a.gcol0 + (int64_t)s * a.F;
    const float sc = valid ? a.out_scale : 0.f;
    for (int f0 = 0; f0 < a.F; f0 += kFC) {
      float gv[kFC], part[kFC];
#pragma unroll
      for (int j = 0; j < kFC; ++j) {
        gv[j] = (VEC || f0 + j < a.F) ? sc * grow[min(f0 + j, a.F - 1)] : 0.f;
        part[j] = 0.f;
      }
#pragma unroll
      for (int t = 0; t < D; ++t) {
        float cf[kFC], df[kFC];
        if constexpr (VEC) {
#pragma unroll
          for (int q = 0; q < kFC; q += 4) {
            const float4 c4 = *reinterpret_cast<ConstAS<float4>*>(tab + (int64_t)t * a.ldt + f0 + q);
            const float4 d4 = *reinterpret_cast<ConstAS<float4>*>(dtab + (int64_t)t * a.lddt + f0 + q);
            cf[q] = c4.x; cf[q + 1] = c4.y; cf[q + 2] = c4.z; cf[q + 3] = c4.w;
            df[q] = d4.x; df[q + 1] = d4.y; df[q + 2] = d4.z; df[q + 3] = d4.w;
          }
        } else {
#pragma unroll
          for (int j = 0; j < kFC; ++j) {
            const int f = min(f0 + j, a.F - 1);
            cf[j] = tab[(int64_t)t * a.ldt + f];
            df[j] = dtab[(int64_t)t * a.lddt + f];
          }
        }
#pragma unroll
        for (int j = 0; j < kFC; ++j) {
          G[t] = fmaf(gv[j], cf[j], G[t]);
          part[j] = fmaf(df[j], net.k[t], part[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < kFC; ++j) part[j] *= gv[j];
      transpose_sum(part, lane);
      const int f = f0 + ((lane & 1) << 2 | (lane & 2) | (lane & 4) >> 2);
      if (lane < kFC && f < a.F) add_gfreq(a, sgf, f, part[0]);
    }
#pragma unroll
    for (int t = 0; t < D; ++t) mine[__float_as_int(net.w[t])] = G[t];       // sorted position -> entry order (lane-private row)
    if (valid) {
#pragma unroll
      for (int u = 0; u < D; ++u) a.gkey[(int64_t)(start + u) * a.ldk + s] = mine[u];
    }
  }
}

template <int D>
__device__ __forceinline__ void cart_bwd_reg_weighted(const CartBwd& a, int p, int pe, float* sgf, float* tr) {
  const int items = (pe - p) * a.S;
  const int lane = lane_id();
  const double tau = (double)a.tau;
  float* mine = tr + threadIdx.x * kRegLd;
  for (int i0 = 0; i0 < items; i0 += blockDim.x) {
    const int i = i0 + threadIdx.x;
    const bool valid = i < items;
    const int ic = valid ? i : items - 1;
    const int r = ic / a.S, s = ic - r * a.S;
    const int node = a.perm[p + r];
    const int start = a.rowptr[node];
    IndexedNet<D + 1> net;
    double m = 0.0;
#pragma unroll
    for (int t = 0; t < D; ++t) {
      net.k[t] = a.Xp[(int64_t)a.col[start + t] * a.ldp + s];
      net.w[t] = __int_as_float(t);
      m += (double)(a.w ? a.w[start + t] : 1.f);
    }
    net.k[D] = 0.f;                                   // the reference's pad element at x = 0, last among equal keys
    net.w[D] = __int_as_float(D);
    const double padw = fmax(tau - m, 0.0);           // float64: it enters the float64 cumulative weight (fsw_common.h: pad_residual)
    const double inv = 1.0 / fmax(m, tau);
    sort_network<D + 1>(net);
    double cn[D + 1];
    double cum = 0.0;
#pragma unroll
    for (int t = 0; t <= D; ++t) {
      const int id = __float_as_int(net.w[t]);
      cum += id < D ? (double)(a.w ? a.w[start + id] : 1.f) : padw;
      cn[t] = cum * inv;
    }
    float G[D + 1];
#pragma unroll
    for (int t = 0; t <= D; ++t) G[t] = 0.f;
    const float* grow = a.g + (int64_t)node * a.ldg + a.gcol0 + (int64_t)s * a.F;
    const float sc = valid ? a.out_scale : 0.f;
    for (int f = 0; f < a.F; ++f) {
      const FCoef fc((double)as_const(a.freqs)[f]);
      const float gv = sc * grow[f];
      double Fp = 0.0, dFp = 0.0;                     // F(0) = dF(0) = 0
      float ds = 0.f;
#pragma unroll
      for (int t = 0; t <= D; ++t) {
        double Fv, dFv;
        F_dF(fc, cn[t], Fv, dFv);
        G[t] = fmaf(gv, (float)(Fv - Fp), G[t]);
        ds = fmaf((float)(dFv - dFp), net.k[t], ds);
        Fp = Fv;
        dFp = dFv;
      }
      const float tot = wave_sum(gv * ds);
      if (lane == 0) add_gfreq(a, sgf, f, tot);
    }
#pragma unroll
    for (int t = 0; t <= D; ++t) {
      const int id = __float_as_int(net.w[t]);
      if (id < D) mine[id] = G[t];                    // the pad element has no entry
    }
    if (valid) {
#pragma unroll
      for (int u = 0; u < D; ++u) a.gkey[(int64_t)(start + u) * a.ldk + s] = mine[u];
    }
  }
}

template <bool UNIT, bool VEC>
__global__ void __launch_bounds__(256) k_cart_bwd_reg(const CartBwd a) {
  __shared__ float tr[256 * kRegLd];
  __shared__ float sgf[kGfLds];
  const bool lds_sum = a.gfreq && a.F <= kGfLds;
  if (lds_sum)
    for (int f = threadIdx.x; f < a.F; f += blockDim.x) sgf[f] = 0.f;
  __syncthreads();
  int D, p, pe;
  if (find_degree_tile<kCartRows>(a.bin_start, 1, FSW_REG_MAX_DEG, (int)blockIdx.x, D, p, pe)) {
    switch (D) {
#define X(d)                                                           \
  case d:                                                              \
    if constexpr (UNIT) cart_bwd_reg_unit<d, VEC>(a, p, pe, sgf, tr);  \
    else cart_bwd_reg_weighted<d>(a, p, pe, sgf, tr);                  \
    break;
      FSW_CASES_1_32(X)
#undef X
      default:
        break;
    }
  }
  __syncthreads();
  if (lds_sum)
    for (int f = threadIdx.x; f < a.F; f += blockDim.x) {
      const float v = sgf[f];
      if (v != 0.f) atomicAdd(a.gfreq + f, v);
    }
}

// One wavefront per (row, slice) for lines of up to 64 M elements; rows perm[p0 + blockIdx.x], slice blockIdx.y.
template <int M, bool WEIGHTED>
__global__ void __launch_bounds__(64) k_cart_bwd_wave(const CartBwd a, int p0) {
  constexpr int LMAX = 64 * M;
  const int lane = threadIdx.x;
  const int node = a.perm[p0 + blockIdx.x];
  const int s = blockIdx.y;
  const int start = a.rowptr[node];
  const int D = a.rowptr[node + 1] - start;
  const int L = WEIGHTED ? D + 1 : D;              // unit weights with tau <= 1: the pad element has weight 0 and is left out
  if (L > LMAX || L <= 0) return;                  // longer lines: the generic kernel
  WaveLine64<M> ln;
  double mpart = 0.0;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const int e = lane * M + j;
    float key = __builtin_inff();                  // fill elements sort behind the line
    if (e < D) {
      key = a.Xp[(int64_t)a.col[start + e] * a.ldp + s];
      mpart += (double)(a.w ? a.w[start + e] : 1.f);
    } else if (WEIGHTED && e == D) {
      key = 0.f;                                   // the pad element, last among equal keys (index D)
    }
    ln.e[j] = pack_key_index(key, e);
  }
  const double m = wave_sum(mpart);
  const double tau = (double)a.tau;
  const double inv = 1.0 / fmax(m, tau);
  const float padw = (float)fmax(tau - m, 0.0);
  const double rho = pad_residual(tau - m, padw);  // what the float wt[] loses of the pad weight: added where the walk passes the pad (fsw_common.h)
  ln.sort();
  float key[M];
  int idx[M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    key[j] = lane * M + j < L ? ln.key(j) : 0.f;   // fill elements: coefficient 0, and no inf in the frequency sums
    idx[j] = ln.index(j);
  }
  // normalised cumulative weight up to and including each of this lane's elements
  double cbase = 0.0;
  float wt[WEIGHTED ? M : 1];
  if constexpr (WEIGHTED) {
    double pre = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const int id = idx[j];
      wt[j] = id < D ? (a.w ? a.w[start + id] : 1.f) : (id == D ? padw : 0.f);
      pre += (double)wt[j] + (id == D ? rho : 0.0);
    }
    cbase = wave_exclusive_scan_f64(pre);
  }
  float G[M];
#pragma unroll
  for (int j = 0; j < M; ++j) G[j] = 0.f;
  const float* grow = a.g + (int64_t)node * a.ldg + a.gcol0 + (int64_t)s * a.F;
  const double invD = 1.0 / (double)D;
  for (int f = 0; f < a.F; ++f) {
    const FCoef fc((double)a.freqs[f]);
    const float gv = a.out_scale * grow[f];
    double F0 = 0.0, dF0 = 0.0, Fp = 0.0, dFp = 0.0, c = cbase;
    float ds = 0.f;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const int t = lane * M + j;
      double cn;
      if constexpr (WEIGHTED) {
        c += (double)wt[j] + (idx[j] == D ? rho : 0.0);
        cn = c * inv;
      } else {
        cn = (double)min(t + 1, D) * invD;
      }
      double Fv, dFv;
      F_dF(fc, cn, Fv, dFv);
      if (j == 0) {
        F0 = Fv;
        dF0 = dFv;
      } else {
        G[j] = fmaf(gv, (float)(Fv - Fp), G[j]);
        ds = fmaf((float)(dFv - dFp), key[j], ds);
      }
      Fp = Fv;
      dFp = dFv;
    }
    // the lower bound of this lane's first element is the value at the last element of the lane below (lane 0: F(0) = 0)
    double Fl = __shfl_up(Fp, 1), dFl = __shfl_up(dFp, 1);
    if (lane == 0) Fl = dFl = 0.0;
    G[0] = fmaf(gv, (float)(F0 - Fl), G[0]);
    ds = fmaf((float)(dF0 - dFl), key[0], ds);
    const float tot = wave_sum(gv * ds);
    if (lane == 0 && a.gfreq) atomicAdd(a.gfreq + f, tot);
  }
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const int id = idx[j];
    if (lane * M + j < L && id < D) a.gkey[(int64_t)(start + id) * a.ldk + s] = G[j];
  }
}

template <int M>
int launch_cart_bwd_wave(const CartBwd& t, bool weighted, int p0, int rows, hipStream_t stream) {
  if (rows <= 0) return 0;
  dim3 grid((unsigned)rows, (unsigned)t.S);
  if (weighted) k_cart_bwd_wave<M, true><<<grid, kWave, 0, stream>>>(t, p0);
  else k_cart_bwd_wave<M, false><<<grid, kWave, 0, stream>>>(t, p0);
  FSW_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace fsw

using namespace fsw;

extern "C" int fsw_embed_cart_backward_keys_f32(const fsw_cart_args* c, const float* unit_dtable, int64_t lddt, fsw_stream_t stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  int rc;
  if ((rc = cart_check_common(c))) return rc;
  FSW_REQUIRE(c->value_dtype == 0 && c->g && c->gkey && !c->gw,
              "fsw_embed_cart_backward_keys_f32: float32, needs g and gkey, gw must be NULL (fsw_embed_cart_generic for the weights)");
  FSW_REQUIRE(c->perm && c->bin_start && c->bin_start_host, "fsw_embed_cart_backward_keys_f32: needs perm, bin_start and its host copy");
  FSW_REQUIRE(c->ldg >= (int64_t)c->has_mass + (int64_t)c->S * c->F && c->ldk >= c->S,
              "fsw_embed_cart_backward_keys_f32: bad gradient strides");
  const bool unit_fast = cart_unit_fast(c);
  FSW_REQUIRE(!unit_fast || (c->unit_table && c->ldt >= c->F && unit_dtable && lddt >= c->F),
              "fsw_embed_cart_backward_keys_f32: unit weights with tau <= 1 need unit_table and unit_dtable");
  if (c->num_rows == 0) return 0;
  const int32_t* bs = c->bin_start_host;
  // FSW_CART_SPLIT_BWD_LINES: the giant class in the split form where one exists (lines > 0), refused before any launch when the buffer is short
  const CartSplitBwdPlan split = (c->flags & FSW_CART_SPLIT_BWD_LINES) ? cart_split_bwd_plan(c) : CartSplitBwdPlan{};
  if (split.lines > 0) {
    FSW_REQUIRE(c->scratch && ((uintptr_t)c->scratch & 15) == 0 && c->scratch_bytes >= split.bytes,
                "fsw_embed_cart_backward_keys_f32: FSW_CART_SPLIT_BWD_LINES needs a 16-byte aligned scratch buffer of "
                "fsw_embed_cart_split_backward_scratch_bytes(args) bytes");
  }
  // FSW_CART_SPLIT_W_BWD_LINES: the same for general weights (a call has one of the two forms at most: unit weights or not)
  const CartSplitWBwdPlan split_w = (c->flags & FSW_CART_SPLIT_W_BWD_LINES) ? cart_split_w_bwd_plan(c) : CartSplitWBwdPlan{};
  if (split_w.lines > 0) {
    FSW_REQUIRE(c->scratch && ((uintptr_t)c->scratch & 15) == 0 && c->scratch_bytes >= split_w.bytes,
                "fsw_embed_cart_backward_keys_f32: FSW_CART_SPLIT_W_BWD_LINES needs a 16-byte aligned scratch buffer of "
                "fsw_embed_cart_split_w_backward_scratch_bytes(args) bytes");
  }

  CartBwd t;
  cart_fill_inputs_w(t, c);
  cart_fill_grads(t, c);
  t.table = c->unit_table; t.dtable = unit_dtable; t.ldt = c->ldt; t.lddt = lddt;

  // 1 <= D <= 32: one lane per (row, slice); grid = the exact number of tiles of every degree bin
  int64_t tiles = 0;
  for (int d = 1; d <= FSW_REG_MAX_DEG; ++d) tiles += ceil_div(bs[d + 1] - bs[d], kCartRows);
  if (tiles > 0) {
    const bool vec = c->F % kFC == 0 && c->ldt % 4 == 0 && lddt % 4 == 0 && (uintptr_t)c->unit_table % 16 == 0 &&
                     (uintptr_t)unit_dtable % 16 == 0;
    if (unit_fast && vec) k_cart_bwd_reg<true, true><<<(unsigned)tiles, 256, 0, stream>>>(t);
    else if (unit_fast) k_cart_bwd_reg<true, false><<<(unsigned)tiles, 256, 0, stream>>>(t);
    else k_cart_bwd_reg<false, false><<<(unsigned)tiles, 256, 0, stream>>>(t);
    FSW_LAUNCH_CHECK();
  }
  // 33 <= line <= 2048: one wavefront per (row, slice); the forward's grouping of the degree bins by keys per lane
  const int extra = unit_fast ? 0 : 1;
  rc = for_each_wave_group(bs, extra, [&](int Mb, int p0, int rows) {
    switch (Mb) {
      case 1: return launch_cart_bwd_wave<1>(t, !unit_fast, p0, rows, stream);
      case 2: return launch_cart_bwd_wave<2>(t, !unit_fast, p0, rows, stream);
      case 4: return launch_cart_bwd_wave<4>(t, !unit_fast, p0, rows, stream);
      case 8: return launch_cart_bwd_wave<8>(t, !unit_fast, p0, rows, stream);
      case 16: return launch_cart_bwd_wave<16>(t, !unit_fast, p0, rows, stream);
      default: return launch_cart_bwd_wave<32>(t, !unit_fast, p0, rows, stream);
    }
  });
  if (rc) return rc;
  // lines above kCartMaxLine elements (the classes of embed_cart.h: kCartLong): one wavefront per line in a scratch line
  if ((rc = unit_fast ? launch_cart_hub_bwd(c, stream) : launch_cart_hub_w_bwd(c, stream))) return rc;
  // the giant class (any length): sorted runs + merge path in the scratch lines of c->scratch, one workgroup per line -- or, unit weights
  // with FSW_CART_SPLIT_BWD_LINES (general weights: FSW_CART_SPLIT_W_BWD_LINES), every line split over the workgroups of a launch per phase
  if (split.lines > 0) return launch_cart_split_bwd(c, split, stream);
  if (split_w.lines > 0) return launch_cart_split_w_bwd(c, split_w, stream);
  return launch_cart_giant_bwd(c, stream);
}
