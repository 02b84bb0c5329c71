// Cartesian slice x frequency mode (reference fsw_embedding.py:241-259, 1037-1045): every slice s is sorted ONCE and its sorted
// line is read out at all F frequencies, out[r, s * F + f] (the order torch.flatten gives, :853-854).  gfx950.
//
// The diagonal kernels pair slice k with frequency k; here the sort, the cumulative weights and the gathers cost S lines per row
// and only the readout costs S * F.  Three degree classes for the tuned float32 forward (fsw_embed_cart_f32), on the CSR build
// and degree bins of fsw_graph_build and the projection Xp of fsw_project_f32:
//   1 <= D <= 32     one lane per (row, slice): the line is sorted in registers by the exact-size network of sortnet.h, then the
//                    F outputs are formed from those registers and stored as one contiguous run per lane (lanes of adjacent
//                    slices are adjacent, so a wavefront's stores cover whole lines).  Unit weights with tau <= 1 read the
//                    coefficients of fsw_unit_coeff_table built for the F frequencies (wave-uniform: every lane of a workgroup
//                    has the same D); general weights carry a float64 cumulative weight per element, as embed_reg.hip does.
//   33 <= L <= 2048  (L = D, + 1 for the pad element of general weights) one wavefront per (row, slice): the line is sorted across
//                    the wavefront (wave_sort.h, WaveLine), the sorted keys and cumulative weights are staged in LDS, and the
//                    readout lanes are (frequency, rank phase) pairs -- lane = f + NF q sums the ranks t = q (mod Q) for
//                    frequency f, Q = 64 / NF -- so that F < 64 does not leave most lanes idle; LDS reads are broadcasts.
//   2049 <= D <= 32768, unit weights with tau <= 1: one workgroup of 2 .. 16 wavefronts per (row, slice), the line in their registers
//                    (embed_cart_hub.hip: k_cart_hub, the hub machinery of the diagonal kernels), no scratch.
//   2049 <= L <= 16384, general weights: one workgroup of 2, 4 or 8 wavefronts per (row, slice), keys and weights in their registers
//                    (embed_cart_hub_w.hip: k_cart_hub_w), no scratch.
//   longer lines     (general weights above 16384 elements, any row above 32768; any length) one workgroup per (row, slice), the line
//                    in sorted blocks in a scratch line: embed_giant_cart.hip (k_cart_giant: bitonic block sweeps) and
//                    embed_giant_cart_w.hip (k_cart_mergepath_w: merge path).  Their backward: embed_giant_cart_bwd.hip; its split
//                    forms: embed_split_cart_bwd.hip (unit weights), embed_split_cart_w_bwd.hip (general weights).
//                    Unit weights with args->flags & FSW_CART_SPLIT_LINES: embed_split_cart.hip, one line split over many workgroups.
//                    General weights with args->flags & FSW_CART_SPLIT_W_LINES: embed_split_cart_w.hip, the same.
// Readout, by summation by parts of the reference's Delta_t = 2 w_t sinc(xi w_t) cos(pi xi (2 c_t - w_t)):
//   out = (1 + xi) / (pi xi) sum_t sin(2 pi xi c_t) (p_(t) - p_(t+1)),  p_(L) = 0;   xi = 0:  out = sum_t 2 c_t (p_(t) - p_(t+1)).
//
// fsw_embed_cart_generic (any degree, float32 or float64 storage, float64 arithmetic, forward and backward) is that same generic
// kernel on every row; this file only checks its arguments.  Backward, for the output gradient g:
//   gkey[e, s] = sum_f out_scale g[r, s F + f] (1 + xi_f) Delta_t(xi_f)                       (stored)
//   gfreq[f]  += sum_{r, s} out_scale g[r, s F + f] d out[r, s F + f] / d xi_f                (accumulated)
//   gw[e]     += sum_{s, f} out_scale g[r, s F + f] d out[r, s F + f] / d w_e                 (accumulated; mass column excluded)
#include <algorithm>
#include "embed_cart.h"
#include "embed_launch.h"
#include "sortnet.h"
#include "wave_sort.h"

namespace fsw {

namespace {

// ---- tuned float32 forward ------------------------------------------------------------------------------------------------
struct CartTuned {
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
  int64_t ldt;
  float* out;
  int64_t ldo;
  const float* bias;
  float out_scale;
  int has_mass, mass_fn;
  float mass_scale;
};

// VEC: four frequencies per step -- 16-byte coefficient loads (wave-uniform) and 16-byte output stores (F % 4 == 0, column has_mass of
// every row 16-byte aligned: launch condition on the host)
template <int D, bool VEC>
__device__ __forceinline__ void cart_reg_unit(const CartTuned& a, int p, int pe) {
  const int items = (pe - p) * a.S;
  ConstAS<float>* tab = as_const(a.table + (int64_t)(D * (D - 1) / 2) * a.ldt);
  for (int i = threadIdx.x; i < items; i += blockDim.x) {
    const int r = i / a.S, s = i - r * a.S;
    const int node = a.perm[p + r];
    const int start = a.rowptr[node];
    KeyNet<D> net;
#pragma unroll
    for (int t = 0; t < D; ++t) net.k[t] = a.Xp[(int64_t)a.col[start + t] * a.ldp + s];
    sort_network<D>(net);
    float* orow = a.out + (int64_t)node * a.ldo;
    const int64_t c0 = (int64_t)a.has_mass + (int64_t)s * a.F;
    if constexpr (VEC) {
      for (int f = 0; f < a.F; f += 4) {
        float4 acc = a.bias ? *reinterpret_cast<const float4*>(a.bias + c0 + f) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int t = 0; t < D; ++t) {
          const float4 cf = *reinterpret_cast<ConstAS<float4>*>(tab + (int64_t)t * a.ldt + f);
          acc.x = fmaf(cf.x, net.k[t], acc.x);
          acc.y = fmaf(cf.y, net.k[t], acc.y);
          acc.z = fmaf(cf.z, net.k[t], acc.z);
          acc.w = fmaf(cf.w, net.k[t], acc.w);
        }
        *reinterpret_cast<float4*>(orow + c0 + f) =
            make_float4(a.out_scale * acc.x, a.out_scale * acc.y, a.out_scale * acc.z, a.out_scale * acc.w);
      }
    } else for (int f = 0; f < a.F; ++f) {
      float acc = a.bias ? a.bias[c0 + f] : 0.f;
#pragma unroll
      for (int t = 0; t < D; ++t) acc = fmaf(tab[(int64_t)t * a.ldt + f], net.k[t], acc);   // wave-uniform coefficient
      orow[c0 + f] = a.out_scale * acc;
    }
    if (a.has_mass && s == 0) orow[0] = mass_column((float)D, a.mass_fn, a.mass_scale, a.bias, a.out_scale);
  }
}

template <int D>
__device__ __forceinline__ void cart_reg_weighted(const CartTuned& a, int p, int pe) {
  const int items = (pe - p) * a.S;
  const double tau = (double)a.tau;
  for (int i = threadIdx.x; i < items; i += blockDim.x) {
    const int r = i / a.S, s = i - r * a.S;
    const int node = a.perm[p + r];
    const int start = a.rowptr[node];
    PairNet<D + 1> net;
    double m = 0.0;
#pragma unroll
    for (int t = 0; t < D; ++t) {
      const float wt = a.w ? a.w[start + t] : 1.f;
      net.k[t] = a.Xp[(int64_t)a.col[start + t] * a.ldp + s];
      net.w[t] = wt;
      m += (double)wt;
    }
    net.k[D] = 0.f;                                   // the reference's pad element at x = 0
    net.w[D] = (float)fmax(tau - m, 0.0);
    const double rho = pad_residual(tau - m, net.w[D]);   // what the float lane lost of the pad weight (fsw_common.h)
    const double inv = 1.0 / fmax(m, tau);
    sort_network<D + 1>(net);
    double cn[D + 1];
    double cum = 0.0;
#pragma unroll
    for (int t = 0; t <= D; ++t) {
      cum += (double)net.w[t];
      cn[t] = (cum + pad_residual_at(rho, net.k[t])) * inv;
    }
    float* orow = a.out + (int64_t)node * a.ldo;
    const int64_t c0 = (int64_t)a.has_mass + (int64_t)s * a.F;
    for (int f = 0; f < a.F; ++f) {
      const float xif = as_const(a.freqs)[f];
      const double xi = (double)xif;
      float val;
      if (fabsf(xif) < 1e-30f) {                             // xi == 0: Delta_t = 2 w_t
        float acc0 = 0.f;
#pragma unroll
        for (int t = 0; t <= D; ++t) acc0 = fmaf(net.w[t], net.k[t], acc0);
        val = 2.f * acc0 * (float)inv;
      } else {
        float acc = 0.f, sprev = 0.f;
#pragma unroll
        for (int t = 0; t <= D; ++t) {
          const float sn = sin2pi_rev(xi * cn[t]);
          acc = fmaf(sn - sprev, net.k[t], acc);
          sprev = sn;
        }
        val = (float)((1.0 + xi) / (kPi * xi)) * acc;
      }
      orow[c0 + f] = a.out_scale * (val + (a.bias ? a.bias[c0 + f] : 0.f));
    }
    if (a.has_mass && s == 0)
      orow[0] = mass_column((float)m, a.mass_fn, a.mass_scale, a.bias, a.out_scale);
  }
}

template <bool UNIT, bool VEC>
__global__ void __launch_bounds__(256) k_cart_reg(const CartTuned a) {
  int D, p, pe;
  if (!find_degree_tile<kCartRows>(a.bin_start, 1, FSW_REG_MAX_DEG, (int)blockIdx.x, D, p, pe)) return;
  switch (D) {
#define X(d)                                       \
  case d:                                          \
    if constexpr (UNIT) cart_reg_unit<d, VEC>(a, p, pe); \
    else cart_reg_weighted<d>(a, p, pe);           \
    break;
    FSW_CASES_1_32(X)
#undef X
    default:
      break;
  }
}

// One wavefront per (row, slice) for lines of up to 64 M elements; rows perm[p0 + blockIdx.x], slice blockIdx.y.
template <int M, bool WEIGHTED>
__global__ void __launch_bounds__(64) k_cart_wave(const CartTuned a, int p0) {
  constexpr int LMAX = 64 * M;
  __shared__ float lk[LMAX];
  __shared__ double lc[WEIGHTED ? LMAX : 1];
  __shared__ float red[kWave];
  const int lane = threadIdx.x;
  const int node = a.perm[p0 + blockIdx.x];
  const int s = blockIdx.y;
  const int start = a.rowptr[node];
  const int D = a.rowptr[node + 1] - start;
  const int L = WEIGHTED ? D + 1 : D;              // unit weights with tau <= 1: the pad element has weight 0 and is left out
  if (L > LMAX || L <= 0) return;                  // longer lines: the generic kernel (block-uniform exit, before any barrier)
  WaveLine<M, WEIGHTED> ln;
  double mpart = 0.0;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const int e = lane * M + j;
    float key = __builtin_inff(), wt = 0.f;
    if (e < D) {
      key = a.Xp[(int64_t)a.col[start + e] * a.ldp + s];
      wt = a.w ? a.w[start + e] : 1.f;
    }
    ln.k[j] = key;
    if constexpr (WEIGHTED) ln.w[j] = wt;
    mpart += (double)wt;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mpart += __shfl_xor(mpart, off);
  const double m = mpart;
  const double tau = (double)a.tau;
  const double inv = 1.0 / fmax(m, tau);
  const float padw = (float)fmax(tau - m, 0.0);
  const double rho = pad_residual(tau - m, padw);    // what the float line loses of the pad weight (fsw_common.h)
  if constexpr (WEIGHTED) {
#pragma unroll
    for (int j = 0; j < M; ++j)
      if (lane * M + j == D) {
        ln.k[j] = 0.f;
        ln.w[j] = padw;
      }
  }
  ln.sort();
  double pre = 0.0;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    lk[lane * M + j] = ln.k[j];
    if constexpr (WEIGHTED) pre += (double)ln.w[j];
  }
  if constexpr (WEIGHTED) {
    double inc = pre;                                // exclusive scan of the lanes' weight totals
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const double t = __shfl_up(inc, off);
      if (lane >= off) inc += t;
    }
    double c = inc - pre;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      c += (double)ln.w[j];
      lc[lane * M + j] = (c + pad_residual_at(rho, ln.k[j])) * inv;   // telescoped readout: a zero key's term has dp == 0 unless the pad lies before it
    }
  }
  __syncthreads();
  float* orow = a.out + (int64_t)node * a.ldo;
  const int64_t c0 = (int64_t)a.has_mass + (int64_t)s * a.F;
  const double invD = 1.0 / (double)D;
  for (int f0 = 0; f0 < a.F; f0 += kWave) {
    const int NF = min(kWave, a.F - f0);
    const int Q = kWave / NF;
    const int f = f0 + lane % NF, q = lane / NF;
    const double xi = (double)a.freqs[f];
    const bool lin = fabs(xi) < 1e-30;
    float acc = 0.f;
    if (q < Q) {
      for (int t = q; t < L; t += Q) {
        const double c = WEIGHTED ? lc[t] : (double)(t + 1) * invD;
        const float dp = lk[t] - (t + 1 < L ? lk[t + 1] : 0.f);
        const float term = lin ? (float)(2.0 * c) : sin2pi_rev(xi * c);
        acc = fmaf(term, dp, acc);
      }
    }
    red[lane] = acc;
    __syncthreads();
    if (lane < NF) {
      float sum = 0.f;
      for (int u = 0; u < Q; ++u) sum += red[lane + u * NF];
      const float val = lin ? sum : (float)((1.0 + xi) / (kPi * xi)) * sum;
      orow[c0 + f] = a.out_scale * (val + (a.bias ? a.bias[c0 + f] : 0.f));
    }
    __syncthreads();
  }
  if (a.has_mass && s == 0 && lane == 0)
    orow[0] = mass_column((float)m, a.mass_fn, a.mass_scale, a.bias, a.out_scale);
}

template <int M>
int launch_cart_wave(const CartTuned& t, bool weighted, int p0, int rows, int S, hipStream_t stream) {
  if (rows <= 0) return 0;
  dim3 grid((unsigned)rows, (unsigned)S);
  if (weighted) k_cart_wave<M, true><<<grid, kWave, 0, stream>>>(t, p0);
  else k_cart_wave<M, false><<<grid, kWave, 0, stream>>>(t, p0);
  FSW_LAUNCH_CHECK();
  return 0;
}

}  // namespace

int cart_check_common(const fsw_cart_args* c) {
  FSW_REQUIRE(c, "fsw_embed_cart: null args");
  FSW_REQUIRE(c->rowptr && c->Xp && c->freqs && (c->num_rows == 0 || c->col || c->max_degree == 0), "fsw_embed_cart: null pointer");
  FSW_REQUIRE(c->num_rows >= 0 && c->S >= 1 && c->F >= 1 && c->ldp >= c->S && c->max_degree >= 0 && c->tau > 0.0,
              "fsw_embed_cart: bad sizes");
  FSW_REQUIRE(c->S <= 65535 && (int64_t)c->S * c->F < (1ll << 31), "fsw_embed_cart: S <= 65535 and S * F < 2^31 required");
  FSW_REQUIRE(c->has_mass == 0 || c->has_mass == 1, "fsw_embed_cart: has_mass must be 0 or 1");
  FSW_REQUIRE(c->mass_fn >= 0 && c->mass_fn <= 2, "fsw_embed_cart: mass_fn must be 0, 1 or 2");
  return 0;
}

}  // namespace fsw

using namespace fsw;

// the backward's scratch for a longest row of max_degree neighbours and long_rows rows from the first class on
static size_t cart_backward_scratch_bytes(const CartLongMode& m, int64_t max_degree, int64_t long_rows, int32_t S) {
  if (max_degree <= m.cls[0].dlo) return 0;
  const int64_t rows = std::max<int64_t>(long_rows, 1);
  size_t bytes = cart_line_buffer_bytes(cart_line_elems(m, std::min<int64_t>(max_degree, m.last().dhi)), rows * std::max<int32_t>(S, 1));
  // the rows beyond the classes run on the generic kernel out of the same buffer
  if (max_degree >= m.generic_min_degree) bytes = std::max(bytes, fsw_embed_cart_generic_scratch_bytes(max_degree, rows));
  return bytes;
}

extern "C" size_t fsw_embed_cart_scratch_bytes(const fsw_cart_args* c, int backward) {
  if (!c || !c->bin_start_host) return 0;
  const CartLongMode& m = cart_long_mode(cart_unit_fast(c));
  const int32_t* bs = c->bin_start_host;
  // forward: only the rows that run on the generic kernel need scratch
  const int64_t generic_rows = (int64_t)bs[FSW_NUM_BINS] - bs[m.generic_bin];
  const size_t forward = c->max_degree < m.generic_min_degree
                             ? 0 : fsw_embed_cart_generic_scratch_bytes(c->max_degree, std::max<int64_t>(generic_rows, 1));
  if (!backward) return forward;
  // unit weights without a row in the class bins: the backward runs the same kernels as the forward, out of the forward's buffer
  if (m.pad == 0 && bs[m.last().bin_hi + 1] == bs[m.cls[0].bin_lo]) return forward;
  return cart_backward_scratch_bytes(m, c->max_degree, (int64_t)bs[FSW_NUM_BINS] - bs[m.cls[0].bin_lo], c->S);
}

// forward of the tuned entry point: one scratch line per workgroup the launcher of the giant class would use, at most 2 GiB, at least one
extern "C" size_t fsw_embed_cart_forward_scratch_bytes(const fsw_cart_args* c) {
  if (!c || !c->bin_start_host) return 0;
  const CartLongMode& m = cart_long_mode(cart_unit_fast(c));
  const int64_t rows = cart_giant_rows(c, m);
  if (rows <= 0) return 0;
  const size_t line_bytes = cart_giant_line_bytes(m, c->max_degree);
  const size_t cap = (size_t)2 << 30;                            // as cart_line_buffer_bytes
  const size_t lines = std::min<size_t>((size_t)cart_giant_workgroups(m, INT64_MAX, rows * std::max<int32_t>(c->S, 1)), cap / line_bytes);
  return std::max<size_t>(lines, 1) * line_bytes;
}

// the split form of the longest unit-weight rows (embed_split_cart.hip, embed_cart.h: cart_split_plan): host values only
extern "C" size_t fsw_embed_cart_split_scratch_bytes(const fsw_cart_args* c) { return cart_split_plan(c).bytes; }
extern "C" int64_t fsw_embed_cart_split_lines(const fsw_cart_args* c) { return cart_split_plan(c).lines; }
extern "C" int64_t fsw_embed_cart_split_max_lines(void) { return kCartSplitMaxLines; }

// the split form of the longest general-weight rows (embed_split_cart_w.hip, embed_cart.h: cart_split_w_plan): host values only
extern "C" size_t fsw_embed_cart_split_w_scratch_bytes(const fsw_cart_args* c) { return cart_split_w_plan(c).bytes; }
extern "C" int64_t fsw_embed_cart_split_w_lines(const fsw_cart_args* c) { return cart_split_w_plan(c).lines; }
extern "C" int64_t fsw_embed_cart_split_w_max_lines(void) { return kCartSplitWMaxLines; }

// backward of the tuned entry point: the larger of what the launches of the classes with a scratch line per wavefront need and of one
// scratch line per workgroup the launcher of the giant class would use (at most 2 GiB, at least one line)
extern "C" size_t fsw_embed_cart_backward_keys_scratch_bytes(const fsw_cart_args* c) {
  if (!c || !c->bin_start_host) return 0;
  const CartLongMode& m = cart_long_mode(cart_unit_fast(c));
  const int32_t S = std::max<int32_t>(c->S, 1);
  size_t bytes = cart_line_classes_bwd_bytes(c, m);
  const int64_t rows = cart_giant_rows(c, m);
  if (rows > 0) {
    const size_t line_bytes = cart_giant_bwd_line_bytes(m, c->max_degree);
    const size_t cap = (size_t)2 << 30;                          // as cart_line_buffer_bytes
    const size_t lines = std::min<size_t>((size_t)cart_giant_bwd_workgroups(m, INT64_MAX, rows * S), cap / line_bytes);
    bytes = std::max(bytes, std::max<size_t>(lines, 1) * line_bytes);
  }
  return bytes;
}

// the split form of the longest unit-weight rows' backward (embed_split_cart_bwd.hip, embed_cart.h: cart_split_bwd_plan): host values only
extern "C" size_t fsw_embed_cart_split_backward_scratch_bytes(const fsw_cart_args* c) { return cart_split_bwd_plan(c).bytes; }
extern "C" int64_t fsw_embed_cart_split_backward_lines(const fsw_cart_args* c) { return cart_split_bwd_plan(c).lines; }
extern "C" int64_t fsw_embed_cart_split_backward_max_lines(void) { return kCartSplitBwdMaxLines; }

extern "C" size_t fsw_embed_cart_backward_scratch_bytes(int64_t max_degree, int64_t long_rows, int32_t S) {
  return cart_backward_scratch_bytes(kCartLong[0], max_degree, long_rows, S);
}

extern "C" size_t fsw_embed_cart_weighted_backward_scratch_bytes(int64_t max_degree, int64_t long_rows, int32_t S) {
  return cart_backward_scratch_bytes(kCartLong[1], max_degree, long_rows, S);
}

extern "C" int fsw_embed_cart_generic(const fsw_cart_args* c, fsw_stream_t stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  int rc;
  if ((rc = cart_check_common(c))) return rc;
  FSW_REQUIRE(c->value_dtype == 0 || c->value_dtype == 1, "fsw_embed_cart_generic: value_dtype must be 0 (float32) or 1 (float64)");
  const int64_t width = (int64_t)c->has_mass + (int64_t)c->S * c->F;
  if (c->g) {
    FSW_REQUIRE(c->ldg >= width && (!c->gkey || c->ldk >= c->S), "fsw_embed_cart_generic: bad gradient strides");
  } else {
    FSW_REQUIRE(c->out && c->ldo >= width, "fsw_embed_cart_generic: bad output");
  }
  if (c->num_rows == 0) return 0;
  return launch_embed_generic(generic_args(*c, true, c->F), c->value_dtype, nullptr, c->num_rows, 0, stream);
}

extern "C" int fsw_embed_cart_f32(const fsw_cart_args* c, fsw_stream_t stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  int rc;
  if ((rc = cart_check_common(c))) return rc;
  FSW_REQUIRE(c->value_dtype == 0 && !c->g, "fsw_embed_cart_f32: float32 forward only (fsw_embed_cart_generic for the rest)");
  FSW_REQUIRE(c->perm && c->bin_start && c->bin_start_host, "fsw_embed_cart_f32: needs perm, bin_start and its host copy");
  FSW_REQUIRE(c->out && c->ldo >= (int64_t)c->has_mass + (int64_t)c->S * c->F, "fsw_embed_cart_f32: bad output");
  const bool unit_fast = cart_unit_fast(c);
  FSW_REQUIRE(!unit_fast || (c->unit_table && c->ldt >= c->F), "fsw_embed_cart_f32: unit weights with tau <= 1 need unit_table");
  if (c->num_rows == 0) return 0;
  const int32_t* bs = c->bin_start_host;
  // FSW_CART_SPLIT_LINES: the giant class in the split form where one exists (lines > 0), refused before any launch when the buffer is short
  const CartSplitPlan split = (c->flags & FSW_CART_SPLIT_LINES) ? cart_split_plan(c) : CartSplitPlan{};
  if (split.lines > 0) {
    FSW_REQUIRE(c->scratch && ((uintptr_t)c->scratch & 15) == 0 && c->scratch_bytes >= split.bytes,
                "fsw_embed_cart_f32: FSW_CART_SPLIT_LINES needs a 16-byte aligned scratch buffer of fsw_embed_cart_split_scratch_bytes(args) bytes");
  }
  // FSW_CART_SPLIT_W_LINES: the same for general weights (a call has one of the two forms at most: unit weights or not)
  const CartSplitWPlan split_w = (c->flags & FSW_CART_SPLIT_W_LINES) ? cart_split_w_plan(c) : CartSplitWPlan{};
  if (split_w.lines > 0) {
    FSW_REQUIRE(c->scratch && ((uintptr_t)c->scratch & 15) == 0 && c->scratch_bytes >= split_w.bytes,
                "fsw_embed_cart_f32: FSW_CART_SPLIT_W_LINES needs a 16-byte aligned scratch buffer of fsw_embed_cart_split_w_scratch_bytes(args) bytes");
  }

  CartTuned t;
  cart_fill_inputs_w(t, c);
  cart_fill_outputs(t, c);
  t.table = c->unit_table; t.ldt = c->ldt;

  // rows of in-degree 0: the embedding of the pad element alone is 0 -> out_scale * bias (mass column: f(0) = 0)
  if (bs[1] > bs[0]) {
    fsw_embed_args z = {};
    z.perm = c->perm; z.bin_start = c->bin_start; z.S = c->S * c->F; z.out = (float*)c->out; z.ldo = c->ldo;
    z.bias = (const float*)c->bias; z.out_scale = (float)c->out_scale; z.has_mass = c->has_mass;
    if ((rc = launch_zero_rows(z, stream))) return rc;
  }
  // 1 <= D <= 32: one lane per (row, slice); grid = the exact number of tiles of every degree bin
  int64_t tiles = 0;
  for (int d = 1; d <= FSW_REG_MAX_DEG; ++d) tiles += ceil_div(bs[d + 1] - bs[d], kCartRows);
  if (tiles > 0) {
    // 16-byte stores and bias loads start at column has_mass of a row: what has to be aligned is that address, not the row's
    const bool vec = c->F % 4 == 0 && c->ldt % 4 == 0 && c->ldo % 4 == 0 && (uintptr_t)((const float*)c->out + c->has_mass) % 16 == 0 &&
                     (uintptr_t)c->unit_table % 16 == 0 && (!c->bias || (uintptr_t)((const float*)c->bias + c->has_mass) % 16 == 0);
    if (unit_fast && vec) k_cart_reg<true, true><<<(unsigned)tiles, 256, 0, stream>>>(t);
    else if (unit_fast) k_cart_reg<true, false><<<(unsigned)tiles, 256, 0, stream>>>(t);
    else k_cart_reg<false, false><<<(unsigned)tiles, 256, 0, stream>>>(t);
    FSW_LAUNCH_CHECK();
  }
  // 33 <= line <= 2048: one wavefront per (row, slice); consecutive bins that need the same keys per lane share a launch
  const int extra = unit_fast ? 0 : 1;
  rc = for_each_wave_group(bs, extra, [&](int Mb, int p0, int rows) {
    switch (Mb) {
      case 1: return launch_cart_wave<1>(t, !unit_fast, p0, rows, c->S, stream);
      case 2: return launch_cart_wave<2>(t, !unit_fast, p0, rows, c->S, stream);
      case 4: return launch_cart_wave<4>(t, !unit_fast, p0, rows, c->S, stream);
      case 8: return launch_cart_wave<8>(t, !unit_fast, p0, rows, c->S, stream);
      case 16: return launch_cart_wave<16>(t, !unit_fast, p0, rows, c->S, stream);
      default: return launch_cart_wave<32>(t, !unit_fast, p0, rows, c->S, stream);
    }
  });
  if (rc) return rc;
  // lines above kCartMaxLine elements (the classes of embed_cart.h: kCartLong): one workgroup of 2 .. 16 wavefronts per line
  if ((rc = unit_fast ? launch_cart_hub(c, stream) : launch_cart_hub_w(c, stream))) return rc;
  // the giant class (any length): sorted blocks in the scratch lines of c->scratch, one workgroup per line -- or, unit weights with
  // FSW_CART_SPLIT_LINES (general weights: FSW_CART_SPLIT_W_LINES), every line split over the workgroups of a launch per phase
  if (split.lines > 0) return launch_cart_split(c, split, stream);
  if (split_w.lines > 0) return launch_cart_split_w(c, split_w, stream);
  return unit_fast ? launch_cart_giant(c, stream) : launch_cart_giant_w(c, stream);
}
