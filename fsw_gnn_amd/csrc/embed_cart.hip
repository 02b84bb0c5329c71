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
//   longer lines     the generic kernel below (correct, not tuned: DESIGN.md).
// Readout, by summation by parts of the reference's Delta_t = 2 w_t sinc(xi w_t) cos(pi xi (2 c_t - w_t)):
//   out = (1 + xi) / (pi xi) sum_t sin(2 pi xi c_t) (p_(t) - p_(t+1)),  p_(L) = 0;   xi = 0:  out = sum_t 2 c_t (p_(t) - p_(t+1)).
//
// The generic kernel (fsw_embed_cart_generic) restates k_embed_generic of embed_generic.hip for the Cartesian product: any degree,
// float32 or float64 storage, float64 arithmetic, forward and backward.  Backward, for the output gradient g:
//   gkey[e, s] = sum_f out_scale g[r, s F + f] (1 + xi_f) Delta_t(xi_f)                       (stored)
//   gfreq[f]  += sum_{r, s} out_scale g[r, s F + f] d out[r, s F + f] / d xi_f                (accumulated)
//   gw[e]     += sum_{s, f} out_scale g[r, s F + f] d out[r, s F + f] / d w_e                 (accumulated; mass column excluded)
// with the per-frequency terms of embed_generic.hip:17-20 summed over f (the weight gradient is linear in H_t, so H is summed
// over the frequencies first and the reverse cumulative sum runs once per slice).
#include <algorithm>
#include "embed_cart.h"
#include "embed_launch.h"
#include "sortnet.h"
#include "wave_sort.h"

namespace fsw {

namespace {

constexpr int kCgThreads = 256;
constexpr int kCgLdsElems = 2048;
constexpr int kCartScratchBytesPerElem = 8 + 4 + 8 + 8 + 8;   // key, index, cumulative weight, H / reverse sum, key gradient

template <class T>
struct CartGen {
  const int32_t* rowptr;
  const int32_t* col;
  const T* w;
  const int32_t* rows;   // null: rows 0 .. num_rows - 1; else rows[0 .. num_rows - 1] (the tuned entry's long rows)
  int64_t num_rows;
  int min_deg;           // rows of fewer neighbours are skipped (belong to another kernel)
  const T* Xp;
  int64_t ldp;
  const T* freqs;
  int S, F;
  double tau;
  T* out;
  int64_t ldo;
  const T* bias;
  double out_scale;
  int has_mass, mass_fn;
  double mass_scale;
  const T* g;
  int64_t ldg;
  T* gkey;
  int64_t ldk;
  T* gfreq;
  T* gw;
  char* scratch;
  int64_t line_elems;
};

__device__ __forceinline__ double sinc_c(double z) { return z == 0.0 ? 1.0 : sinpi(z) / (kPi * z); }
__device__ __forceinline__ double dsinc_c(double z) { return z == 0.0 ? 0.0 : (cospi(z) - sinc_c(z)) / z; }

__device__ __forceinline__ double cg_block_sum(double v, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if (lane_id() == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ double cg_block_scan(double v, double* red, double* total) {
  double inc = v;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const double t = __shfl_up(inc, off);
    if (lane_id() >= off) inc += t;
  }
  __syncthreads();
  if (lane_id() == kWave - 1) red[threadIdx.x >> 6] = inc;
  __syncthreads();
  double base = 0.0, tot = 0.0;
#pragma unroll
  for (int i = 0; i < kCgThreads / kWave; ++i) {
    if (i < (int)(threadIdx.x >> 6)) base += red[i];
    tot += red[i];
  }
  *total = tot;
  return base + inc;
}

// ---- generic kernel: one workgroup per row, slices in turn, frequencies per sorted slice -------------------------------------
template <class T>
__global__ void __launch_bounds__(kCgThreads) k_embed_cart_generic(const CartGen<T> a) {
  __shared__ double lkey[kCgLdsElems];
  __shared__ int lidx[kCgLdsElems];
  __shared__ double red[4];
  char* myscr = a.scratch + (int64_t)blockIdx.x * a.line_elems * kCartScratchBytesPerElem;
  double* gkeyb = reinterpret_cast<double*>(myscr);
  double* cw = gkeyb + a.line_elems;
  double* hr = cw + a.line_elems;
  double* gks = hr + a.line_elems;
  int* gidx = reinterpret_cast<int*>(gks + a.line_elems);
  const bool backward = a.g != nullptr;
  const int tid = threadIdx.x;
  for (int64_t i = blockIdx.x; i < a.num_rows; i += gridDim.x) {
    const int64_t row = a.rows ? (int64_t)a.rows[i] : i;
    const int start = a.rowptr[row];
    const int D = a.rowptr[row + 1] - start;
    if (D < a.min_deg) continue;                                           // workgroup-uniform
    const int Dtot = D + 1;
    int Dp = 1;
    while (Dp < Dtot) Dp <<= 1;
    const bool in_lds = Dp <= kCgLdsElems;
    double* keys = in_lds ? lkey : gkeyb;
    int* idx = in_lds ? lidx : gidx;
    double part = 0.0;
    for (int t = tid; t < D; t += kCgThreads) part += a.w ? (double)a.w[start + t] : 1.0;
    const double m = cg_block_sum(part, red);
    const double M = fmax(m, a.tau);
    const double padw = fmax(a.tau - m, 0.0);
    const double invM = 1.0 / M;
    auto raw_weight = [&](int e) -> double { return e < D ? (a.w ? (double)a.w[start + e] : 1.0) : (e == D ? padw : 0.0); };
    if (!backward && a.has_mass && tid == 0)
      a.out[row * a.ldo] = (T)mass_column(m, a.mass_fn, a.mass_scale, a.bias, a.out_scale);
    for (int s = 0; s < a.S; ++s) {
      for (int t = tid; t < Dp; t += kCgThreads) {
        double key = __builtin_inf();
        if (t < D) key = (double)a.Xp[(int64_t)a.col[start + t] * a.ldp + s];
        else if (t == D) key = 0.0;
        keys[t] = key;
        idx[t] = t;
      }
      __syncthreads();
      for (int size = 2; size <= Dp; size <<= 1) {
        for (int st = size >> 1; st >= 1; st >>= 1) {
          for (int j = tid; j < Dp; j += kCgThreads) {
            const int k = j ^ st;
            if (k > j) {
              const double kj = keys[j], kk = keys[k];
              const int ij = idx[j], ik = idx[k];
              const bool up = (j & size) == 0;
              const bool gt = kj > kk || (kj == kk && ij > ik);
              if (gt == up) {
                keys[j] = kk;
                keys[k] = kj;
                idx[j] = ik;
                idx[k] = ij;
              }
            }
          }
          __syncthreads();
        }
      }
      double run = 0.0;
      for (int b0 = 0; b0 < Dtot; b0 += kCgThreads) {
        const int t = b0 + tid;
        const double wv = t < Dtot ? raw_weight(idx[t]) * invM : 0.0;
        double tot;
        const double inc = cg_block_scan(wv, red, &tot);
        if (t < Dtot) cw[t] = run + inc;
        run += tot;
      }
      __syncthreads();
      if (backward)
        for (int t = tid; t < Dtot; t += kCgThreads) { gks[t] = 0.0; hr[t] = 0.0; }   // each t is owned by one thread below
      for (int f = 0; f < a.F; ++f) {
        const double xi = (double)a.freqs[f];
        const int64_t oc = (int64_t)a.has_mass + (int64_t)s * a.F + f;
        const double gk = backward ? a.out_scale * (double)a.g[row * a.ldg + oc] : 0.0;
        if (backward && gk == 0.0) continue;                                           // workgroup-uniform
        double acc = 0.0, dacc = 0.0;
        for (int t = tid; t < Dtot; t += kCgThreads) {
          const double wv = raw_weight(idx[t]) * invM;
          const double c = cw[t];
          const double B = xi * (2.0 * c - wv);
          const double sc = sinc_c(xi * wv);
          const double cb = cospi(B);
          const double delta = 2.0 * wv * sc * cb;
          const double key = keys[t];
          acc += delta * key;
          if (backward) {
            const double ddelta = 2.0 * wv * (wv * dsinc_c(xi * wv) * cb - sc * kPi * (2.0 * c - wv) * sinpi(B));
            dacc += (delta + (1.0 + xi) * ddelta) * key;
            gks[t] += gk * (1.0 + xi) * delta;
            if (a.gw) {
              const double knext = t + 1 < Dtot ? keys[t + 1] : 0.0;
              hr[t] += gk * 2.0 * (1.0 + xi) * cospi(2.0 * xi * c) * (key - knext);
            }
          }
        }
        if (!backward) {
          const double val = cg_block_sum(acc, red);
          if (tid == 0) a.out[row * a.ldo + oc] = (T)(a.out_scale * ((1.0 + xi) * val + (a.bias ? (double)a.bias[oc] : 0.0)));
        } else if (a.gfreq) {
          const double dv = cg_block_sum(dacc, red);
          if (tid == 0) atomic_add_t(&a.gfreq[f], gk * dv);
        }
      }
      if (backward) {
        if (a.gkey)
          for (int t = tid; t < Dtot; t += kCgThreads) {
            const int e = idx[t];
            if (e < D) a.gkey[(int64_t)(start + e) * a.ldk + s] = (T)gks[t];
          }
        if (a.gw) {
          __syncthreads();
          double hc = 0.0;
          for (int t = tid; t < Dtot; t += kCgThreads) hc += hr[t] * cw[t];
          const double HC = cg_block_sum(hc, red);
          double runr = 0.0;
          const int nchunk = (Dtot + kCgThreads - 1) / kCgThreads;
          for (int cix = nchunk - 1; cix >= 0; --cix) {
            const int t = cix * kCgThreads + (kCgThreads - 1 - tid);
            const double hv = t < Dtot ? hr[t] : 0.0;
            double tot;
            const double inc = cg_block_scan(hv, red, &tot);
            __syncthreads();
            if (t < Dtot) hr[t] = runr + inc;
            runr += tot;
          }
          __syncthreads();
          double rp = 0.0;
          for (int t = tid; t < Dtot; t += kCgThreads)
            if (idx[t] == D) rp = hr[t];
          const double Rpad = cg_block_sum(rp, red);
          const double corr = (m <= a.tau ? Rpad : 0.0) + (m >= a.tau ? HC : 0.0);
          for (int t = tid; t < Dtot; t += kCgThreads) {
            const int e = idx[t];
            const double v = (hr[t] - corr) * invM;
            if (e < D && v != 0.0) atomic_add_t(&a.gw[start + e], v);
          }
        }
      }
      __syncthreads();
    }
  }
}

int64_t cart_line_elems(int64_t max_degree) {
  int64_t line = 1;
  while (line < max_degree + 1) line <<= 1;
  return line;
}

template <class T>
int run_cart_generic(const fsw_cart_args* c, const int32_t* rows, int64_t num_rows, int min_deg, hipStream_t stream) {
  CartGen<T> a;
  a.rowptr = c->rowptr; a.col = c->col; a.w = (const T*)c->w; a.rows = rows; a.num_rows = num_rows; a.min_deg = min_deg;
  a.Xp = (const T*)c->Xp; a.ldp = c->ldp; a.freqs = (const T*)c->freqs; a.S = c->S; a.F = c->F; a.tau = c->tau;
  a.out = (T*)c->out; a.ldo = c->ldo; a.bias = (const T*)c->bias; a.out_scale = c->out_scale;
  a.has_mass = c->has_mass; a.mass_fn = c->mass_fn; a.mass_scale = c->mass_scale;
  a.g = (const T*)c->g; a.ldg = c->ldg; a.gkey = (T*)c->gkey; a.ldk = c->ldk; a.gfreq = (T*)c->gfreq; a.gw = (T*)c->gw;
  a.line_elems = cart_line_elems(c->max_degree);
  a.scratch = (char*)c->scratch;
  const int64_t per_wg = a.line_elems * kCartScratchBytesPerElem;
  int64_t nwg = std::min<int64_t>(num_rows, 2048);
  nwg = std::min<int64_t>(nwg, (int64_t)(c->scratch_bytes / (size_t)per_wg));
  FSW_REQUIRE(c->scratch && nwg >= 1, "fsw_embed_cart: scratch buffer too small (need fsw_embed_cart_generic_scratch_bytes)");
  k_embed_cart_generic<T><<<(unsigned)nwg, kCgThreads, 0, stream>>>(a);
  FSW_LAUNCH_CHECK();
  return 0;
}

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

// VEC: four frequencies per step -- 16-byte coefficient loads (wave-uniform) and 16-byte output stores (F % 4 == 0, no mass column
// in front of the run, 16-byte aligned rows: launch condition on the host)
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
    const double inv = 1.0 / fmax(m, tau);
    sort_network<D + 1>(net);
    double cn[D + 1];
    double cum = 0.0;
#pragma unroll
    for (int t = 0; t <= D; ++t) {
      cum += (double)net.w[t];
      cn[t] = cum * inv;
    }
    float* orow = a.out + (int64_t)node * a.ldo;
    const int64_t c0 = (int64_t)a.has_mass + (int64_t)s * a.F;
    for (int f = 0; f < a.F; ++f) {
      const float xif = as_const(a.freqs)[f];
      const double xi = (double)xif;
      float val;
      if (xif < 1e-30f) {                             // xi == 0: Delta_t = 2 w_t
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
    FSW_CART_CASES_1_32(X)
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
  if constexpr (WEIGHTED) {
#pragma unroll
    for (int j = 0; j < M; ++j)
      if (lane * M + j == D) {
        ln.k[j] = 0.f;
        ln.w[j] = (float)fmax(tau - m, 0.0);
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
      lc[lane * M + j] = c * inv;
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
    const bool lin = xi < 1e-30;
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

int bin_upper_degree(int b) {
  constexpr int sizes[FSW_NUM_MID_BINS] = FSW_MID_SIZES;
  if (b <= FSW_REG_MAX_DEG) return b;
  if (b < FSW_BIN_LDS0) return sizes[b - FSW_BIN_MID0];
  if (b < FSW_BIN_HUB0) return 512 << (b - FSW_BIN_LDS0);
  return 1 << 30;
}

int launch_cart_generic_f32(const fsw_cart_args* c, const int32_t* rows, int64_t num_rows, int min_deg, hipStream_t stream) {
  return run_cart_generic<float>(c, rows, num_rows, min_deg, stream);
}

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

extern "C" size_t fsw_embed_cart_generic_scratch_bytes(int64_t max_degree, int64_t num_rows) {
  const size_t per_wg = (size_t)cart_line_elems(max_degree) * kCartScratchBytesPerElem;
  const size_t cap = (size_t)1 << 30;
  size_t nwg = (size_t)std::max<int64_t>(1, std::min<int64_t>(num_rows, 2048));
  nwg = std::max<size_t>(1, std::min<size_t>(nwg, cap / per_wg));
  return nwg * per_wg;
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
  return c->value_dtype == 0 ? run_cart_generic<float>(c, nullptr, c->num_rows, 0, stream)
                             : run_cart_generic<double>(c, nullptr, c->num_rows, 0, stream);
}

extern "C" int fsw_embed_cart_f32(const fsw_cart_args* c, fsw_stream_t stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  int rc;
  if ((rc = cart_check_common(c))) return rc;
  FSW_REQUIRE(c->value_dtype == 0 && !c->g, "fsw_embed_cart_f32: float32 forward only (fsw_embed_cart_generic for the rest)");
  FSW_REQUIRE(c->perm && c->bin_start && c->bin_start_host, "fsw_embed_cart_f32: needs perm, bin_start and its host copy");
  FSW_REQUIRE(c->out && c->ldo >= (int64_t)c->has_mass + (int64_t)c->S * c->F, "fsw_embed_cart_f32: bad output");
  const bool unit_fast = c->w == nullptr && c->tau <= 1.0;
  FSW_REQUIRE(!unit_fast || (c->unit_table && c->ldt >= c->F), "fsw_embed_cart_f32: unit weights with tau <= 1 need unit_table");
  if (c->num_rows == 0) return 0;
  const int32_t* bs = c->bin_start_host;

  CartTuned t;
  t.rowptr = c->rowptr; t.col = c->col; t.w = (const float*)c->w; t.perm = c->perm; t.bin_start = c->bin_start;
  t.Xp = (const float*)c->Xp; t.ldp = c->ldp; t.freqs = (const float*)c->freqs; t.S = c->S; t.F = c->F; t.tau = (float)c->tau;
  t.table = c->unit_table; t.ldt = c->ldt; t.out = (float*)c->out; t.ldo = c->ldo; t.bias = (const float*)c->bias;
  t.out_scale = (float)c->out_scale; t.has_mass = c->has_mass; t.mass_fn = c->mass_fn; t.mass_scale = (float)c->mass_scale;

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
    const bool vec = c->F % 4 == 0 && c->ldt % 4 == 0 && c->has_mass == 0 && c->ldo % 4 == 0 && (uintptr_t)c->out % 16 == 0 &&
                     (uintptr_t)c->unit_table % 16 == 0 && (!c->bias || (uintptr_t)c->bias % 16 == 0);
    if (unit_fast && vec) k_cart_reg<true, true><<<(unsigned)tiles, 256, 0, stream>>>(t);
    else if (unit_fast) k_cart_reg<true, false><<<(unsigned)tiles, 256, 0, stream>>>(t);
    else k_cart_reg<false, false><<<(unsigned)tiles, 256, 0, stream>>>(t);
    FSW_LAUNCH_CHECK();
  }
  // 33 <= line <= 2048: one wavefront per (row, slice); consecutive bins that need the same keys per lane share a launch
  const int extra = unit_fast ? 0 : 1;
  int b = FSW_BIN_MID0;
  while (b < FSW_BIN_HUB0) {
    const int Mb = (int)std::min<uint32_t>(32, pow2ceil((uint32_t)ceil_div(bin_upper_degree(b) + extra, kWave)));
    int e = b;
    while (e + 1 < FSW_BIN_HUB0 &&
           (int)std::min<uint32_t>(32, pow2ceil((uint32_t)ceil_div(bin_upper_degree(e + 1) + extra, kWave))) == Mb)
      ++e;
    const int p0 = bs[b], rows = bs[e + 1] - bs[b];
    switch (Mb) {
      case 1: rc = launch_cart_wave<1>(t, !unit_fast, p0, rows, c->S, stream); break;
      case 2: rc = launch_cart_wave<2>(t, !unit_fast, p0, rows, c->S, stream); break;
      case 4: rc = launch_cart_wave<4>(t, !unit_fast, p0, rows, c->S, stream); break;
      case 8: rc = launch_cart_wave<8>(t, !unit_fast, p0, rows, c->S, stream); break;
      case 16: rc = launch_cart_wave<16>(t, !unit_fast, p0, rows, c->S, stream); break;
      default: rc = launch_cart_wave<32>(t, !unit_fast, p0, rows, c->S, stream); break;
    }
    if (rc) return rc;
    b = e + 1;
  }
  // longer lines (D > 2048; general weights: D + 1 > 2048): the generic kernel on the rows of the last LDS bin and above
  const int min_long = kCartMaxLine + 1 - extra;
  if (c->max_degree >= min_long) {
    const int p0 = bs[FSW_BIN_LDS0 + FSW_NUM_LDS_BINS - 1];
    const int64_t rows = (int64_t)bs[FSW_NUM_BINS] - p0;
    if (rows > 0 && (rc = run_cart_generic<float>(c, c->perm + p0, rows, min_long, stream))) return rc;
  }
  return 0;
}
