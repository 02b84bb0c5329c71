// The generic neighbourhood kernel, any in-degree, float32 or float64 storage: the float64 build of the path, the gradients with
// respect to the weights, and the long rows of tuned Cartesian mode.  gfx950.
//
// The tuned kernels (embed_reg / embed_mid / embed_hub / embed_wsort, embed_cart) are float32, specialised per degree class and
// treat the weights as constants.  This file states the same per-neighbourhood computation once, for every degree, both value
// types and both readouts, with all arithmetic in float64:
//   T = double   FSW_embedding / FSW_conv(dtype=torch.float64) (the reference's test_conv.py runs the layer in float64,
//                test_conv.py:24): forward and backward, pinned to the reference's float64 goldens at 1e-12;
//   T = float    d loss / d W for the float32 path (reference ag.div_sparse_dense.backward fsw_embedding.py:1656,
//                ag.cumsum_sparse.backward :2160 = reverse segmented cumsum, ag.permute_sparse.backward :1286).
// One workgroup per recipient row, looping over the slices.  Per (row, slice): (key, element index) pairs -- the reference's
// pad element x = 0 (fsw_embedding.py:787-821) is element D -- sorted by a bitonic network in LDS (up to 2048 elements) or in
// the workgroup's global scratch (any degree), ties by element index (the project's rule, DESIGN.md "equal keys"; the reference's order there is unspecified); cumulative weights by a
// workgroup scan (the segmented cumsum of fsw_embedding.py:1031-1032); readout
//   Delta_t = 2 w_t sinc(xi w_t) cos(pi xi (2 c_t - w_t))      (fsw_embedding.py:1047-1075, the product form: no cancellation)
//   out     = (1 + xi) sum_t Delta_t p_(t)                      (fsw_embedding.py:1084-1109).
// The sorted slice s is read out at
//   diagonal   (fsw_embed_generic)        xi = freqs[s] alone, into column has_mass + s;
//   Cartesian  (fsw_embed_cart_generic)   every xi = freqs[f], f < F, into column has_mass + s F + f (reference :1037-1045).
// Backward, with gk = out_scale g[row, column] per readout: d out / d p_(t) = (1 + xi) Delta_t, summed over the slice's readouts
// and stored per CSR entry (gkey), d out / d xi summed per frequency, and for the weights
//   d out / d c_t = 2 (1 + xi) cos(2 pi xi c_t) (p_(t) - p_(t+1)) = H_t,   c_t = A_t / M,  A_t = raw cumulative weight,  M = max(m, tau)
//   d out / d a_j = [ R(rank_j) - [m <= tau] R(rank_pad) - [m >= tau] sum_t H_t c_t ] / M,   R(r) = sum_{t >= r} H_t
// (a reverse cumulative sum over the sorted order; the two clamps pass gradients like the reference's custom_lowclamp, :1735-1744).
// The weight gradient is linear in H_t, so gk H_t is summed over the slice's readouts first and the reverse cumulative sum runs once
// per slice.  With one readout per slice this gives what multiplying by gk at the end gives: the forward, gkey (0 + x) and gfreq
// bit for bit, and gw up to float64 rounding (gk (R - corr) became the reverse sum of gk H_t minus its own corr).
#include <algorithm>
#include "embed_launch.h"

namespace fsw {

constexpr int kGenThreads = 256;
constexpr int kGenLdsElems = 2048;   // lines up to this many elements are sorted in LDS
constexpr int kGenMaxWorkgroups = 2048;

__device__ __forceinline__ double sinc_g(double z) { return z == 0.0 ? 1.0 : sinpi(z) / (kPi * z); }
__device__ __forceinline__ double dsinc_g(double z) { return z == 0.0 ? 0.0 : (cospi(z) - sinc_g(z)) / z; }   // reference sp.dsinc :2760-2774

// workgroup-wide sum of a double (all threads get the result)
__device__ __forceinline__ double block_sum(double v, double* red /* LDS [4] */) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if (lane_id() == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// inclusive scan of one double per thread over the workgroup; returns this thread's inclusive value, *total = sum of all
__device__ __forceinline__ double block_inclusive_scan(double v, double* red /* LDS [4] */, double* total) {
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
  for (int i = 0; i < kGenThreads / kWave; ++i) {
    if (i < (int)(threadIdx.x >> 6)) base += red[i];
    tot += red[i];
  }
  *total = tot;
  return base + inc;
}

template <class T>
__global__ void __launch_bounds__(kGenThreads) k_embed_generic(const GenArgs a) {
  __shared__ double lkey[kGenLdsElems];
  __shared__ int lidx[kGenLdsElems];
  __shared__ double red[4];
  const T* const w = (const T*)a.w;
  const T* const Xp = (const T*)a.Xp;
  const T* const Ke = (const T*)a.Ke;
  const T* const freqs = (const T*)a.freqs;
  const T* const bias = (const T*)a.bias;
  const T* const g = (const T*)a.g;
  T* const out = (T*)a.out;
  T* const gkey = (T*)a.gkey;
  T* const gfreq = (T*)a.gfreq;
  T* const gw = (T*)a.gw;
  char* myscr = a.scratch + (int64_t)blockIdx.x * a.line_elems * kGenScratchBytesPerElem;
  double* gkeyb = reinterpret_cast<double*>(myscr);                       // [line_elems] keys (rows above the LDS size)
  double* cw = gkeyb + a.line_elems;                                      // [line_elems] cumulative normalised weight
  double* hr = cw + a.line_elems;                                         // [line_elems] sum of gk H_t, then reverse sums
  double* gks = hr + a.line_elems;                                        // [line_elems] key gradient of the sorted element
  int* gidx = reinterpret_cast<int*>(gks + a.line_elems);                 // [line_elems]
  const bool backward = g != nullptr;
  const int tid = threadIdx.x;
  for (int64_t i = blockIdx.x; i < a.num_rows; i += gridDim.x) {
    const int64_t row = a.rows ? (int64_t)a.rows[i] : i;
    const int start = a.rowptr[row];
    const int D = a.rowptr[row + 1] - start;
    if (D < a.min_deg) continue;                                           // workgroup-uniform
    const int Dtot = D + 1;                                                // + the pad element
    int Dp = 1;
    while (Dp < Dtot) Dp <<= 1;
    const bool in_lds = Dp <= kGenLdsElems;
    double* keys = in_lds ? lkey : gkeyb;
    int* idx = in_lds ? lidx : gidx;
    // total mass, pad weight, normalisation (fsw_embedding.py:778-829)
    double part = 0.0;
    for (int t = tid; t < D; t += kGenThreads) part += w ? (double)w[start + t] : 1.0;
    const double m = block_sum(part, red);
    const double M = fmax(m, a.tau);
    const double padw = fmax(a.tau - m, 0.0);
    const double invM = 1.0 / M;
    auto raw_weight = [&](int e) -> double { return e < D ? (w ? (double)w[start + e] : 1.0) : (e == D ? padw : 0.0); };
    if (!backward && a.has_mass && tid == 0)
      out[row * a.ldo] = (T)mass_column(m, a.mass_fn, a.mass_scale, bias, a.out_scale);
    for (int s = 0; s < a.S; ++s) {
      // A. keys
      for (int t = tid; t < Dp; t += kGenThreads) {
        double key = __builtin_inf();
        if (t < D) {
          key = (double)Xp[(int64_t)a.col[start + t] * a.ldp + s];
          if (Ke) key += (double)Ke[(int64_t)(start + t) * a.ldke + s];
        } else if (t == D) {
          key = 0.0;
        }
        keys[t] = key;
        idx[t] = t;
      }
      __syncthreads();
      // B. bitonic sort by (key, index)
      for (int size = 2; size <= Dp; size <<= 1) {
        for (int st = size >> 1; st >= 1; st >>= 1) {
          for (int j = tid; j < Dp; j += kGenThreads) {
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
      // C. cumulative normalised weights in sorted order
      double run = 0.0;
      for (int b0 = 0; b0 < Dtot; b0 += kGenThreads) {
        const int t = b0 + tid;
        const double wv = t < Dtot ? raw_weight(idx[t]) * invM : 0.0;
        double tot;
        const double inc = block_inclusive_scan(wv, red, &tot);
        if (t < Dtot) cw[t] = run + inc;
        run += tot;
      }
      __syncthreads();
      if (backward)
        for (int t = tid; t < Dtot; t += kGenThreads) { gks[t] = 0.0; hr[t] = 0.0; }   // each t is owned by one thread below
      // D. readouts of the sorted slice (and the per-key coefficients for the backward)
      const int f0 = a.cartesian ? 0 : s, f1 = a.cartesian ? a.F : s + 1;
      for (int f = f0; f < f1; ++f) {
        const double xi = (double)freqs[f];
        const int64_t oc = (int64_t)a.has_mass + (a.cartesian ? (int64_t)s * a.F + f : (int64_t)s);
        const double gk = backward ? a.out_scale * (double)g[row * a.ldg + oc] : 0.0;
        if (backward && gk == 0.0) continue;                                           // workgroup-uniform
        double acc = 0.0, dacc = 0.0;
        for (int t = tid; t < Dtot; t += kGenThreads) {
          const double wv = raw_weight(idx[t]) * invM;
          const double c = cw[t];
          const double B = xi * (2.0 * c - wv);            // phase / pi
          const double sc = sinc_g(xi * wv);
          const double cb = cospi(B);
          const double delta = 2.0 * wv * sc * cb;
          const double key = keys[t];
          acc += delta * key;
          if (backward) {
            const double ddelta = 2.0 * wv * (wv * dsinc_g(xi * wv) * cb - sc * kPi * (2.0 * c - wv) * sinpi(B));
            dacc += (delta + (1.0 + xi) * ddelta) * key;
            gks[t] += gk * (1.0 + xi) * delta;
            if (gw) {
              const double knext = t + 1 < Dtot ? keys[t + 1] : 0.0;
              hr[t] += gk * 2.0 * (1.0 + xi) * cospi(2.0 * xi * c) * (key - knext);
            }
          }
        }
        if (!backward) {
          const double val = block_sum(acc, red);
          if (tid == 0) out[row * a.ldo + oc] = (T)(a.out_scale * ((1.0 + xi) * val + (bias ? (double)bias[oc] : 0.0)));
        } else if (gfreq) {
          const double dv = block_sum(dacc, red);
          if (tid == 0) atomic_add_t(&gfreq[f], gk * dv);
        }
      }
      if (backward) {
        if (gkey)
          for (int t = tid; t < Dtot; t += kGenThreads) {
            const int e = idx[t];
            if (e < D) gkey[(int64_t)(start + e) * a.ldk + s] = (T)gks[t];
          }
        if (gw) {
          // E. weights: reverse cumulative sums of H over the sorted order, sum_t H_t c_t, the pad element's rank
          __syncthreads();
          double hc = 0.0;
          for (int t = tid; t < Dtot; t += kGenThreads) hc += hr[t] * cw[t];
          const double HC = block_sum(hc, red);
          double runr = 0.0;
          const int nchunk = (Dtot + kGenThreads - 1) / kGenThreads;
          for (int cix = nchunk - 1; cix >= 0; --cix) {      // chunks from the end; inside a chunk the scan runs over mirrored threads
            const int t = cix * kGenThreads + (kGenThreads - 1 - tid);
            const double hv = t < Dtot ? hr[t] : 0.0;
            double tot;
            const double inc = block_inclusive_scan(hv, red, &tot);
            __syncthreads();
            if (t < Dtot) hr[t] = runr + inc;                // R(t) = sum_{s >= t} H_s
            runr += tot;
          }
          __syncthreads();
          double rp = 0.0;
          for (int t = tid; t < Dtot; t += kGenThreads)
            if (idx[t] == D) rp = hr[t];
          const double Rpad = block_sum(rp, red);
          const double corr = (m <= a.tau ? Rpad : 0.0) + (m >= a.tau ? HC : 0.0);
          for (int t = tid; t < Dtot; t += kGenThreads) {
            const int e = idx[t];
            const double v = (hr[t] - corr) * invM;
            if (e < D && v != 0.0) atomic_add_t(&gw[start + e], v);
          }
        }
      }
      __syncthreads();
    }
  }
}

// ---- float64 projection on the matrix cores: Xp [n, ldp] = X [n, ldx] . V [S, ldv]^T ---------------------------------------
// v_mfma_f64_16x16x4_f64: lane l supplies A[l % 16][l / 16] and B[l / 16][l % 16] of a 16 x 4 by 4 x 16 product and holds
// C[l / 16 + 4 i][l % 16], i < 4.  One wavefront per 16 x 16 output tile, operands straight from global memory (this is the
// float64 build for tests, reference fsw_embedding.py:909-913 in float64; the measured path is project.hip).
using f64x4 = __attribute__((ext_vector_type(4))) double;

__global__ void __launch_bounds__(256) k_project_f64(const double* __restrict__ X, int64_t n, int d, int64_t ldx,
                                                     const double* __restrict__ V, int S, int64_t ldv, double* __restrict__ Xp,
                                                     int64_t ldp, int32_t* __restrict__ stats) {
  const int lane = lane_id();
  const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nct = (S + 15) / 16;
  const int64_t rt = tile / nct;
  const int ct = (int)(tile - rt * nct);
  if (rt * 16 >= n) return;
  const int64_t r = rt * 16 + (lane & 15);
  const int c = ct * 16 + (lane & 15);
  const int kq = lane >> 4;
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  int nonfinite = 0;
  for (int k0 = 0; k0 < d; k0 += 4) {
    const int k = k0 + kq;
    const double av = (r < n && k < d) ? X[r * ldx + k] : 0.0;
    const double bv = (c < S && k < d) ? V[(int64_t)c * ldv + k] : 0.0;
    nonfinite |= !(fabs(av) <= 1.7976931348623157e308);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t orow = rt * 16 + kq + 4 * i;      // C/D map of the f64 MFMA: row = (lane >> 4) + 4 reg, col = lane & 15
    if (orow < n && c < S) Xp[orow * ldp + c] = acc[i];
  }
  if (stats && nonfinite && ct == 0) atomicOr(&stats[FSW_STAT_FLAGS], FSW_FLAG_X_NONFINITE);
}

// The scratch of a launch on num_rows rows of up to max_degree neighbours within `bytes` bytes: one line per workgroup, of the
// next power of two >= max_degree + 1 elements (the bitonic sort's size, pad element included).
struct GenScratch {
  int64_t line_elems;
  size_t wg_bytes;
  int64_t workgroups;   // 0: not even one line fits
};

static GenScratch generic_scratch_layout(int64_t max_degree, int64_t num_rows, size_t bytes) {
  GenScratch l;
  l.line_elems = 1;
  while (l.line_elems < max_degree + 1) l.line_elems <<= 1;
  l.wg_bytes = (size_t)l.line_elems * kGenScratchBytesPerElem;
  l.workgroups = std::min<int64_t>(std::min<int64_t>(num_rows, kGenMaxWorkgroups), (int64_t)(bytes / l.wg_bytes));
  return l;
}

static size_t generic_scratch_bytes(int64_t max_degree, int64_t num_rows) {
  const GenScratch l = generic_scratch_layout(max_degree, std::max<int64_t>(num_rows, 1), (size_t)1 << 30);
  return (size_t)std::max<int64_t>(l.workgroups, 1) * l.wg_bytes;
}

int launch_embed_generic(GenArgs a, int value_dtype, const int32_t* rows, int64_t num_rows, int min_deg, hipStream_t stream) {
  a.rows = rows;
  a.num_rows = num_rows;
  a.min_deg = min_deg;
  const GenScratch l = generic_scratch_layout(a.max_degree, num_rows, a.scratch ? a.scratch_bytes : 0);
  a.line_elems = l.line_elems;
  FSW_REQUIRE(l.workgroups >= 1, a.cartesian ? "fsw_embed_cart: scratch buffer too small (need fsw_embed_cart_generic_scratch_bytes)"
                                             : "fsw_embed_generic: scratch buffer too small (need fsw_embed_generic_scratch_bytes)");
  if (value_dtype == 0) k_embed_generic<float><<<(unsigned)l.workgroups, kGenThreads, 0, stream>>>(a);
  else k_embed_generic<double><<<(unsigned)l.workgroups, kGenThreads, 0, stream>>>(a);
  FSW_LAUNCH_CHECK();
  return 0;
}

}  // namespace fsw

using namespace fsw;

extern "C" size_t fsw_embed_generic_scratch_bytes(int64_t max_degree, int64_t num_rows) {
  return generic_scratch_bytes(max_degree, num_rows);
}

extern "C" size_t fsw_embed_cart_generic_scratch_bytes(int64_t max_degree, int64_t num_rows) {
  return generic_scratch_bytes(max_degree, num_rows);
}

extern "C" int fsw_embed_generic(const fsw_generic_args* g, fsw_stream_t stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  FSW_REQUIRE(g, "fsw_embed_generic: null args");
  FSW_REQUIRE(g->value_dtype == 0 || g->value_dtype == 1, "fsw_embed_generic: value_dtype must be 0 (float32) or 1 (float64)");
  FSW_REQUIRE(g->rowptr && g->Xp && g->freqs && g->scratch && (g->num_rows == 0 || g->col || g->max_degree == 0), "fsw_embed_generic: null pointer");
  FSW_REQUIRE(g->num_rows >= 0 && g->S >= 1 && g->ldp >= g->S && g->max_degree >= 0 && g->tau > 0.0, "fsw_embed_generic: bad sizes");
  FSW_REQUIRE(!g->Ke || g->ldke >= g->S, "fsw_embed_generic: bad edge-term stride");
  if (g->g) {
    FSW_REQUIRE(g->ldg >= g->S + g->has_mass && (!g->gkey || g->ldk >= g->S), "fsw_embed_generic: bad gradient strides");
  } else {
    FSW_REQUIRE(g->out && g->ldo >= g->S + g->has_mass, "fsw_embed_generic: bad output");
  }
  if (g->num_rows == 0) return 0;
  GenArgs a = generic_args(*g, false, 1);
  a.Ke = g->Ke;
  a.ldke = g->ldke;
  return launch_embed_generic(a, g->value_dtype, nullptr, g->num_rows, 0, stream);
}

extern "C" int fsw_project_f64(const double* X, int64_t n, int d, int64_t ldx, const double* V, int S, int64_t ldv, double* Xp,
                               int64_t ldp, int32_t* stats, fsw_stream_t stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  FSW_REQUIRE(X && V && Xp && n >= 1 && d >= 1 && S >= 1 && ldx >= d && ldv >= d && ldp >= S, "fsw_project_f64: bad arguments");
  const int64_t tiles = ceil_div(n, 16) * ceil_div(S, 16);
  FSW_REQUIRE(ceil_div(tiles, 4) < (1ll << 31), "fsw_project_f64: grid too large");
  k_project_f64<<<(unsigned)ceil_div(tiles, 4), 256, 0, stream>>>(X, n, d, ldx, V, S, ldv, Xp, ldp, stats);
  FSW_LAUNCH_CHECK();
  return 0;
}
