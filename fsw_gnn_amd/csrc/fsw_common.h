// Shared host/device helpers for libfsw_hip.so (gfx950 only).
#pragma once
#include <stdlib.h>
#include <algorithm>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <atomic>
#include "../../include/fsw_hip.h"

namespace fsw {

void set_error(const char* fmt, ...);

#define FSW_CHECK_HIP(expr)                                                              \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      fsw::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return 2;                                                                          \
    }                                                                                    \
  } while (0)

#define FSW_REQUIRE(cond, ...)            \
  do {                                    \
    if (!(cond)) {                        \
      fsw::set_error(__VA_ARGS__);        \
      return 1;                           \
    }                                     \
  } while (0)

#define FSW_LAUNCH_CHECK() FSW_CHECK_HIP(hipGetLastError())

// Function attributes (the dynamic-LDS ceiling of a kernel) belong to a DEVICE: one flag per device ordinal and call site, so
// a process that uses several GPUs sets them on each (racing host threads at worst set the same value twice).
struct PerDeviceOnce {
  std::atomic<bool> done[64];
};
#define FSW_SET_MAX_LDS_ONCE(kernel, bytes)                                                                          \
  do {                                                                                                               \
    static fsw::PerDeviceOnce once_;                                                                                 \
    int dev_ = 0;                                                                                                    \
    FSW_CHECK_HIP(hipGetDevice(&dev_));                                                                              \
    if (dev_ < 0 || dev_ >= 64 || !once_.done[dev_].load(std::memory_order_relaxed)) {                               \
      FSW_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes))); \
      if (dev_ >= 0 && dev_ < 64) once_.done[dev_].store(true, std::memory_order_relaxed);                           \
    }                                                                                                                \
  } while (0)

constexpr int kWave = 64;

__host__ __device__ inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

__device__ __forceinline__ int lane_id() { return threadIdx.x & (kWave - 1); }
// wave index inside the workgroup as a provably wave-uniform (SGPR) value
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// edge features: key + <e_ij, v_k[d_in:]> of CSR entry `entry` and slice k (reference fsw_embedding.py:934-968)
__device__ __forceinline__ float add_edge_term(float key, int64_t entry, int k, const float* efeat, const float* Ve, int64_t ldve,
                                               int d_edge) {
  const float* er = efeat + entry * d_edge;
  const float* vr = Ve + (int64_t)k * ldve;
  for (int q = 0; q < d_edge; ++q) key = fmaf(er[q], vr[q], key);
  return key;
}

// the exact degree bins 1 .. FSW_REG_MAX_DEG as switch cases (conv_fused.hip has its own list from 0)
#define FSW_CASES_1_32(X)                                                                                              \
  X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) X(21) \
  X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)

__host__ __device__ inline int degree_bin(int deg) {
  if (deg <= FSW_REG_MAX_DEG) return deg;
  if (deg > FSW_HUB_MAX_DEG) return FSW_BIN_GLOBAL;
  if (deg > FSW_LDS_MAX_DEG) return FSW_BIN_HUB0 + (deg > 4096) + (deg > 8192) + (deg > 16384);
  if (deg > FSW_MID_MAX_DEG) return FSW_BIN_LDS0 + (deg > 512) + (deg > 1024);
  constexpr int sizes[FSW_NUM_MID_BINS] = FSW_MID_SIZES;
  int i = 0;
#pragma unroll
  for (int j = 0; j < FSW_NUM_MID_BINS - 1; ++j) i += deg > sizes[j];
  return FSW_BIN_MID0 + i;
}

// general weights without edge features: rows of up to this many neighbours (+ the pad element = 8192 = four wavefronts x 32 keys per
// lane) keep their (key, weight) line in registers (embed_hub.hip: k_embed_hub_w); above, sorted blocks + merge path (k_embed_mergepath_w)
constexpr int kHubWMaxDeg = 8191;

// rows of the degree bins lo .. hi when the caller passed the host copy of bin_start, `upper` (a bound) otherwise
inline int64_t bin_rows_or(const fsw_embed_args& a, int lo, int hi, int64_t upper) {
  return a.bin_start_host ? (int64_t)a.bin_start_host[hi + 1] - a.bin_start_host[lo] : upper;
}

__host__ __device__ inline uint32_t pow2ceil(uint32_t v) {
  uint32_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

constexpr double kPi = 3.14159265358979323846;

// total-mass encoding (reference fsw_embedding.py:857-865): identity | 2 (sqrt(1 + m) - 1), written without cancellation | log(1 + m)
__device__ __forceinline__ float mass_encode(float m, int fn) {
  if (fn == 1) return 2.f * (m / (sqrtf(m + 1.f) + 1.f));
  if (fn == 2) return log1pf(m);
  return m;
}
__device__ __forceinline__ double mass_encode(double m, int fn) {   // the float64 paths of embed_generic.hip / embed_cart.hip
  if (fn == 1) return 2.0 * (m / (sqrt(m + 1.0) + 1.0));
  if (fn == 2) return log1p(m);
  return m;
}
// value of the total-mass output column of a row of total mass m; b0: the column's bias (0 without bias).  (k_embed_mid_* and
// k_embed_hub_q4 write the expression out: with the branches of the encoding and of the bias inlined through this function their
// sorting networks get another register allocation.)
__device__ __forceinline__ float mass_column(float m, int mass_fn, float mass_scale, float b0, float out_scale) {
  return out_scale * (mass_encode(m, mass_fn) * mass_scale + b0);
}
__device__ __forceinline__ float mass_column(float m, int mass_fn, float mass_scale, const float* bias, float out_scale) {
  return out_scale * (mass_encode(m, mass_fn) * mass_scale + (bias ? bias[0] : 0.f));
}
template <class T>   // float64 arithmetic, bias in the output's precision
__device__ __forceinline__ double mass_column(double m, int mass_fn, double mass_scale, const T* bias, double out_scale) {
  return out_scale * (mass_encode(m, mass_fn) * mass_scale + (bias ? (double)bias[0] : 0.0));
}

// sin(2 pi x) for a float64 phase x in revolutions: reduced in float64, evaluated in float32 with relative accuracy (sinpif on |r| <= 1)
__device__ __forceinline__ float sin2pi_rev(double x) {
  const double r = x - rint(x);
  return sinpif(2.f * (float)r);
}

// The pad element's weight max(tau - m, 0) lives in a float lane array next to the neighbours' float weights, but the cumulative
// weight is a float64 sum and the phase 2 pi xi c magnifies what that rounding loses (3e-8 of the denominator) by 2 pi xi:
// 1e-4 at xi = 511.  pad_residual: the part of the pad weight its float copy padw does not hold, exact in float64 (deficit = tau - m
// in float64).  It is added to the cumulative weight from the pad element on.
__device__ __forceinline__ double pad_residual(double deficit, float padw) { return fmax(deficit, 0.0) - (double)padw; }
// Forward kernels: an element's coefficient is multiplied by its key, and every element with key == 0 contributes nothing, so
// adding the residual to the cumulative weight of every element with key >= 0 (-0.0 included) is exact wherever the pad element
// ranks among the zeros.  rho == 0 unless the row is deficient.
__device__ __forceinline__ double pad_residual_at(double rho, float key) { return key >= 0.f ? rho : 0.0; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// sum of v over the lanes below this one
__device__ __forceinline__ double wave_exclusive_scan_f64(double v) {
  double inc = v;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const double t = __shfl_up(inc, off);
    if (lane_id() >= off) inc += t;
  }
  return inc - v;
}
// sum of v over the lanes above this one
__device__ __forceinline__ double wave_reverse_exclusive_scan_f64(double v) {
  double inc = v;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const double t = __shfl_down(inc, off);
    if (lane_id() + off < kWave) inc += t;
  }
  const double above = __shfl_down(inc, 1);
  return lane_id() == kWave - 1 ? 0.0 : above;
}

// gradient accumulators are float32 or float64 (the generic / Cartesian paths in either precision)
__device__ __forceinline__ void atomic_add_t(float* p, double v) { atomicAdd(p, (float)v); }
__device__ __forceinline__ void atomic_add_t(double* p, double v) { atomicAdd(p, v); }

// sin and cos of 2 pi x for x in REVOLUTIONS (|x| < 2^40), absolute error ~1e-15: reduction to [-1/8, 1/8] revolutions around the
// nearest quarter turn (exact in float64), Taylor polynomials on |angle| <= pi/4, quadrant fix-up.  About a third of the
// instructions of sincospi() -- the long-row kernels evaluate two of these per lane and row to start a recurrence.
__device__ __forceinline__ void sincos_rev(double x, double* s, double* c) {
  const double r = x - rint(x);                 // [-1/2, 1/2]
  const double qd = rint(4.0 * r);              // -2 .. 2
  const double a = (r - 0.25 * qd) * 6.283185307179586476925;
  const double a2 = a * a;
  double sp = 1.0 / 6227020800.0;
  sp = fma(sp, a2, -1.0 / 39916800.0);
  sp = fma(sp, a2, 1.0 / 362880.0);
  sp = fma(sp, a2, -1.0 / 5040.0);
  sp = fma(sp, a2, 1.0 / 120.0);
  sp = fma(sp, a2, -1.0 / 6.0);
  const double sa = fma(sp * a2, a, a);
  double cp = -1.0 / 87178291200.0;
  cp = fma(cp, a2, 1.0 / 479001600.0);
  cp = fma(cp, a2, -1.0 / 3628800.0);
  cp = fma(cp, a2, 1.0 / 40320.0);
  cp = fma(cp, a2, -1.0 / 720.0);
  cp = fma(cp, a2, 1.0 / 24.0);
  cp = fma(cp, a2, -0.5);
  const double ca = fma(cp, a2, 1.0);
  const int q = (int)qd & 3;                    // angle = a + q pi / 2
  const double s1 = (q & 1) ? ca : sa, c1 = (q & 1) ? sa : ca;
  *s = (q & 2) ? -s1 : s1;
  *c = (q == 1 || q == 2) ? -c1 : c1;
}

// Unit weights (c_t = t / D): coefficient of rank r in a neighbourhood of D at frequency xi,
//   (1 + xi) [sin(2 pi xi (r + 1) / D) - sin(2 pi xi r / D)] / (pi xi)  =  B cos(2 pi step (r + 1/2)),   step = xi / D,
//   B = (1 + xi) / (pi xi) * 2 sin(pi step)
// (reference fsw_embedding.py:1047-1075, 1109 with weights 1 / D, by sum-to-product).  The cosines of consecutive ranks obey
// c_{r+1} = 2 cos(2 pi step) c_r - c_{r-1}: ONE float64 FMA per rank (rounding error after m steps <= m^2 2^-53; every lane
// restarts from exact values at its first rank).
struct UnitCoef {
  double twoc, cur, prev;   // 2 cos(2 pi step), cos(phi_r), cos(phi_{r-1}) for the next rank r
  float B;
  __device__ __forceinline__ void start(double xi, int D, int r0) {
    const double step = xi / (double)D;          // revolutions per rank
    double sh, ch, s0, c0;
    sincos_rev(0.5 * step, &sh, &ch);
    sincos_rev(step * ((double)r0 + 0.5), &s0, &c0);
    const double sd = 2.0 * sh * ch, cd = fma(-2.0 * sh, sh, 1.0);
    twoc = 2.0 * cd;
    cur = c0;
    prev = fma(c0, cd, s0 * sd);                 // cos(phi - theta)
    B = (float)((1.0 + xi) / (kPi * xi) * 2.0 * sh);
  }
  __device__ __forceinline__ float next() {     // cos(phi_r) of the current rank, then advance
    const float v = (float)cur;
    const double n = fma(twoc, cur, -prev);
    prev = cur;
    cur = n;
    return v;
  }
};

// Workgroup index b -> (degree D, perm range [p, pe)) for the kernels that walk the degree bins DHI, DHI - 1, .. DLO in tiles of ROWS
// rows (one degree per workgroup, the longest rows first).  ONE vector load of the bin table (lane l: bin_start[l]) and a wave-level
// suffix sum.  The loop this replaces read bin_start[D], bin_start[D + 1] with scalar loads, bin after bin until it found the tile:
// ~20 DEPENDENT loads, and under the kernels' col-index stream (every neighbour index is a scalar load) they miss the scalar cache --
// the s_memtime stamps of tools/exp_fused_stamps.py put 19 us of a workgroup's 91 us before its first gather.
template <int ROWS>
__device__ __forceinline__ bool find_degree_tile(const int32_t* __restrict__ bin_start, int DLO, int DHI, int b, int& D, int& p, int& pe) {
  static_assert(FSW_REG_MAX_DEG + 1 < 64, "one lane per degree bin");
  const int lane = (int)__lane_id();
  const int lo = bin_start[min(lane, FSW_REG_MAX_DEG + 1)];
  const int hi = __shfl_down(lo, 1);
  const bool mine = lane >= DLO && lane <= DHI;
  const int nb = mine ? (hi - lo + ROWS - 1) / ROWS : 0;
  int suf = nb;                                            // tiles of the bins >= lane
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_down(suf, off);
    if (lane + off < 64) suf += t;
  }
  const int before = suf - nb;                             // tiles of the bins above this one: they come first
  const unsigned long long hit = __ballot(mine && b >= before && b < suf);
  if (!hit) return false;
  D = __ffsll((long long)hit) - 1;
  const int lo_d = __builtin_amdgcn_readlane(lo, D), hi_d = __builtin_amdgcn_readlane(hi, D);
  p = lo_d + (b - __builtin_amdgcn_readlane(before, D)) * ROWS;
  pe = min(p + ROWS, hi_d);
  return true;
}

static_assert(FSW_NUM_LDS_BINS == 3 && FSW_MID_MAX_DEG == 256 && FSW_LDS_MAX_DEG == 2048, "degree_bin assumes LDS bins 512 / 1024 / 2048");
static_assert(FSW_NUM_HUB_BINS == 4 && FSW_HUB_MAX_DEG == 32768, "degree_bin assumes hub bins 4096 / 8192 / 16384 / 32768");

}  // namespace fsw
