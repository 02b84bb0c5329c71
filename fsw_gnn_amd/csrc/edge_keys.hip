// Cartesian mode with edge features: the key of every CSR entry, materialised once (fsw_edge_keys_f32, include/fsw_hip.h).
//
//   K[e, s] = Xp[col[e], s], then key = fmaf(efeat[e, q], Ve[s, q], key) for q = 0 .. d_edge - 1 in that order
//
// -- the rounding rule of the diagonal edge-feature kernels (embed_reg.hip, embed_wsort.hip), so that the Cartesian kernels, which form
// their key at ONE site, Xp[col[start + t] * ldp + s], run unchanged on (K, the identity column array).
//
// Mapping: slice index minor.  A group of G = 2^k <= 64 lanes owns one entry at a time: its lanes read the S contiguous floats of one Xp
// row and write S contiguous floats of K (four per lane when S, the strides and the pointers allow 16-byte accesses, one otherwise);
// col[e] and efeat[e, :] are the same addresses for every lane of the group (one request each).  Ve is staged once per workgroup in LDS,
// transposed to [q][s] so that consecutive lanes read consecutive words; the workgroups stride over the entries, so a workgroup stages it
// once for many entries.  When S * d_edge does not fit (kMaxLdsFloats) the lanes read Ve from global memory (L2-resident) instead.
// Streaming: nnz * (4 + 4 d_edge + 8 S) bytes.  Entries are indexed in 64 bits (nnz up to 2^31 - 1, K up to nnz * ldk floats).
#include "fsw_common.h"

using namespace fsw;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxLdsFloats = 8192;   // 32 KiB of Ve per workgroup: four workgroups per CU keep their copy
constexpr int kMaxBlocks = 2048;      // 8 per CU: the workgroups stride over the entries

// VEC: floats per lane and access (4: S % 4 == 0, ldp % 4 == 0, ldk % 4 == 0, 16-byte aligned Xp and K).  LDS: Ve staged in LDS as
// [d_edge][Sp] (Sp = S rounded up to VEC), else read in place.  lg: log2 of the lanes per entry.
template <int VEC, bool LDS>
__global__ __launch_bounds__(kThreads) void k_edge_keys(const int32_t* __restrict__ col, int64_t nnz, const float* __restrict__ Xp,
                                                        int64_t ldp, const float* __restrict__ efeat, int d_edge,
                                                        const float* __restrict__ Ve, int64_t ldve, int S, float* __restrict__ K,
                                                        int64_t ldk, int lg) {
  extern __shared__ __attribute__((aligned(16))) float ve_lds[];
  const int U = S / VEC;              // accesses per entry (VEC == 4: S % 4 == 0)
  if (LDS) {
    for (int i = threadIdx.x; i < S * d_edge; i += kThreads) {
      const int s = i / d_edge, q = i - s * d_edge;
      ve_lds[q * S + s] = Ve[(int64_t)s * ldve + q];
    }
    __syncthreads();
  }
  const int G = 1 << lg;
  const int u0 = threadIdx.x & (G - 1);
  const int64_t per_block = kThreads >> lg;
  for (int64_t e = (int64_t)blockIdx.x * per_block + (threadIdx.x >> lg); e < nnz; e += (int64_t)gridDim.x * per_block) {
    const float* __restrict__ xrow = Xp + (int64_t)col[e] * ldp;
    const float* __restrict__ ef = efeat + e * d_edge;
    float* __restrict__ krow = K + e * ldk;
    for (int u = u0; u < U; u += G) {
      const int s = u * VEC;
      if (VEC == 4) {
        float4 key = *reinterpret_cast<const float4*>(xrow + s);
        for (int q = 0; q < d_edge; ++q) {
          const float f = ef[q];
          float4 v;
          if (LDS) {
            v = *reinterpret_cast<const float4*>(ve_lds + q * S + s);
          } else {
            v = make_float4(Ve[(int64_t)s * ldve + q], Ve[(int64_t)(s + 1) * ldve + q], Ve[(int64_t)(s + 2) * ldve + q],
                            Ve[(int64_t)(s + 3) * ldve + q]);
          }
          key.x = __fmaf_rn(f, v.x, key.x);
          key.y = __fmaf_rn(f, v.y, key.y);
          key.z = __fmaf_rn(f, v.z, key.z);
          key.w = __fmaf_rn(f, v.w, key.w);
        }
        *reinterpret_cast<float4*>(krow + s) = key;
      } else {
        float key = xrow[s];
        for (int q = 0; q < d_edge; ++q) key = __fmaf_rn(ef[q], LDS ? ve_lds[q * S + s] : Ve[(int64_t)s * ldve + q], key);
        krow[s] = key;
      }
    }
  }
}

template <int VEC, bool LDS>
int launch(const int32_t* col, int64_t nnz, const float* Xp, int64_t ldp, const float* efeat, int d_edge, const float* Ve, int64_t ldve,
           int S, float* K, int64_t ldk, hipStream_t stream) {
  const int U = S / VEC;
  int lg = 0;
  while ((1 << lg) < U && lg < 6) ++lg;       // lanes per entry: the power of two >= U, at most a wavefront
  const int64_t per_block = kThreads >> lg;
  const int64_t blocks = std::min<int64_t>(ceil_div(nnz, per_block), kMaxBlocks);
  const size_t lds = LDS ? (size_t)S * d_edge * sizeof(float) : 0;
  hipLaunchKernelGGL((k_edge_keys<VEC, LDS>), dim3((unsigned)blocks), dim3(kThreads), lds, stream, col, nnz, Xp, ldp, efeat, d_edge, Ve,
                     ldve, S, K, ldk, lg);
  FSW_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int fsw_edge_keys_f32(const int32_t* col, int64_t nnz, const float* Xp, int64_t ldp, const float* efeat, int d_edge,
                                 const float* Ve, int64_t ldve, int S, float* K, int64_t ldk, fsw_stream_t stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  FSW_REQUIRE(nnz >= 0 && nnz <= INT32_MAX, "fsw_edge_keys_f32: need 0 <= nnz < 2^31");
  FSW_REQUIRE(S >= 1 && d_edge >= 1, "fsw_edge_keys_f32: need S >= 1 and d_edge >= 1");
  FSW_REQUIRE(ldp >= S && ldk >= S && ldve >= d_edge, "fsw_edge_keys_f32: need ldp >= S, ldk >= S, ldve >= d_edge");
  if (nnz == 0) return 0;
  FSW_REQUIRE(col && Xp && efeat && Ve && K, "fsw_edge_keys_f32: null pointer");
  const bool vec = S % 4 == 0 && ldp % 4 == 0 && ldk % 4 == 0 && (reinterpret_cast<uintptr_t>(Xp) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(K) & 15) == 0;
  const bool lds = (int64_t)S * d_edge <= kMaxLdsFloats;
  if (vec) {
    return lds ? launch<4, true>(col, nnz, Xp, ldp, efeat, d_edge, Ve, ldve, S, K, ldk, stream)
               : launch<4, false>(col, nnz, Xp, ldp, efeat, d_edge, Ve, ldve, S, K, ldk, stream);
  }
  return lds ? launch<1, true>(col, nnz, Xp, ldp, efeat, d_edge, Ve, ldve, S, K, ldk, stream)
             : launch<1, false>(col, nnz, Xp, ldp, efeat, d_edge, Ve, ldve, S, K, ldk, stream);
}
