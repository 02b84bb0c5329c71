// Host launchers of the neighbourhood-embed kernels that are called from another file of csrc/.  Every launcher enqueues on `stream`
// and returns 0 or the error code of FSW_REQUIRE / FSW_CHECK_HIP; rows_upper bounds the rows of the launcher's degree range (the
// per-bin counts stay on the device unless the caller passed bin_start_host).  fsw_embed_f32 (embed_api.hip) shows which launcher
// takes which (weights, in-degree) class; the backward's classes are in launch_embed_long_bwd (embed_wsort_bwd.hip).
#pragma once
#include "fsw_common.h"

namespace fsw {

// embed_reg.hip
int launch_unit_table(const float* freqs, int S, int max_deg, float* table, int64_t ldt, hipStream_t stream);
int launch_zero_rows(const fsw_embed_args& a, hipStream_t stream);
int launch_embed_reg(const fsw_embed_args& a, bool unit_fast, int64_t rows_upper, hipStream_t stream);              // 1 .. 32

// embed_mid.hip: one lane per slice, the row in the lane's registers
int launch_embed_mid_unit(const fsw_embed_args& a, int64_t rows_upper, hipStream_t stream);                         // 33 .. 256
int launch_embed_mid_weighted(const fsw_embed_args& a, int64_t rows_upper, hipStream_t stream);                     // 33 .. 128

// embed_hub.hip, unit weights with tau <= 1: one line per wavefront / workgroup, in registers
int launch_embed_ws_unit(const fsw_embed_args& a, int64_t rows_upper, hipStream_t stream);                          // 257 .. 2048
int launch_embed_hub(const fsw_embed_args& a, int64_t rows_upper, hipStream_t stream);                              // 2049 .. 32768
int launch_embed_giant(const fsw_embed_args& a, int64_t rows_upper, hipStream_t stream);                            // above
// embed_hub.hip, general weights without edge features: (key, weight) lines in registers
int launch_embed_hub_weighted_lds(const fsw_embed_args& a, int64_t rows_upper, hipStream_t stream);                 // 129 .. 2048
int launch_embed_hub_weighted_hub(const fsw_embed_args& a, int64_t rows_upper, hipStream_t stream);                 // 2049 .. kHubWMaxDeg
int launch_embed_mergepath_w(const fsw_embed_args& a, int bin_lo, int bin_hi, int dlo, int64_t rows_upper, hipStream_t stream);   // above

// embed_wsort.hip, general weights with edge features: LDS-staged lines / one scratch line per wavefront
int launch_embed_wsort_lds(const fsw_embed_args& a, int64_t rows_upper, hipStream_t stream);                        // 129 .. 2048
int launch_embed_wsort_global(const fsw_embed_args& a, int64_t rows_upper, hipStream_t stream);                     // above
size_t embed_global_scratch_bytes(int64_t max_degree);                                                              // embed_wsort_bwd.hip

// backward: embed_mid_bwd.hip (33 .. 128) and embed_wsort_bwd.hip (everything above FSW_REG_MAX_DEG; global: rows above FSW_LDS_MAX_DEG)
int launch_embed_mid_bwd(const fsw_embed_args& a, int64_t rows_upper, const float* g, int64_t ldg, float* gXp, int64_t ldgp,
                         float* gfreq, float* gkey, int64_t ldk, hipStream_t stream);
int launch_embed_long_bwd(const fsw_embed_args& a, bool global, int64_t rows_upper, const float* g, int64_t ldg, float* gXp,
                          int64_t ldgp, float* gfreq, float* gkey, int64_t ldk, hipStream_t stream);

}  // namespace fsw
