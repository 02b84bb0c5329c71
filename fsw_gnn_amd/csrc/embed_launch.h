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

// embed_generic.hip: the generic kernel (any degree, float32 or float64 storage behind the void pointers, float64 arithmetic),
// forward (g == null) or backward.  Sorted slice s is read out at freqs[s] into column has_mass + s (diagonal), or, cartesian, at
// every freqs[f], f < F, into column has_mass + s F + f.
struct GenArgs {
  const int32_t* rowptr;
  const int32_t* col;
  const void* w;         // [nnz] raw weights or null (unit)
  const int32_t* rows;   // null: rows 0 .. num_rows - 1; else rows[0 .. num_rows - 1] (the long rows of the tuned Cartesian entries)
  int64_t num_rows;
  int min_deg;           // rows of fewer neighbours are skipped (they belong to another kernel)
  const void* Xp;        // [num_cols, ldp]
  int64_t ldp;
  const void* Ke;        // [nnz, ldke] edge-feature term of every key, or null
  int64_t ldke;
  const void* freqs;
  int S, F;
  bool cartesian;
  double tau;
  // forward
  void* out;
  int64_t ldo;
  const void* bias;
  double out_scale;
  int has_mass, mass_fn;
  double mass_scale;
  // backward: gkey [nnz, ldk] stored, gfreq and gw [nnz] accumulated with atomics (zeroed by the caller)
  const void* g;
  int64_t ldg;
  void* gkey;
  int64_t ldk;
  void* gfreq;
  void* gw;
  // scratch: per workgroup line_elems * kGenScratchBytesPerElem bytes (max_degree and scratch_bytes: for the launcher)
  char* scratch;
  size_t scratch_bytes;
  int64_t max_degree, line_elems;
};
constexpr int kGenScratchBytesPerElem = 8 + 4 + 8 + 8 + 8;   // key, index, cumulative weight, H / reverse sum, key gradient

// the fields fsw_generic_args and fsw_cart_args have in common by name (rows, num_rows, min_deg, line_elems: the launcher's)
template <class P>
GenArgs generic_args(const P& p, bool cartesian, int F) {
  GenArgs a = {};
  a.rowptr = p.rowptr; a.col = p.col; a.w = p.w; a.Xp = p.Xp; a.ldp = p.ldp; a.freqs = p.freqs; a.S = p.S; a.F = F;
  a.cartesian = cartesian; a.tau = p.tau; a.out = p.out; a.ldo = p.ldo; a.bias = p.bias; a.out_scale = p.out_scale;
  a.has_mass = p.has_mass; a.mass_fn = p.mass_fn; a.mass_scale = p.mass_scale;
  a.g = p.g; a.ldg = p.ldg; a.gkey = p.gkey; a.ldk = p.ldk; a.gfreq = p.gfreq; a.gw = p.gw;
  a.scratch = (char*)p.scratch; a.scratch_bytes = p.scratch_bytes; a.max_degree = p.max_degree;
  return a;
}
// value_dtype 0 float32, 1 float64; rows[0 .. num_rows - 1] (null: all of 0 .. num_rows - 1) of at least min_deg neighbours
int launch_embed_generic(GenArgs a, int value_dtype, const int32_t* rows, int64_t num_rows, int min_deg, hipStream_t stream);

// backward with the gradient of the weights (fsw_embed_backward_w_f32, embed_w_bwd.hip): register kernels for rows of up to
// kWRegMaxDeg neighbours, embed_w_sort_bwd.hip (one (row, slice) line per wavefront) up to kWSortMaxDeg, embed_w_long_bwd.hip (one
// wavefront per (row, kWLongSlices slices) on a scratch line in global memory) above.
// 1024, not FSW_LDS_MAX_DEG: the instance of 64 ranks per lane for 1025 .. 2048 neighbours spills (DESIGN.md has the table).
constexpr int kWRegMaxDeg = 24;
constexpr int kWSortMaxDeg = 1024;
constexpr int kWSortLastBin = FSW_BIN_LDS0 + 1;   // 513 .. 1024
int launch_embed_wsort_w_bwd(const fsw_embed_args& a, const float* w_lo, const float* g, int64_t ldg, float* gkey, int64_t ldk, float* gfreq,
                             float* gw, hipStream_t stream);
// embed_w_long_bwd.hip.  kWLongSlices (fsw_embed_backward_w_long_slices): the slices a wavefront sums in float64 before its one
// float32 add per entry -- DESIGN.md, "Rows above 1024 neighbours", says why 4.  kWLongRanks: ranks per lane of a chunk (chunks of
// 1024 words; the instance of 32 spills 12 bytes per lane at 512 registers: the table there).
constexpr int kWLongSlices = 4;
constexpr int kWLongRanks = 16;
int launch_embed_w_long_bwd(const fsw_embed_args& a, const float* w_lo, int64_t max_degree, const float* g, int64_t ldg, float* gkey,
                            int64_t ldk, float* gfreq, float* gw, void* scratch, size_t scratch_bytes, hipStream_t stream);

// backward: embed_mid_bwd.hip (33 .. 128) and embed_wsort_bwd.hip (everything above FSW_REG_MAX_DEG; global: rows above FSW_LDS_MAX_DEG)
int launch_embed_mid_bwd(const fsw_embed_args& a, int64_t rows_upper, const float* g, int64_t ldg, float* gXp, int64_t ldgp,
                         float* gfreq, float* gkey, int64_t ldk, hipStream_t stream);
int launch_embed_long_bwd(const fsw_embed_args& a, bool global, int64_t rows_upper, const float* g, int64_t ldg, float* gXp,
                          int64_t ldgp, float* gfreq, float* gkey, int64_t ldk, hipStream_t stream);

}  // namespace fsw
