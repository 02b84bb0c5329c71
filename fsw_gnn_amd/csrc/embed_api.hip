// C-ABI entry points of the fused neighbourhood embed: argument checks and per-degree-class dispatch.
#include "embed_launch.h"

using namespace fsw;

extern "C" size_t fsw_unit_table_rows(int max_deg) { return (size_t)max_deg * (max_deg + 1) / 2; }

extern "C" int fsw_unit_coeff_table(const float* freqs, int S, int max_deg, float* table, int64_t ldt, fsw_stream_t stream) {
  FSW_REQUIRE(freqs && table, "fsw_unit_coeff_table: null pointer");
  FSW_REQUIRE(S >= 1 && ldt >= S && max_deg >= 1 && max_deg <= FSW_REG_MAX_DEG,
              "fsw_unit_coeff_table: need S >= 1, ldt >= S, 1 <= max_deg <= %d", FSW_REG_MAX_DEG);
  return launch_unit_table(freqs, S, max_deg, table, ldt, reinterpret_cast<hipStream_t>(stream));
}

extern "C" size_t fsw_embed_scratch_bytes(int64_t max_degree) {
  return max_degree > FSW_LDS_MAX_DEG ? embed_global_scratch_bytes(max_degree) : 0;
}

extern "C" int fsw_embed_f32(const fsw_embed_args* args, fsw_stream_t stream_) {
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
  FSW_REQUIRE(args, "fsw_embed_f32: null args");
  const fsw_embed_args& a = *args;
  FSW_REQUIRE(a.rowptr && a.perm && a.bin_start && a.Xp && a.freqs && a.out, "fsw_embed_f32: null pointer");
  FSW_REQUIRE(a.num_rows >= 1 && a.S >= 1 && a.ldp >= a.S && a.ldo >= a.S + a.has_mass, "fsw_embed_f32: bad sizes");
  FSW_REQUIRE(a.tau > 0.f, "fsw_embed_f32: total_mass_pad_thresh must be positive");  // reference fsw_embedding.py:637
  FSW_REQUIRE(a.has_mass == 0 || a.has_mass == 1, "fsw_embed_f32: has_mass must be 0 or 1");
  FSW_REQUIRE(a.mass_fn >= 0 && a.mass_fn <= 2, "fsw_embed_f32: mass_fn must be 0, 1 or 2");
  FSW_REQUIRE(!a.efeat || (a.w && a.Ve && a.d_edge >= 1 && a.ldve >= a.d_edge),
              "fsw_embed_f32: edge features need a coalesced weighted graph (fsw_graph_build_coalesced) and Ve");
  const bool unit_fast = (a.w == nullptr) && (a.tau <= 1.f);
  FSW_REQUIRE(!unit_fast || (a.unit_table && a.ldt >= a.S), "fsw_embed_f32: unit weights with tau <= 1 need unit_table");

  const int64_t nz = a.num_zero_rows < 0 ? a.num_rows : a.num_zero_rows;
  const int64_t nreg = a.num_reg_rows < 0 ? a.num_rows : a.num_reg_rows;
  const int64_t nlds = a.num_lds_rows < 0 ? a.num_rows : a.num_lds_rows;
  const int64_t nglob = a.num_global_rows < 0 ? a.num_rows : a.num_global_rows;
  int rc;
  if (nz > 0 && (rc = launch_zero_rows(a, stream))) return rc;
  if (nreg > 0 && (rc = launch_embed_reg(a, unit_fast, nreg, stream))) return rc;                      // 1 .. FSW_REG_MAX_DEG = 32
  if (nlds > 0) {   // num_lds_rows bounds the rows of FSW_REG_MAX_DEG < degree <= FSW_LDS_MAX_DEG = 2048
    if (unit_fast) {
      if ((rc = launch_embed_mid_unit(a, nlds, stream))) return rc;                                    // 33 .. 256: one lane per slice
      if ((rc = launch_embed_ws_unit(a, nlds, stream))) return rc;                                     // 257 .. 2048: lines in registers
    } else {
      if ((rc = launch_embed_mid_weighted(a, nlds, stream))) return rc;                                // 33 .. 128: one lane per slice
      if (!a.efeat) {
        if ((rc = launch_embed_hub_weighted_lds(a, nlds, stream))) return rc;                          // 129 .. 2048: (key, weight) lines in registers
      } else if ((rc = launch_embed_wsort_lds(a, nlds, stream))) {                                     // 129 .. 2048: lines staged in LDS
        return rc;
      }
    }
  }
  if (nglob > 0) {   // num_global_rows bounds the rows above FSW_LDS_MAX_DEG
    if (unit_fast) {
      if ((rc = launch_embed_hub(a, nglob, stream))) return rc;                                        // 2049 .. FSW_HUB_MAX_DEG = 32768
      if ((rc = launch_embed_giant(a, nglob, stream))) return rc;                                      // above: sorted blocks + block sweeps
    } else if (!a.efeat) {
      if ((rc = launch_embed_hub_weighted_hub(a, nglob, stream))) return rc;                           // 2049 .. kHubWMaxDeg = 8191
      // above (of bin FSW_BIN_HUB0 + 1 only its rows of exactly 8192 neighbours are left): sorted blocks + merge-path levels
      if ((rc = launch_embed_mergepath_w(a, FSW_BIN_HUB0 + 1, FSW_BIN_GLOBAL, kHubWMaxDeg, nglob, stream))) return rc;
    } else if ((rc = launch_embed_wsort_global(a, nglob, stream))) {                                   // one scratch line per wavefront
      return rc;
    }
  }
  return 0;
}
