// What the forward (embed_cart.hip, embed_cart_hub.hip, embed_cart_hub_w.hip) and the tuned backward (embed_cart_bwd.hip,
// embed_cart_hub_bwd.hip, embed_cart_hub_w_bwd.hip) of Cartesian mode share: the degree classes, the
// constant-address-space reads of wave-uniform tables and the host helpers of the entry points.  gfx950.
#pragma once
#include <algorithm>
#include "embed_launch.h"

namespace fsw {

constexpr int kCartRows = 64;                                 // rows per workgroup tile of the register path
constexpr int kCartMaxLine = 2048;                            // longest line of the wavefront path

// Read-only inputs at wave-uniform addresses (coefficient table, frequencies) are read through the constant address space: the
// compiler then issues scalar loads (s_load_dwordx4).  Through a generic pointer it must assume that the output stores may alias
// them, and every coefficient becomes a vector-memory load next to the gathers.
#if defined(__HIP_DEVICE_COMPILE__)
template <class T>
using ConstAS = const __attribute__((address_space(4))) T;
#else
template <class T>
using ConstAS = const T;   // host pass of the same source: no address spaces
#endif
template <class T>
__device__ __forceinline__ ConstAS<T>* as_const(const T* p) { return (ConstAS<T>*)p; }

#define FSW_CART_CASES_1_32(X)                                                                                         \
  X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19) X(20) X(21) \
  X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30) X(31) X(32)

// embed_cart.hip
int cart_check_common(const fsw_cart_args* c);                // the checks every Cartesian entry point starts with
int bin_upper_degree(int b);                                  // largest in-degree of degree bin b

// The degree bins of 33 .. 2048 neighbours (bin_start_host bs) in groups of consecutive bins whose lines (extra = 1: + the pad
// element of general weights) need the same number Mb of keys per lane of a wavefront: fn(Mb, p0, rows) for the rows
// perm[p0 .. p0 + rows - 1] of every group, until one returns an error code.
template <class Fn>
int for_each_wave_group(const int32_t* bs, int extra, Fn fn) {
  auto keys_per_lane = [&](int b) { return (int)std::min<uint32_t>(32, pow2ceil((uint32_t)ceil_div(bin_upper_degree(b) + extra, kWave))); };
  for (int b = FSW_BIN_MID0; b < FSW_BIN_HUB0;) {
    const int Mb = keys_per_lane(b);
    int e = b + 1;                                            // one past the group's last bin
    while (e < FSW_BIN_HUB0 && keys_per_lane(e) == Mb) ++e;
    if (const int rc = fn(Mb, bs[b], bs[e] - bs[b])) return rc;
    b = e;
  }
  return 0;
}

// embed_cart_hub.hip / embed_cart_hub_bwd.hip: unit weights with tau <= 1, the rows of the hub bins (FSW_LDS_MAX_DEG < D <= FSW_HUB_MAX_DEG)
int launch_cart_hub(const fsw_cart_args* c, hipStream_t stream);        // forward, no scratch
int launch_cart_hub_bwd(const fsw_cart_args* c, hipStream_t stream);    // backward, c->scratch: fsw_embed_cart_backward_scratch_bytes

// embed_cart_hub_w.hip / embed_cart_hub_w_bwd.hip: general weights (w != NULL or tau > 1), the lines of kCartMaxLine + 1 ..
// FSW_CART_W_MAX_LINE elements (FSW_LDS_MAX_DEG <= D < FSW_CART_W_MAX_LINE: the last LDS bin and the first three hub bins)
int launch_cart_hub_w(const fsw_cart_args* c, hipStream_t stream);      // forward, no scratch
int launch_cart_hub_w_bwd(const fsw_cart_args* c, hipStream_t stream);  // backward, c->scratch: fsw_embed_cart_weighted_backward_scratch_bytes

// Lines the tuned classes do not take (float32 storage): the generic kernel, forward or, with c->g, backward.  unit_fast == false
// (general weights; extra = 1, the pad element): the lines above FSW_CART_W_MAX_LINE elements, on the rows of the third hub bin (which
// holds D = FSW_CART_W_MAX_LINE) and above; unit_fast == true (unit weights with tau <= 1; extra = 0): only the rows of FSW_BIN_GLOBAL.
inline int launch_cart_long_rows(const fsw_cart_args* c, int extra, bool unit_fast, hipStream_t stream) {
  const int min_long = unit_fast ? FSW_HUB_MAX_DEG + 1 : FSW_CART_W_MAX_LINE + 1 - extra;
  const int32_t* bs = c->bin_start_host;
  const int p0 = unit_fast ? bs[FSW_BIN_GLOBAL] : bs[FSW_BIN_HUB0 + 2];
  const int64_t rows = (int64_t)bs[FSW_NUM_BINS] - p0;
  if (c->max_degree < min_long || rows <= 0) return 0;
  return launch_embed_generic(generic_args(*c, true, c->F), 0, c->perm + p0, rows, min_long, stream);
}

}  // namespace fsw
