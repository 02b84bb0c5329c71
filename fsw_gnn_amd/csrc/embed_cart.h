// What the forward (embed_cart.hip) and the tuned backward (embed_cart_bwd.hip) of Cartesian mode share: the degree classes, the
// constant-address-space reads of wave-uniform tables and the host helpers of the entry points.  gfx950.
#pragma once
#include "fsw_common.h"

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
// k_embed_cart_generic (float32 storage) on rows[0 .. num_rows - 1] of at least min_deg neighbours; forward or, with c->g, backward
int launch_cart_generic_f32(const fsw_cart_args* c, const int32_t* rows, int64_t num_rows, int min_deg, hipStream_t stream);

}  // namespace fsw
