// What the forward (embed_cart.hip, embed_cart_hub.hip, embed_cart_hub_w.hip, embed_giant_cart.hip, embed_split_cart.hip, embed_giant_cart_w.hip, embed_split_cart_w.hip) and the tuned backward (embed_cart_bwd.hip,
// embed_cart_hub_bwd.hip, embed_cart_hub_w_bwd.hip, embed_giant_cart_bwd.hip, embed_split_cart_bwd.hip, embed_split_cart_w_bwd.hip) of Cartesian mode share: the degree classes, the
// constant-address-space reads of wave-uniform tables, the row lookup of the split forms and the host helpers of the entry points and of
// the 13 launchers (the fill of a kernel's argument struct from fsw_cart_args, the plans of the split forms).  gfx950.
#pragma once
#include <algorithm>
#include "embed_launch.h"

namespace fsw {

constexpr int kCartRows = 64;                                 // rows per workgroup tile of the register path
constexpr int kCartMaxLine = 2048;                            // longest line of the wavefront path
constexpr int kCartLongM = kCartMaxLine / kWave;              // longer lines: elements per lane of a wavefront's chunk of kCartMaxLine
constexpr int kFB = 16;                                       // longer lines, forward: frequencies per synchronisation of the readout

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

// embed_cart.hip
int cart_check_common(const fsw_cart_args* c);                // the checks every Cartesian entry point starts with

// largest in-degree of degree bin b (include/fsw_hip.h; the last bin has none)
constexpr int bin_upper_degree(int b) {
  constexpr int sizes[FSW_NUM_MID_BINS] = FSW_MID_SIZES;
  if (b <= FSW_REG_MAX_DEG) return b;
  if (b < FSW_BIN_LDS0) return sizes[b - FSW_BIN_MID0];
  if (b < FSW_BIN_GLOBAL) return 512 << (b - FSW_BIN_LDS0);     // the LDS bins and the hub bins double from 512
  return 1 << 30;
}

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

// ---- the classes of the rows whose line is longer than kCartMaxLine elements: THE table (DESIGN.md prints it too) ---------------
// Everything that decides which rows a class takes reads it: the four launchers of embed_cart_hub*.hip, the three of embed_giant_cart*.hip
// and the scratch sizes (fsw_embed_cart_scratch_bytes, fsw_embed_cart_forward_scratch_bytes and
// fsw_embed_cart_backward_keys_scratch_bytes, which the host layer calls).
struct CartLongClass {
  int bin_lo, bin_hi;   // the degree bins its rows lie in
  int dlo, dhi;         // its rows: dlo < D <= dhi
  int nw;               // forward: one workgroup of nw wavefronts keeps the line in registers, kCartMaxLine elements per wavefront
  bool bwd_line;        // backward: one wavefront per line in a scratch line of cart_line_elems(longest such row of the bin) elements
};
struct CartLongMode {
  int pad;              // elements of a line next to the D neighbours: the pad element of general weights
  int num;              // classes
  CartLongClass cls[FSW_NUM_HUB_BINS];
  int generic_bin, generic_min_degree;   // the rows past the classes as the older scratch queries count them (fsw_embed_cart_scratch_bytes and the
                                         // two legacy size functions keep the values they had when these rows ran on the generic kernel)
  int giant_bin, giant_min_degree;       // rows of giant_min_degree neighbours and more (they begin in giant_bin): one workgroup per line in a
                                         // scratch line -- forward: sorted blocks (embed_giant_cart.hip: k_cart_giant, embed_giant_cart_w.hip:
                                         // k_cart_mergepath_w); backward: sorted runs + merge path (embed_giant_cart_bwd.hip: k_cart_giant_bwd)
  constexpr const CartLongClass& last() const { return cls[num - 1]; }
};
constexpr int kCartLastLdsBin = FSW_BIN_HUB0 - 1;             // rows of 1025 .. FSW_LDS_MAX_DEG neighbours
constexpr CartLongMode kCartLong[2] = {
    // unit weights (w == NULL and tau <= 1): lines of D keys, one class per hub bin
    {0, 4,
     {{FSW_BIN_HUB0, FSW_BIN_HUB0, 2048, 4096, 2, true},
      {FSW_BIN_HUB0 + 1, FSW_BIN_HUB0 + 1, 4096, 8192, 4, true},
      {FSW_BIN_HUB0 + 2, FSW_BIN_HUB0 + 2, 8192, 16384, 8, true},
      {FSW_BIN_HUB0 + 3, FSW_BIN_HUB0 + 3, 16384, 32768, 16, true}},
     FSW_BIN_GLOBAL, 32769, FSW_BIN_GLOBAL, 32769},
    // general weights (w != NULL or tau > 1): lines of D + 1 elements, so every class ends one neighbour below a bin's end
    {1, 3,
     {{kCartLastLdsBin, FSW_BIN_HUB0, 2047, 4095, 2, true},
      {FSW_BIN_HUB0, FSW_BIN_HUB0 + 1, 4095, 8191, 4, true},
      {FSW_BIN_HUB0 + 1, FSW_BIN_HUB0 + 2, 8191, 16383, 8, true}},
     FSW_BIN_HUB0 + 2, 16384, FSW_BIN_HUB0 + 2, 16384},
};
constexpr const CartLongMode& cart_long_mode(bool unit_fast) { return kCartLong[unit_fast ? 0 : 1]; }
inline bool cart_unit_fast(const fsw_cart_args* c) { return c->w == nullptr && c->tau <= 1.0; }

// The fields that every launcher copies from fsw_cart_args into its kernel's argument struct T, by name: the inputs (cart_fill_inputs_w:
// with w and tau, for the structs of general weights), the forward's outputs, the backward's gradients.  What else T holds (tables,
// scratch, the class's rows) is the launcher's.
template <class T>
void cart_fill_inputs(T& t, const fsw_cart_args* c) {
  t.rowptr = c->rowptr; t.col = c->col; t.perm = c->perm; t.bin_start = c->bin_start;
  t.Xp = (const float*)c->Xp; t.ldp = c->ldp; t.freqs = (const float*)c->freqs; t.S = c->S; t.F = c->F;
}
template <class T>
void cart_fill_inputs_w(T& t, const fsw_cart_args* c) {
  cart_fill_inputs(t, c);
  t.w = (const float*)c->w; t.tau = (float)c->tau;
}
template <class T>
void cart_fill_outputs(T& t, const fsw_cart_args* c) {
  t.out = (float*)c->out; t.ldo = c->ldo; t.bias = (const float*)c->bias; t.out_scale = (float)c->out_scale;
  t.has_mass = c->has_mass; t.mass_fn = c->mass_fn; t.mass_scale = (float)c->mass_scale;
}
template <class T>
void cart_fill_grads(T& t, const fsw_cart_args* c) {
  t.g = (const float*)c->g; t.ldg = c->ldg; t.gcol0 = c->has_mass; t.out_scale = (float)c->out_scale;
  t.gkey = (float*)c->gkey; t.ldk = c->ldk; t.gfreq = (float*)c->gfreq;
}

constexpr bool cart_long_table_ok(const CartLongMode& m, int max_line) {
  if (m.cls[0].dlo + m.pad != kCartMaxLine || m.last().dhi + m.pad != max_line) return false;   // from the wavefront path to max_line
  if (m.generic_min_degree != m.last().dhi + 1) return false;
  if (bin_upper_degree(m.generic_bin - 1) >= m.generic_min_degree || m.generic_min_degree > bin_upper_degree(m.generic_bin)) return false;
  if (m.giant_min_degree != m.last().dhi + 1) return false;                                     // neither direction leaves a row without a class
  if (m.giant_bin != m.generic_bin) return false;                                               // the older queries count the giant class's rows
  if (bin_upper_degree(m.giant_bin - 1) >= m.giant_min_degree || m.giant_min_degree > bin_upper_degree(m.giant_bin)) return false;
  for (int i = 0; i < m.num; ++i) {
    const CartLongClass& k = m.cls[i];
    if (k.nw != 2 << i || (i > 0 && k.dlo != m.cls[i - 1].dhi)) return false;                   // the launchers index by i
    if (k.dhi + m.pad != k.nw * kCartMaxLine) return false;                                    // the longest line fills the registers
    if (bin_upper_degree(k.bin_lo - 1) > k.dlo || k.dlo >= bin_upper_degree(k.bin_lo)) return false;    // D = dlo + 1 is in bin_lo
    if (bin_upper_degree(k.bin_hi - 1) >= k.dhi || k.dhi > bin_upper_degree(k.bin_hi)) return false;    // D = dhi is in bin_hi
  }
  return true;
}
static_assert(kCartMaxLine == FSW_LDS_MAX_DEG && bin_upper_degree(FSW_BIN_GLOBAL - 1) == FSW_HUB_MAX_DEG, "the bins of include/fsw_hip.h");
static_assert(cart_long_table_ok(kCartLong[0], FSW_HUB_MAX_DEG), "unit weights: the classes tile FSW_LDS_MAX_DEG < D <= FSW_HUB_MAX_DEG");
static_assert(cart_long_table_ok(kCartLong[1], FSW_CART_W_MAX_LINE), "general weights: the classes tile the lines up to FSW_CART_W_MAX_LINE");

// elements of the backward's scratch line for rows of up to `degree` neighbours
inline int64_t cart_line_elems(const CartLongMode& m, int64_t degree) { return (int64_t)pow2ceil((uint32_t)(degree + m.pad)); }
constexpr int kCartLineBytes = 12;                            // per element: the packed (key, index) word and the key gradient
constexpr int kCartLineMaxWaves = 2048;                       // resident wavefronts (one scratch line each) a launch uses at most

// forward grid: virtual blocks = (rows rounded up to 8) x slices (hub_line.h: hub_virtual_line), capped at 2^20 workgroups that stride
inline unsigned cart_hub_grid(int64_t rows, int S) { return (unsigned)std::min<int64_t>(ceil_div(rows, 8) * S * 8, 1ll << 20); }

// backward of the classes with bwd_line: fn(bin, line_elems, nwaves) launches a populated bin that can hold a row of them -- the scratch
// line sized by the bin's own longest such row, as many wavefronts as c->scratch holds lines (<= kCartLineMaxWaves, <= lines), >= 1
template <class Fn>
int for_each_cart_line_bin(const fsw_cart_args* c, const CartLongMode& m, Fn fn) {
  const int32_t* bs = c->bin_start_host;
  int done = -1;                                              // the last bin launched: consecutive classes may share one
  for (int i = 0; i < m.num; ++i) {
    if (!m.cls[i].bwd_line) continue;
    for (int bin = std::max(m.cls[i].bin_lo, done + 1); bin <= m.cls[i].bin_hi; done = bin++) {
      const int64_t rows = (int64_t)bs[bin + 1] - bs[bin];
      const int64_t bin_max = std::min<int64_t>({c->max_degree, bin_upper_degree(bin), m.last().dhi});
      if (rows <= 0 || bin_max <= m.cls[i].dlo) continue;
      FSW_REQUIRE(c->scratch && ((uintptr_t)c->scratch & 15) == 0,
                  "fsw_embed_cart_backward_keys_f32: rows of the long classes need a 16-byte aligned scratch buffer (fsw_embed_cart_scratch_bytes)");
      const int64_t line_elems = cart_line_elems(m, bin_max);
      const int64_t nwaves = std::min<int64_t>({(int64_t)(c->scratch_bytes / ((size_t)line_elems * kCartLineBytes)), kCartLineMaxWaves, rows * c->S});
      FSW_REQUIRE(nwaves >= 1, "fsw_embed_cart_backward_keys_f32: scratch buffer too small (need fsw_embed_cart_scratch_bytes)");
      fn(bin, line_elems, (int)nwaves);
      FSW_LAUNCH_CHECK();
    }
  }
  return 0;
}

// embed_cart_hub*.hip: the classes of kCartLong[0] (launch_cart_hub*) and of kCartLong[1] (launch_cart_hub_w*); the forward needs no scratch
int launch_cart_hub(const fsw_cart_args* c, hipStream_t stream), launch_cart_hub_bwd(const fsw_cart_args* c, hipStream_t stream);
int launch_cart_hub_w(const fsw_cart_args* c, hipStream_t stream), launch_cart_hub_w_bwd(const fsw_cart_args* c, hipStream_t stream);

// ---- forward of the giant class (rows of giant_min_degree neighbours and more): one workgroup per (row, slice) line, the line in sorted
// blocks in the workgroup's scratch line ------------------------------------------------------------------------------------------------
constexpr int kCartGiantNW = 16;                              // unit weights: wavefronts of a workgroup, kCartLongM keys per lane each
constexpr int kCartGiantBlk = kCartGiantNW * kCartMaxLine;    // unit weights: keys of a block (sorted in the workgroup's registers)
constexpr int kCartGiantWBlk = kCartLong[1].cls[1].dhi + kCartLong[1].pad;   // general weights: (key, weight) elements of a block: the longest
                                                              // line of the four-wavefront class (= merge_path.h: kMpBlk)
constexpr int kCartGiantMaxWg[2] = {256, 512};                // resident workgroups: one (130 KiB of LDS) / two (64 KiB) per CU of 256
static_assert(kCartGiantBlk == kCartLong[0].last().dhi && kCartLong[0].last().nw == kCartGiantNW && kCartLong[1].cls[1].nw == 4,
              "blocks: the longest line of the 16-wavefront unit class / of the four-wavefront general-weight class");

// bytes of one scratch line for rows of up to max_degree neighbours: the block-rounded line at 4 B per key (unit weights), four
// block-rounded float lines (general weights: keys and weights, ping and pong)
inline size_t cart_giant_line_bytes(const CartLongMode& m, int64_t max_degree) {
  const int64_t blk = m.pad ? kCartGiantWBlk : kCartGiantBlk;
  return (size_t)(ceil_div(max_degree + m.pad, blk) * blk) * sizeof(float) * (m.pad ? 4 : 1);
}
// workgroups of a launch over nlines lines out of a buffer that holds `held` scratch lines: a multiple of 8 from 8 on (one residue per XCD)
inline int64_t cart_giant_workgroups(const CartLongMode& m, int64_t held, int64_t nlines) {
  int64_t n = std::min<int64_t>({held, nlines, (int64_t)kCartGiantMaxWg[m.pad]});
  if (n >= 8) n &= ~(int64_t)7;
  return n;
}
// rows the giant class may hold: all from its first bin on.  The host knows the bins, not the degrees: general weights share that bin
// with the class below, whose rows are counted here and skipped by the kernel (workgroup-uniform `continue`)
inline int64_t cart_giant_rows(const fsw_cart_args* c, const CartLongMode& m) {
  return c->max_degree < m.giant_min_degree ? 0 : (int64_t)c->bin_start_host[FSW_NUM_BINS] - c->bin_start_host[m.giant_bin];
}
// embed_giant_cart.hip (kCartLong[0]) and embed_giant_cart_w.hip (kCartLong[1]); scratch: fsw_embed_cart_forward_scratch_bytes
int launch_cart_giant(const fsw_cart_args* c, hipStream_t stream);
int launch_cart_giant_w(const fsw_cart_args* c, hipStream_t stream);

// what the launchers of the giant class check before they launch: sets *nwg (0: nothing to launch) and *line_bytes
inline int cart_giant_plan(const fsw_cart_args* c, const CartLongMode& m, int64_t* nwg, size_t* line_bytes) {
  *nwg = 0;
  const int64_t rows = (int64_t)c->bin_start_host[FSW_NUM_BINS] - c->bin_start_host[m.giant_bin];
  if (rows <= 0 || (c->max_degree > 0 && c->max_degree < m.giant_min_degree)) return 0;
  FSW_REQUIRE(c->max_degree >= m.giant_min_degree, "fsw_embed_cart_f32: max_degree (host value) is required for the rows of the longest class");
  FSW_REQUIRE(c->scratch && ((uintptr_t)c->scratch & 15) == 0,
              "fsw_embed_cart_f32: rows of the longest class need a 16-byte aligned scratch buffer (fsw_embed_cart_forward_scratch_bytes)");
  *line_bytes = cart_giant_line_bytes(m, c->max_degree);
  *nwg = cart_giant_workgroups(m, (int64_t)(c->scratch_bytes / *line_bytes), rows * c->S);
  FSW_REQUIRE(*nwg >= 1, "fsw_embed_cart_f32: scratch buffer too small for one line (need fsw_embed_cart_forward_scratch_bytes)");
  return 0;
}

// ---- what the four split plans below start with (host values only: bin_start_host, max_degree, w, tau, S, F).  lines == 0, no split
// form for this call: no arguments, the other weight mode, no row of the giant class, or regions above 2 GiB (kCartSplitCap: as
// fsw_embed_cart_forward_scratch_bytes and fsw_embed_cart_backward_keys_scratch_bytes) ----------------------------------------------
constexpr size_t kCartSplitCap = (size_t)2 << 30;
constexpr size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
struct CartSplitBase {
  int64_t rows, lines;                                        // rows from the giant class's first bin on; x S
  size_t line_bytes;                                          // of one line's regions: line_bytes_of(mode, max_degree)
};
inline CartSplitBase cart_split_base(const fsw_cart_args* c, bool unit, size_t (*line_bytes_of)(const CartLongMode&, int64_t)) {
  CartSplitBase b = {};
  if (!c || !c->bin_start_host || cart_unit_fast(c) != unit || c->S < 1 || c->F < 1) return b;
  const CartLongMode& m = cart_long_mode(unit);
  const int64_t rows = cart_giant_rows(c, m);
  if (rows <= 0) return b;
  const size_t line_bytes = line_bytes_of(m, c->max_degree);
  const int64_t lines = rows * c->S;
  if (line_bytes > kCartSplitCap || (size_t)lines > kCartSplitCap / line_bytes) return b;
  b.rows = rows; b.lines = lines; b.line_bytes = line_bytes;
  return b;
}

// The row at position p of perm as the kernels of the four split forms look it up: l.node, l.start, l.D.  What a form needs on top (the
// slice, the line's blocks or runs, the skip rule against ITS line size) is its own
template <class A, class L>
__device__ __forceinline__ void cart_row_at(const A& a, int p, L& l) {
  l.node = a.perm[p];
  l.start = a.rowptr[l.node];
  l.D = a.rowptr[l.node + 1] - l.start;
}

// ---- split form of the giant class's forward, unit weights (embed_split_cart.hip; args->flags & FSW_CART_SPLIT_LINES): every phase of
// k_cart_giant is a launch of its own over (line, block), so one long line keeps many workgroups busy.  Every line owns a scratch
// region of line_bytes; the per-block partial sums [lines][nbmax][F] follow the regions -------------------------------------------------
constexpr int64_t kCartSplitMaxLines = 128;                   // fsw_embed_cart_split_max_lines: the largest measured line count, and the split form won there
struct CartSplitPlan {
  int64_t lines;                                              // rows from the giant class's first bin on x S; 0: no split form for this call
  size_t line_bytes;                                          // cart_giant_line_bytes: nbmax blocks of kCartGiantBlk keys
  int nbmax;                                                  // blocks of the longest line
  size_t partial_offset;                                      // bytes: where the partial sums begin (16-byte aligned)
  size_t bytes;                                               // fsw_embed_cart_split_scratch_bytes
};
inline CartSplitPlan cart_split_plan(const fsw_cart_args* c) {
  CartSplitPlan p = {};
  const CartSplitBase b = cart_split_base(c, true, cart_giant_line_bytes);
  if (b.lines <= 0) return p;
  const int64_t nbmax = (int64_t)(b.line_bytes / (kCartGiantBlk * sizeof(float)));
  const size_t offset = up16((size_t)b.lines * b.line_bytes);
  const size_t partial = (size_t)b.lines * (size_t)nbmax * (size_t)c->F * sizeof(float);   // lines * nbmax <= 2^14, F < 2^31
  if (offset + partial > kCartSplitCap) return p;
  p.lines = b.lines; p.line_bytes = b.line_bytes; p.nbmax = (int)nbmax; p.partial_offset = offset; p.bytes = offset + partial;
  return p;
}
// embed_split_cart.hip: the giant class of kCartLong[0] in the split form, out of c->scratch (>= p.bytes, 16-byte aligned: checked by the caller)
int launch_cart_split(const fsw_cart_args* c, const CartSplitPlan& p, hipStream_t stream);

// ---- split form of the giant class's forward, general weights (embed_split_cart_w.hip; args->flags & FSW_CART_SPLIT_W_LINES): every
// phase of k_cart_mergepath_w is a launch of its own over (line, piece).  Every line owns four block-rounded float lines (keys and
// weights, ping and pong: cart_giant_line_bytes); behind the regions follow the float64 sums of the weights of every tile of
// kCartSplitWTile ranks [lines][tiles], the per-tile partial sums [lines][tiles][F] and the float64 partial sums of the rows' masses
// [rows][nbmax], every part 16-byte aligned -------------------------------------------------------------------------------------------
constexpr int kCartSplitWTile = kCartGiantWBlk / 2;           // ranks of a tile of the levels and of the readout: half a block (= merge_path.h: kMpTile)
constexpr int64_t kCartSplitWMaxLines = 256;                  // fsw_embed_cart_split_w_max_lines: the largest measured line count at which the split form won
static_assert(kCartGiantWBlk % kCartSplitWTile == 0, "tiles must not straddle blocks");
struct CartSplitWPlan {
  int64_t lines;                                              // rows from the giant class's first bin on x S; 0: no split form for this call
  int64_t rows;                                               // lines / S
  int64_t cap;                                                // elements of each of a line's four float lines: nbmax blocks of kCartGiantWBlk
  int nbmax, tiles;                                           // blocks / tiles of the longest line
  size_t tsum_offset, partial_offset, mass_offset;            // bytes: where the tile sums, the partial sums and the mass pieces begin
  size_t bytes;                                               // fsw_embed_cart_split_w_scratch_bytes
};
inline CartSplitWPlan cart_split_w_plan(const fsw_cart_args* c) {
  CartSplitWPlan p = {};
  const CartSplitBase b = cart_split_base(c, false, cart_giant_line_bytes);
  if (b.lines <= 0) return p;
  const size_t cap = kCartSplitCap, lines = (size_t)b.lines;
  const int64_t elems = (int64_t)(b.line_bytes / (4 * sizeof(float)));
  const int64_t nbmax = elems / kCartGiantWBlk, tiles = elems / kCartSplitWTile;
  const size_t regions = lines * b.line_bytes;                 // a multiple of 16
  const size_t tsum = up16(lines * (size_t)tiles * sizeof(double));                      // lines * tiles <= 2^15
  if ((size_t)c->F > cap / (lines * (size_t)tiles * sizeof(float))) return p;
  const size_t partial = up16(lines * (size_t)tiles * (size_t)c->F * sizeof(float));
  const size_t mass = up16((size_t)b.rows * (size_t)nbmax * sizeof(double));
  if (regions + tsum + partial + mass > cap) return p;
  p.lines = b.lines; p.rows = b.rows; p.cap = elems; p.nbmax = (int)nbmax; p.tiles = (int)tiles;
  p.tsum_offset = regions; p.partial_offset = regions + tsum; p.mass_offset = regions + tsum + partial;
  p.bytes = regions + tsum + partial + mass;
  return p;
}
// embed_split_cart_w.hip: the giant class of kCartLong[1] in the split form, out of c->scratch (>= p.bytes, 16-byte aligned: checked by the caller)
int launch_cart_split_w(const fsw_cart_args* c, const CartSplitWPlan& p, hipStream_t stream);

// ---- backward of the giant class: one workgroup of four wavefronts per (row, slice) line; the line as packed (key, entry index) words
// in sorted runs of kCartMaxLine (one wavefront's chunk), merged by merge path (merge_path64.h) between two scratch lines -------------
constexpr int kCartGiantBwdElemBytes = 16;                    // per word of the line: ping and pong; the key gradients pass through the one
                                                              // that the last level leaves free
constexpr int kCartGiantBwdMaxWg[2] = {512, 512};             // resident workgroups: two (20.5 KiB of LDS, <= 256 registers) per CU of 256
// bytes of one scratch line for rows of up to max_degree neighbours: the line rounded up to whole runs
inline size_t cart_giant_bwd_line_bytes(const CartLongMode& m, int64_t max_degree) {
  return (size_t)(ceil_div(max_degree + m.pad, kCartMaxLine) * kCartMaxLine) * kCartGiantBwdElemBytes;
}
// workgroups of a launch over nlines lines out of a buffer that holds `held` scratch lines: a multiple of 8 from 8 on (one residue per XCD)
inline int64_t cart_giant_bwd_workgroups(const CartLongMode& m, int64_t held, int64_t nlines) {
  int64_t n = std::min<int64_t>({held, nlines, (int64_t)kCartGiantBwdMaxWg[m.pad]});
  if (n >= 8) n &= ~(int64_t)7;
  return n;
}
// embed_giant_cart_bwd.hip: the giant class of the call's mode out of c->scratch (fsw_embed_cart_backward_keys_scratch_bytes)
int launch_cart_giant_bwd(const fsw_cart_args* c, hipStream_t stream);

// a buffer for `lines` scratch lines of the classes with bwd_line: at most kCartLineMaxWaves of them and 2 GiB (fewer wavefronts then
// share the work), at least one
inline size_t cart_line_buffer_bytes(int64_t line_elems, int64_t lines) {
  const size_t line_bytes = (size_t)line_elems * kCartLineBytes;
  const size_t cap = (size_t)2 << 30;                            // as embed_global_scratch_bytes
  const size_t waves = std::min<size_t>((size_t)std::min<int64_t>(lines, kCartLineMaxWaves), cap / line_bytes);
  return std::max<size_t>(waves, 1) * line_bytes;
}
// what the backward of the classes with bwd_line needs (for_each_cart_line_bin); 0 when it launches none: no row that long, or unit
// weights without a row in the class bins.  Host values only
inline size_t cart_line_classes_bwd_bytes(const fsw_cart_args* c, const CartLongMode& m) {
  const int32_t* bs = c->bin_start_host;
  if (c->max_degree <= m.cls[0].dlo || (m.pad == 0 && bs[m.last().bin_hi + 1] == bs[m.cls[0].bin_lo])) return 0;
  const int64_t rows = std::max<int64_t>((int64_t)bs[FSW_NUM_BINS] - bs[m.cls[0].bin_lo], 1);
  return cart_line_buffer_bytes(cart_line_elems(m, std::min<int64_t>(c->max_degree, m.last().dhi)), rows * std::max<int32_t>(c->S, 1));
}

// ---- split form of the giant class's backward, unit weights (embed_split_cart_bwd.hip; args->flags & FSW_CART_SPLIT_BWD_LINES): every
// phase of k_cart_giant_bwd<false> is a launch of its own over (line, piece).  Every line owns a scratch region of line_bytes (ping and
// pong, cart_giant_bwd_line_bytes); the per-tile partial sums of the frequency gradients [lines][ntmax][F] follow the regions ----------
constexpr int kCartSplitBwdWalk = 256 * 16;                   // ranks of a tile of the walk: 256 threads x kGbVT[0] of k_cart_giant_bwd
constexpr int64_t kCartSplitBwdMaxLines = 128;                // fsw_embed_cart_split_backward_max_lines: the largest measured line count at which the split form won
struct CartSplitBwdPlan {
  int64_t lines;                                              // rows from the giant class's first bin on x S; 0: no split form for this call
  size_t line_bytes;                                          // cart_giant_bwd_line_bytes: two lines of whole runs
  int ntmax;                                                  // walk tiles of the longest line
  size_t partial_offset;                                      // bytes: where the partial sums begin (16-byte aligned)
  size_t bytes;                                               // fsw_embed_cart_split_backward_scratch_bytes: the rows of the other classes included
};
inline CartSplitBwdPlan cart_split_bwd_plan(const fsw_cart_args* c) {
  CartSplitBwdPlan p = {};
  const CartSplitBase b = cart_split_base(c, true, cart_giant_bwd_line_bytes);
  if (b.lines <= 0) return p;
  const int64_t ntmax = ceil_div(c->max_degree, (int64_t)kCartSplitBwdWalk);
  const size_t offset = (size_t)b.lines * b.line_bytes;        // a multiple of 16
  const size_t partial = up16((size_t)b.lines * (size_t)ntmax * (size_t)c->F * sizeof(float));   // lines * ntmax < 2^16, F < 2^31
  if (offset + partial > kCartSplitCap) return p;
  p.lines = b.lines; p.line_bytes = b.line_bytes; p.ntmax = (int)ntmax; p.partial_offset = offset;
  p.bytes = std::max(offset + partial, cart_line_classes_bwd_bytes(c, kCartLong[0]));
  return p;
}
// embed_split_cart_bwd.hip: the giant class of kCartLong[0] in the split form, out of c->scratch (>= p.bytes, 16-byte aligned: checked by the caller)
int launch_cart_split_bwd(const fsw_cart_args* c, const CartSplitBwdPlan& p, hipStream_t stream);

// ---- split form of the giant class's backward, general weights (embed_split_cart_w_bwd.hip; args->flags & FSW_CART_SPLIT_W_BWD_LINES):
// every phase of k_cart_giant_bwd<true> is a launch of its own over (line, piece).  Every line owns two regions (ping and pong) of `words`
// packed words: the line of max_degree + 1 elements rounded up to whole runs; behind the regions follow the float64 mass pieces of the
// rows [rows][tiles], the float64 sums of the weights of every walk tile [lines][tiles] and the per-tile partial sums of the frequency
// gradients [lines][tiles][F], every part 16-byte aligned ------------------------------------------------------------------------------
constexpr int kCartSplitWBwdWalk = 256 * 8;                   // ranks of a tile of the walk: 256 threads x kGbVT[1] of k_cart_giant_bwd = one run
constexpr int64_t kCartSplitWBwdMaxLines = 256;               // fsw_embed_cart_split_w_backward_max_lines: the largest measured line count at which the split form won
static_assert(kCartSplitWBwdWalk == kCartMaxLine, "a walk tile is one run: the mass pieces, the tile sums and the partial sums share `tiles`");
struct CartSplitWBwdPlan {
  int64_t lines;                                              // rows from the giant class's first bin on x S; 0: no split form for this call
  int64_t rows;                                               // lines / S
  int64_t words;                                              // words of each of a line's two regions: (max_degree + 1) in whole runs
  int tiles;                                                  // runs = walk tiles of the longest line
  size_t mass_offset, tsum_offset, partial_offset;            // bytes: where the mass pieces, the tile sums and the partial sums begin
  size_t bytes;                                               // fsw_embed_cart_split_w_backward_scratch_bytes: the rows of the classes below included
};
inline CartSplitWBwdPlan cart_split_w_bwd_plan(const fsw_cart_args* c) {
  CartSplitWBwdPlan p = {};
  const CartSplitBase b = cart_split_base(c, false, cart_giant_bwd_line_bytes);
  if (b.lines <= 0) return p;
  const size_t cap = kCartSplitCap, lines = (size_t)b.lines;
  const int64_t words = (int64_t)(b.line_bytes / kCartGiantBwdElemBytes), tiles = words / kCartSplitWBwdWalk;
  const size_t regions = lines * b.line_bytes;                 // a multiple of 16
  const size_t mass = up16((size_t)b.rows * (size_t)tiles * sizeof(double));             // lines * tiles <= 2^16
  const size_t tsum = up16(lines * (size_t)tiles * sizeof(double));
  if ((size_t)c->F > cap / (lines * (size_t)tiles * sizeof(float))) return p;
  const size_t partial = up16(lines * (size_t)tiles * (size_t)c->F * sizeof(float));
  if (regions + mass + tsum + partial > cap) return p;
  p.lines = b.lines; p.rows = b.rows; p.words = words; p.tiles = (int)tiles;
  p.mass_offset = regions; p.tsum_offset = regions + mass; p.partial_offset = regions + mass + tsum;
  p.bytes = std::max(regions + mass + tsum + partial, cart_line_classes_bwd_bytes(c, kCartLong[1]));
  return p;
}
// embed_split_cart_w_bwd.hip: the giant class of kCartLong[1] in the split form, out of c->scratch (>= p.bytes, 16-byte aligned: checked by the caller)
int launch_cart_split_w_bwd(const fsw_cart_args* c, const CartSplitWBwdPlan& p, hipStream_t stream);

}  // namespace fsw
