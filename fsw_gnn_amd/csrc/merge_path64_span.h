// Merge path for packed 64-bit words, one level as a launch of its own: which part of a level a workgroup takes when the levels of
// merge_path64.h run over many workgroups per line.  gfx950.  Caller: embed_split_cart_bwd.hip (k_split_bwd_level).
//
// A line of `total` words has total / kMp64Tile tile slots at every level: the first lv.ntiles are output tiles of paired runs, the
// rest is the run without a partner, which moves on unchanged.  A workgroup takes a span of `span` consecutive slots: it finds the
// boundaries of its own merge tiles (mp64_boundary: span + 1 binary searches in the level's SOURCE line), merges them into the other
// line and copies its share of the run without a partner.  It reads the source line only and writes its own slots of the destination
// only, so the workgroups of a level need no order among themselves; consecutive launches order the levels.
// tests/native/test_split_bwd_levels.cpp runs the levels on the CPU with these helpers, the spans of a level in reversed and shuffled order.
#pragma once
#include "merge_path64.h"

namespace fsw {

constexpr int kMp64MaxSpan = 16;                    // tile slots a workgroup takes at most: boundaries held in LDS

struct Mp64Span {
  int t0, nt;           // merge tiles t0 .. t0 + nt - 1 of the level
  int c0, c1;           // words [c0, c1) of the run without a partner
};
// span sp of a line of `total` words at level lv; false: the span lies past the line
FSW_HD bool mp64_span(int total, const Mp64Level& lv, int span, int sp, Mp64Span& s) {
  const int slots = total / kMp64Tile;
  const int64_t b64 = (int64_t)sp * span;
  if (b64 >= (int64_t)slots) return false;
  const int b = (int)b64, e = mp64_min(b + span, slots);
  s.t0 = mp64_min(b, lv.ntiles);
  s.nt = mp64_min(e, lv.ntiles) - s.t0;
  s.c0 = mp64_max(b, lv.ntiles) * kMp64Tile;
  s.c1 = mp64_max(e, lv.ntiles) * kMp64Tile;
  return true;
}
// spans that cover a line of `total` words
FSW_HD int mp64_num_spans(int total, int span) { return (total / kMp64Tile + span - 1) / span; }
// run length of level k = 0, 1, ..; a level of the line while it is below `total`
FSW_HD int64_t mp64_level_run(int k) { return (int64_t)kMp64Run << k; }

#if defined(__HIPCC__)
// tiles g0 .. g0 + cnt - 1 (1 <= cnt <= kMp64MaxSpan) of level lv from sk into dk: the tile loop of merge_path64_levels.  (That loop
// stays written out in merge_path64.h: calling this function from there changes the code k_cart_giant_bwd compiles to.)
// tk: kMp64TileLds words of LDS, part: cnt + 1 ints.  Every thread of the workgroup (kMp64NT threads) calls it.
__device__ __forceinline__ void mp64_merge_tiles(const mp64_t* sk, mp64_t* dk, int total, const Mp64Level& lv, int g0, int cnt, mp64_t* tk,
                                                 int* part) {
  const int tid = threadIdx.x;
  for (int i = tid; i <= cnt; i += kMp64NT) part[i] = mp64_boundary(sk, total, lv, (g0 + i) * kMp64Tile);
  __syncthreads();
  // the tile's words, word tid + u * 256 in register u: the loads of tile i + 1 are issued before tile i is merged out of LDS
  mp64_t pk[kMp64VT];
  auto fetch = [&](const Mp64TileGeo& t) {
#pragma unroll
    for (int u = 0; u < kMp64VT; ++u) pk[u] = sk[mp64_tile_src(t, lv.R, tid + u * kMp64NT)];
  };
  fetch(mp64_tile_geo(total, lv, g0, part[0], part[1]));
  for (int i = 0; i < cnt; ++i) {
    const Mp64TileGeo g = mp64_tile_geo(total, lv, g0 + i, part[i], part[i + 1]);
#pragma unroll
    for (int u = 0; u < kMp64VT; ++u) tk[mp64_pad(tid + u * kMp64NT)] = pk[u];
    __syncthreads();
    if (i + 1 < cnt) fetch(mp64_tile_geo(total, lv, g0 + i + 1, part[i + 1], part[i + 2]));
    const int dd = tid * kMp64VT;
    mp64_t ok[kMp64VT];
    mp64_merge_serial(tk, g.na, kMp64Tile - g.na, dd, mp64_split_tile(tk, g.na, kMp64Tile - g.na, dd), ok);
    ulonglong2* o2 = reinterpret_cast<ulonglong2*>(dk + g.pos + dd);
#pragma unroll
    for (int j = 0; j < kMp64VT; j += 2) o2[j >> 1] = make_ulonglong2(ok[j], ok[j + 1]);
    if (i + 1 < cnt) __syncthreads();                             // the tile buffer is overwritten by the next tile
  }
}
#endif

}  // namespace fsw
