// Merge path for packed 64-bit words: the merge levels above one sorted run of the longest lines' backward.  gfx950.
// Caller: embed_giant_cart_bwd.hip (k_cart_giant_bwd).  The float lines of the forward: merge_path.h.
//
// The elements are the words of pack_key_index (sortnet.h): orderable key bits in the high half, entry index in the low half.  The
// words of one line are distinct, so ONE unsigned 64-bit compare is a total order, and that order is the project's rule for equal
// keys: equal keys keep entry order, the pad element (index D) sorts last among keys equal to 0, -0 = +0.  Ties cannot occur: the
// result does not depend on the merge algorithm, only on the words.
//
// A line of `total` words (a multiple of kMp64Run) lies in a scratch line as sorted runs of kMp64Run words (one wavefront's
// WaveLine64 sort).  Per level, runs of R words pair up into runs of 2 R:
//   1. one thread per tile boundary finds, by binary search along its diagonal of the (A, B) merge grid, how many words of A precede
//      output position d of its pair (mp64_boundary);
//   2. per tile of kMp64Tile = 256 threads x kMp64VT outputs: the A-part and the B-part the tile needs (together exactly kMp64Tile
//      words) are staged in LDS with coalesced loads (mp64_tile_src) while the loads of the next tile are in flight, every thread
//      splits the tile at its own diagonal (mp64_split_tile) and merges kMp64VT outputs serially out of LDS (mp64_merge_serial);
//   3. the outputs leave as 64 contiguous bytes per thread into the other line of the ping-pong.
// A run without a partner is copied (mp64_copy_run).  A workgroup-scope fence and a barrier separate the levels.
// The index arithmetic is written as FSW_HD helpers: tests/native/test_merge_path64.cpp runs the levels on the CPU, tile by tile and
// thread by thread, with the helpers the kernel calls.
#pragma once
#include <stdint.h>
#include "sortnet.h"

namespace fsw {

typedef unsigned long long mp64_t;

constexpr int kMp64NT = 256;                        // threads per workgroup
constexpr int kMp64VT = 8;                          // outputs per thread and tile: 64 bytes
constexpr int kMp64Tile = kMp64NT * kMp64VT;        // 2048 words = 16 KiB
constexpr int kMp64Run = 2048;                      // words of an initial sorted run
constexpr int kMp64Parts = 512;                     // tile boundaries held in LDS at a time
constexpr int kMp64TileLds = kMp64Tile + kMp64Tile / 8;   // words of LDS per staged tile (mp64_pad)
static_assert(kMp64Run % kMp64Tile == 0, "tiles must not straddle runs");

FSW_HD int mp64_min(int a, int b) { return a < b ? a : b; }
FSW_HD int mp64_max(int a, int b) { return a > b ? a : b; }

// LDS index of tile word i: one spare word per 8.  Thread t starts its serial merge near word 8 t; unpadded that is 16 banks apart
// (of 64 banks of 4 bytes): lanes t and t + 4 collide on every read.  With the spare word the stride is 18 banks: the 32 lanes of one
// pass of an 8-byte read fall into 32 different bank pairs.
FSW_HD int mp64_pad(int i) { return i + (i >> 3); }

// one level: runs of R words -> runs of 2 R
struct Mp64Level {
  int R;
  int nruns;            // >= 2
  int covered;          // words that belong to a pair of runs; the rest is one run without a partner
  int ntiles;           // covered / kMp64Tile
  unsigned pair_mask;   // 2 R - 1: a pair starts where a position has these bits clear
};
FSW_HD Mp64Level mp64_level(int total, int R) {
  Mp64Level l;
  l.R = R;
  l.nruns = (int)(((int64_t)total + R - 1) / R);
  const int64_t cov = (int64_t)(l.nruns >> 1) * 2 * R;
  l.covered = cov < (int64_t)total ? (int)cov : total;
  l.ntiles = l.covered / kMp64Tile;
  l.pair_mask = 2u * (unsigned)R - 1u;
  return l;
}

// words of A among the first d outputs of merge(A[0..nA), B[0..nB)).  0 <= d <= nA + nB.
FSW_HD int mp64_split(const mp64_t* A, int nA, const mp64_t* B, int nB, int d) {
  int lo = mp64_max(0, d - nB), hi = mp64_min(d, nA);
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (A[mid] < B[d - 1 - mid]) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// words of A before output position pos (a tile boundary) of the pair it lies in; 0 at the start of a pair and past the pairs
FSW_HD int mp64_boundary(const mp64_t* src, int total, const Mp64Level& l, int pos) {
  if (pos >= l.covered) return 0;
  const int pb = (int)((unsigned)pos & ~l.pair_mask), d = pos - pb;
  if (d == 0) return 0;
  return mp64_split(src + pb, l.R, src + pb + l.R, mp64_min(l.R, total - pb - l.R), d);
}

// tile `tile` of a level: start of its pair, its A-part [a0, a0 + na) of run A and its B-part [b0, b0 + kMp64Tile - na) of run B
struct Mp64TileGeo {
  int pos, pb, a0, b0, na;
};
// a0: mp64_boundary at the tile's start, a1_next: at its end (not read when the pair ends with this tile: all of A is before its end)
FSW_HD Mp64TileGeo mp64_tile_geo(int total, const Mp64Level& l, int tile, int a0, int a1_next) {
  Mp64TileGeo t;
  t.pos = tile * kMp64Tile;
  t.pb = (int)((unsigned)t.pos & ~l.pair_mask);
  const int d0 = t.pos - t.pb;
  const int nB = mp64_min(l.R, total - t.pb - l.R);
  const int a1 = (d0 + kMp64Tile >= l.R + nB) ? l.R : a1_next;
  t.a0 = a0;
  t.b0 = d0 - a0;
  t.na = a1 - a0;
  return t;
}
// where word e of the staged tile (A-part first, then B-part) lies in the source line
FSW_HD int mp64_tile_src(const Mp64TileGeo& t, int R, int e) { return e < t.na ? t.pb + t.a0 + e : t.pb + R + t.b0 + (e - t.na); }

// mp64_split on a staged tile: A = words 0 .. na - 1, B = words na .. na + nbb - 1 (padded indices)
FSW_HD int mp64_split_tile(const mp64_t* tk, int na, int nbb, int d) {
  int lo = mp64_max(0, d - nbb), hi = mp64_min(d, na);
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tk[mp64_pad(mid)] < tk[mp64_pad(na + d - 1 - mid)]) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// outputs dd .. dd + kMp64VT - 1 of the staged tile, given ia = mp64_split_tile(tk, na, nbb, dd)
FSW_HD void mp64_merge_serial(const mp64_t* tk, int na, int nbb, int dd, int ia, mp64_t* out) {
  int ib = dd - ia;
  mp64_t ka = tk[mp64_pad(mp64_min(ia, kMp64Tile - 1))], kb = tk[mp64_pad(mp64_min(na + ib, kMp64Tile - 1))];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < kMp64VT; ++j) {
    const bool ta = ia < na && (ib >= nbb || ka < kb);            // a word read past the end of its part is never compared
    out[j] = ta ? ka : kb;
    ia += ta ? 1 : 0;
    ib += ta ? 0 : 1;
    const mp64_t kn = tk[mp64_pad(mp64_min(ta ? ia : na + ib, kMp64Tile - 1))];   // the next word of the part that gave this output
    ka = ta ? kn : ka;
    kb = ta ? kb : kn;
  }
}

// a run without a partner moves on unchanged: thread tid's share, 16 bytes at a time (covered and total are even)
FSW_HD void mp64_copy_run(const mp64_t* src, mp64_t* dst, int covered, int total, int tid) {
  for (int e = covered + tid * 2; e < total; e += kMp64NT * 2) {
    const mp64_t x = src[e], y = src[e + 1];
    dst[e] = x;
    dst[e + 1] = y;
  }
}

// levels that merge total / kMp64Run runs into one (0 for one run)
FSW_HD int mp64_num_levels(int total) {
  int n = 0;
  for (int64_t R = kMp64Run; R < (int64_t)total; R <<= 1) ++n;
  return n;
}

#if defined(__HIPCC__)
// total / kMp64Run sorted runs in s0 -> one sorted line; s1: the second line of the ping-pong; returns the line that holds the result
// (s0 after an even number of levels).  tk: kMp64TileLds words of LDS, part: kMp64Parts + 1 ints.  Every thread of the workgroup
// (kMp64NT threads) calls it; the runs in s0 must be visible to the workgroup (fence + barrier) before, the result is after.
__device__ __forceinline__ mp64_t* merge_path64_levels(mp64_t* s0, mp64_t* s1, int total, mp64_t* tk, int* part) {
  const int tid = threadIdx.x;
  mp64_t *sk = s0, *dk = s1;
  for (int64_t R64 = kMp64Run; R64 < (int64_t)total; R64 <<= 1) {
    const Mp64Level lv = mp64_level(total, (int)R64);
    for (int g0 = 0; g0 < lv.ntiles; g0 += kMp64Parts) {
      const int cnt = mp64_min(kMp64Parts, lv.ntiles - g0);
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
        __syncthreads();                                          // the tile buffer (and, after the last tile, part) is overwritten next
      }
    }
    if (lv.nruns & 1) mp64_copy_run(sk, dk, lv.covered, total, tid);
    // the next level reads what other wavefronts of this workgroup wrote: workgroup scope is enough (one CU, one L1, stores
    // write through), an agent-scope fence would write back the XCD's L2
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __syncthreads();
    mp64_t* t = sk;
    sk = dk;
    dk = t;
  }
  return sk;
}
#endif

}  // namespace fsw
