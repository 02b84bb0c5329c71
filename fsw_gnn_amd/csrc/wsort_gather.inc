// Gather + transpose of one slice group, included INSIDE the loop over the slice groups of k_embed_wsort (embed_wsort.hip),
// k_embed_wsort_bwd (embed_wsort_bwd.hip) and k_embed_wsort_w_bwd (embed_w_sort_bwd.hip), ahead of the group's first barrier:
// tile[kk][t] = key of neighbour t < D at slice k0 + kk (the neighbour's row of Xp, + the edge-feature term), and 0 for t == D, the
// reference's pad element at x = 0 (Dtot = D + 1: general weights).  Consecutive threads take consecutive slices of one neighbour.
// kGatherDepth loads are issued before the first LDS store: the loop is otherwise one HBM round trip per iteration.  The tail is
// clamped: it reads the last element again and stores the same value; the slices past S - 1 of the last group read slice S - 1.
// In scope at the point of inclusion: tile, start, D, Dtot, k0, S, col, Xp, ldp and the compile-time constants M, SC and LINE
// (wsort_tile.h); with FSW_WS_GATHER_EDGE defined as 1 by the including file also efeat (nullptr: none), Ve, ldve and d_edge.
// Text and not a device function: as ws_gather_tile<M, SC>(tile, start, ...) every weighted instance of the forward and all nine
// instances of the backward came out longer (k_embed_wsort<64, true>: 25123 -> 25136 instructions, k_embed_wsort_bwd<4, false>:
// 2253 -> 2260).  The edge-feature term is add_edge_term (fsw_common.h) written out: as a call inside this text the same kernels keep
// their length and get another register allocation.  Included text leaves them instruction-identical (tools/compare_kernel_asm.py).
      constexpr int kGatherDepth = 8;
      const int total = Dtot * SC;
      for (int i0 = threadIdx.x; i0 < total; i0 += blockDim.x * kGatherDepth) {
        float key[kGatherDepth];
        int pos[kGatherDepth];
#pragma unroll
        for (int u = 0; u < kGatherDepth; ++u) {
          const int i = min(i0 + u * (int)blockDim.x, total - 1);
          const int kk = i % SC, t = i / SC;
          pos[u] = kk * LINE + t + t / M;
          key[u] = 0.f;
          if (t < D) {
            key[u] = Xp[(int64_t)col[start + t] * ldp + min(k0 + kk, S - 1)];
#if FSW_WS_GATHER_EDGE
            if (efeat) {
              const float* er = efeat + (int64_t)(start + t) * d_edge;
              const float* vr = Ve + (int64_t)min(k0 + kk, S - 1) * ldve;
              for (int q = 0; q < d_edge; ++q) key[u] = fmaf(er[q], vr[q], key[u]);
            }
#endif
          }
        }
#pragma unroll
        for (int u = 0; u < kGatherDepth; ++u) tile[pos[u]] = key[u];
      }
