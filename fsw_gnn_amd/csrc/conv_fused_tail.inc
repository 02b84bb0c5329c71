// Phases 2 and 3 of a fused tile, included INSIDE the body of k_conv_fused_unit and of k_conv_fused_cart (conv_fused.hip) once phase 1
// has left the tile's embedding rows in H: H . W1^T on the matrix cores, + Yin / bias, activation, rows of Y stored by node id.
// It starts with the barrier that ends phase 1 and ends the kernel.  In scope at the point of inclusion: a (FusedArgs), smem, H,
// nodeS, p, nrows, wv, lane, fr, fh and the compile-time constants ABL and TR.
// Text and not a device function: as an inlined function the same statements get another register allocation in all three
// k_conv_fused_unit instantiations (110 -> 123 VGPRs; by reference or by value, with or without the early return), and those
// kernels are the headline of bench.py.  Included text leaves them instruction-identical (tools/compare_kernel_asm.py).
  const int nslabs = (a.Hout + 31) / 32;
  if (nslabs <= 4) {
    // ---- Hout <= 128: one slab per wave, output tile staged through LDS so that Y is written as whole rows ----
    // Rows of Yin (= x . W2^T + b, stored by the projection kernel in perm order: this workgroup's 32 rows are one
    // contiguous run).  Wave w finishes rows 8w..8w+7; lane owns columns lane and lane+64.  Issued after phase 1
    // (registers are free again) and before the barrier: in flight while the other waves finish their rows.
    // Branch-free (rows past the tile's end re-read its last row, columns past Hout the last column; neither is used): with a
    // branch per load every load sat in its own basic block and waited for the one before it (s_waitcnt vmcnt(0) per block) --
    // 10 us of a workgroup's 91 (tools/exp_fused_stamps.py)
    float lb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) lb[h] = (!a.Yin && a.lin_bias && lane + 64 * h < a.Hout) ? a.lin_bias[lane + 64 * h] : 0.f;
    // TR == 32: the staging tile reuses H; TR == 128: its own LDS behind the node ids (four sub-tiles read H one after the other)
    float* T = TR == kFusedRows ? smem : reinterpret_cast<float*>(nodeS + TR);   // [32][kLdT]
#pragma unroll 1
    for (int r0 = 0; r0 < TR; r0 += kFusedRows) {
      if (TR > kFusedRows && r0 >= nrows) break;           // uniform
      const int nsub = min(nrows - r0, kFusedRows);
      float yin[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) yin[q] = 0.f;
      if ((ABL & 2) == 0 && a.Yin) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = r0 + min(wv * 8 + (q >> 1), nsub - 1), c = min(lane + 64 * (q & 1), a.Hout - 1);
          yin[q] = a.Yin[(int64_t)(a.yin_by_node ? a.perm[p + row] : p + row) * a.ldyin + c];
        }
      }
      FSW_FSTAMP(2);                                       // Yin loads issued
      __syncthreads();                       // first sub-tile: phase 1 complete; later ones: the previous epilogue has read T
      FSW_FSTAMP(3);                                       // barrier: waited for the slowest wavefront's phase 1
      f32x16 acc;
      if (wv < nslabs) slab_mma<ABL>(a, H + r0 * a.ldh, wv, fr, fh, acc);
      FSW_FSTAMP(4);                                       // matrix phase
      if (TR == kFusedRows) __syncthreads(); // every wave has finished reading H: reuse it for the output tile
      if (wv < nslabs) {
#pragma unroll
        for (int r = 0; r < 16; ++r) T[((r & 3) + 8 * (r >> 2) + 4 * fh) * kLdT + wv * 32 + fr] = acc[r];
      }
      __syncthreads();
      FSW_FSTAMP(5);                                       // barrier, accumulators into the staging tile, barrier
#pragma unroll
      for (int rr = 0; rr < 8; ++rr) {
        const int row = wv * 8 + rr;
        const int node = row < nsub ? nodeS[r0 + row] : -1;
        if (node < 0) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int c = lane + 64 * h;
          if (c < a.Hout) {
            float y = T[row * kLdT + c] + lb[h] + yin[rr * 2 + h];
            if (a.act == 1) y = fmaxf(y, 0.f);
            else if (a.act == 2) y = y >= 0.f ? y : a.slope * y;
            if ((ABL & 4) == 0 || y == 12345.f) a.Y[(int64_t)node * a.ldy + c] = y;
          }
        }
      }
    }
    FSW_FSTAMP(6);                                         // epilogue: + Yin, activation, Y rows stored
    return;
  }

  // ---- wide layers (Hout > 128): slabs round-robin over the waves, every wave stores its own 32 x 32 tiles ----
  __syncthreads();
  for (int slab = wv; slab < nslabs; slab += 4) {
    const int j = slab * 32 + fr;
    float yin[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * fh;     // C/D map of the 32x32 MFMA
      yin[r] = (a.Yin && row < nrows && j < a.Hout) ? a.Yin[(int64_t)(a.yin_by_node ? a.perm[p + row] : p + row) * a.ldyin + j] : 0.f;
    }
    f32x16 acc;
    slab_mma<ABL>(a, H, slab, fr, fh, acc);
    if (j < a.Hout) {
      const float lb = (!a.Yin && a.lin_bias) ? a.lin_bias[j] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int node = nodeS[(r & 3) + 8 * (r >> 2) + 4 * fh];
        if (node >= 0) {
          float y = acc[r] + lb + yin[r];
          if (a.act == 1) y = fmaxf(y, 0.f);
          else if (a.act == 2) y = y >= 0.f ? y : a.slope * y;
          a.Y[(int64_t)node * a.ldy + j] = y;
        }
      }
    }
  }
