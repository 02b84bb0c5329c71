// One sorted run of a backward line, included INSIDE k_cart_bwd_long (embed_cart_hub_bwd.hip), k_cart_giant_bwd
// (embed_giant_cart_bwd.hip), k_split_bwd_runs (embed_split_cart_bwd.hip) and k_splitw_bwd_runs (embed_split_cart_w_bwd.hip): the
// wavefront gathers elements c0 + j * 64 + lane (j < M; striped: lane-contiguous col reads) of its slice, packs every key with its
// entry index, sorts the run in registers
// (WaveLine64) and parks it at run_line[c0 + lane * M + j].  Fill elements (past the line) have key +inf and sort behind it.  RUN_PAD
// (general weights): element D is the reference's pad element at key 0 with index D, last among equal keys.
// In scope at the point of inclusion: a (its ldp), colrow (a.col + the row's start), xs (a.Xp + slice), c0, D, lane, the compile-time
// constants M and RUN_PAD, and run_line (the line's packed words).  The text declares ln and c and opens no scope of its own: include
// it inside braces of its own, where neither name is in scope yet.
// Text and not a device function: as an inlined function (destination as a pointer to the run, or as the line and c0) the same
// statements came out with another register allocation or schedule in all six kernels (k_split_bwd_runs: 11023 -> 11017 instructions,
// k_cart_bwd_long: 17833 -> 17792).  Included text leaves them instruction-identical (tools/compare_kernel_asm.py).  k_cart_bwd_long_w
// keeps its own copy: it sums the row's mass inside the gather loop, and with that sum in a loop of its own next to this text it
// compiles to other code (449 -> 448 vector registers, 20081 -> 20341 instructions).
  WaveLine64<M> ln;
  int c[M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const int t = c0 + j * kWave + lane;
    c[j] = t < D ? colrow[t] : -1;
  }
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const int t = c0 + j * kWave + lane;
    const float fill = (RUN_PAD && t == D) ? 0.f : __builtin_inff();
    ln.e[j] = pack_key_index(c[j] >= 0 ? xs[(int64_t)c[j] * a.ldp] : fill, t);
  }
  ln.sort();
#pragma unroll
  for (int j = 0; j < M; ++j) run_line[c0 + lane * M + j] = ln.e[j];
