// The first statements of every kernel with one lane per slice (grid.y = ceil(S / 256), four wavefronts per workgroup; embed_reg.hip,
// embed_mid.hip, embed_mid_bwd.hip, embed_bwd.hip, embed_w_bwd.hip): the wavefront's chunk of 64 slices and the lane's slice k.  A
// wavefront whose chunk lies behind the last slice RETURNS from the kernel here.  Lanes behind the last slice of the last chunk
// (kvalid false) compute slice kc = S - 1 again and store nothing, or the same value to the same address.
// In scope at the point of inclusion: S.  The text declares chunk, k, kvalid and kc.
// Text and not a device function: a function that returns "leave" with k, kvalid and kc as results has them computed ahead of the
// branch, and the kernels come out with another register allocation (k_segment_sum_rows, k_embed_reg_w_bwd) or another length
// (k_embed_reg_unit_bwd<17, 32>: 65250 -> 65253 instructions, k_embed_mid_unit_pf<192, 192>: 13507 -> 13515).  Included text leaves all
// eleven instruction-identical (tools/compare_kernel_asm.py).
  [[maybe_unused]] const int chunk = blockIdx.y * 4 + wave_id();
  if (chunk * kWave >= S) return;
  [[maybe_unused]] const int k = chunk * kWave + lane_id();
  [[maybe_unused]] const bool kvalid = k < S;
  const int kc = kvalid ? k : S - 1;
