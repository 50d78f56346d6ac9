// One lane's share of a dueling-head dot product: PER = HD / 64 features against PER weights.
//
// The dueling forward exists twice -- head.hip dueling_fwd_kernel and td.hip td_duel_row (the
// forward fused into the TD launch) -- and their Q rows are claimed, and tested
// (tests/test_td_head_gpu.py), to agree bit for bit.  That holds only if both sums round the same
// way, and "s += h[e] * w[e]" leaves the compiler a choice: at PER = 8 (HD = 512) the two kernels
// came out with different mixes of FMAs and of packed multiplies followed by separate adds, and
// the Q rows differed in the last bits.  So at PER = 8 the sum is an explicit FMA chain, which the
// compiler may pack but cannot split.  Up to PER = 4 both kernels contract the plain expression
// alike (the same test pins it), and it stays as it is: the heads in use (HD = 64, 256) keep the
// bits they have.
#pragma once

template <int PER>
__device__ __forceinline__ float head_lane_dot(const float (&h)[PER], const float* w) {
  float s = 0.f;
  if constexpr (PER > 4) {
#pragma unroll
    for (int e = 0; e < PER; ++e) s = __builtin_fmaf(h[e], w[e], s);
  } else {
#pragma unroll
    for (int e = 0; e < PER; ++e) s += h[e] * w[e];
  }
  return s;
}
