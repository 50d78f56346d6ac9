// One element of the Adam update (torch.optim.Adam: bias-corrected, eps outside the sqrt), shared
// by optim.hip's adam_kernel (scalar, no packs) and adam_pack_kernel (rms_pack.h opt_pack_items
// with AdamUpd), which are claimed, and tested (tests/test_optim_fast_gpu.py), to agree bit for
// bit:
//   m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g ; p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
// with bc1 = 1 - b1^t, bc2 = 1 - b2^t.  The step count t = *step + step_off is read from device
// memory so HIP-graph replays advance it: step_off 1 when the update runs before the priority
// tail advances the counter (the plain step), 0 when it runs after (the hoisted step).
//
// "b1 * m + (1 - b1) * g" leaves the compiler a choice of FMAs (csrc/head_dot.h met the same):
// adam_kernel came out with none -- separate (packed) multiplies and adds -- and the pack kernel's
// quad loop need not.  The contraction is therefore switched off for the helper's body: every
// product and sum below is rounded on its own, in both kernels.
#pragma once
#include "common.h"

struct AdamCoef {
  float b1, b2, omb1, omb2, step_size, bc2s, eps;
};

__device__ __forceinline__ AdamCoef adam_coef(float lr, float b1, float b2, float eps,
                                              const int64_t* __restrict__ step, int64_t step_off) {
  const float t = (float)(*step + step_off);
  const float bc1 = 1.f - powf(b1, t), bc2 = 1.f - powf(b2, t);
  return AdamCoef{b1, b2, 1.f - b1, 1.f - b2, lr / bc1, sqrtf(bc2), eps};
}

__device__ __forceinline__ float adam_elem(float& m, float& v, float p, float gr, const AdamCoef& c) {
#pragma clang fp contract(off)
  const float mi = c.b1 * m + c.omb1 * gr;
  const float vi = c.b2 * v + c.omb2 * gr * gr;
  m = mi;
  v = vi;
  return p - c.step_size * mi / (sqrtf(vi) / c.bc2s + c.eps);
}

// the update functor of rms_pack.h opt_pack_items / opt_torso_items (state words: m, v)
struct AdamUpd {
  AdamCoef c;
  __device__ __forceinline__ float operator()(float& m, float& v, float p, float gr) const {
    return adam_elem(m, v, p, gr, c);
  }
};
