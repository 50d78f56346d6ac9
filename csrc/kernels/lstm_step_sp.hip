// Split-precision LSTM step kernel for gfx950 (MI355X): the recurrence of lstm.hip's plain step
// kernel with fp32-accurate products (csrc/split.h), one launch per step, no inter-workgroup
// hand-off.
//
// Why: the split-precision recurrence existed only as the persistent tagged kernel
// (lstm_persist.hip, r2_lstm_fwd_tag_sp), whose grid must be co-resident at one workgroup per CU.
// An actor group's step (E = 256 rows x 2 nets = 32 groups x 16 workgroups) cannot be placed that
// way, and under the concurrent driver's CU masks no co-residency can be promised at all.  This
// kernel has the decomposition of lstm_fwd_step_kernel -- workgroup j owns hidden units
// [16j, 16j+16) = 64 packed gate columns, grid.y = chain, one wave per (32-row M tile, 32-column
// N tile), pointwise cell fused after one LDS exchange -- so it runs on any CU subset.
//
// Operands: W_hh as packed hi / lo planes; h_{t-1} as fp32 at t == 0 (h0, split into hi / lo in
// registers) and as the stored planes h_seq[t-1] / h_seq_lo[t-1] afterwards; every fragment pair
// takes the three passes lo.hi + hi.lo + hi.hi (mfma32_x3) into one fp32 accumulator.
//
// Registers: 512 threads at 2 waves per SIMD leave 256 VGPRs (arch + acc) per lane.  Four
// operand fragment sets (A hi / lo, B hi / lo) are 16 VGPRs per k-step, so the full K = 256 of the
// bf16 kernel (16 k-steps) would need 256 for operands alone.  K is therefore walked in chunks of
// SP_KC = 4 k-steps (64 VGPRs) through a ring of two: the loads of chunk c + 1 are issued before
// the MFMAs of chunk c, and chunks 0 and 1 -- with every other load that does not depend on the
// result (xproj, c_prev) -- at kernel entry.  No scratch at any H (profiles/actor_fp32_step_ab.txt).
#include "../common.h"
#include "../split.h"
#include "../lstm_common.h"

#define SP_UNITS 16
#define SP_GCOLS 64
#define SP_MAX_CHAINS 4
#define SP_ITEMS 4            // (row, unit) pairs per thread: B*16 pairs over 128*ceil(B/32) threads
#define SP_KC 4               // k-steps per register chunk

struct LstmSpArgs {
  PChain ch[SP_MAX_CHAINS];   // lstm_common.h: h0 is fp32, whh_lo / h_seq_lo are the lo planes
  int B;
  int t;
};

// FIRST: t == 0, h_{t-1} = h0 in fp32, split here; otherwise the stored planes of step t - 1.
template <int H, bool FIRST>
__global__ __launch_bounds__(512) void lstm_fwd_step_sp_kernel(const LstmSpArgs a) {
  constexpr int G = 4 * H;
  constexpr int LDSW = SP_GCOLS + 4;
  constexpr int KS = H / 16;                   // k-steps
  constexpr int NC = KS / SP_KC;               // register chunks
  static_assert(KS % SP_KC == 0 && NC >= 1, "H");
  __shared__ float gl[128 * LDSW];
  const PChain& cd = a.ch[blockIdx.y];
  const int j = blockIdx.x;
  const int B = a.B, t = a.t;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int mt = wave >> 1, nt = wave & 1;
  const float* cp = FIRST ? cd.c0 : cd.c_seq + (size_t)(t - 1) * B * H;

  // ---- recurrent GEMM operands: gates[b][n] = sum_k h[b][k] * Whh_pk[j][n][k]
  const int m = mt * 32 + (lane & 31);
  const int kh = (lane >> 5) * 8;
  const size_t aoff = (size_t)(m < B ? m : B - 1) * H + kh;      // rows >= B: clamped, discarded
  const size_t boff = ((size_t)j * SP_GCOLS + nt * 32 + (lane & 31)) * H + kh;
  const float* a32 = (const float*)cd.h0 + aoff;                               // FIRST
  const bf16* ahi = cd.h_seq + (FIRST ? 0 : (size_t)(t - 1) * B * H) + aoff;   // !FIRST
  const bf16* alo = cd.h_seq_lo + (FIRST ? 0 : (size_t)(t - 1) * B * H) + aoff;
  const bf16* bhi = cd.whh + boff;
  const bf16* blo = cd.whh_lo + boff;
  bf16x8 avh[2][SP_KC], avl[2][SP_KC], bvh[2][SP_KC], bvl[2][SP_KC];
  f32x4 af[2][SP_KC][2];
  auto load_chunk = [&](int c, int slot) {
#pragma unroll
    for (int s = 0; s < SP_KC; ++s) {
      const int k = (c * SP_KC + s) * 16;
      bvh[slot][s] = *(const bf16x8*)(bhi + k);
      bvl[slot][s] = *(const bf16x8*)(blo + k);
      if constexpr (FIRST) {
        af[slot][s][0] = *(const f32x4*)(a32 + k);
        af[slot][s][1] = *(const f32x4*)(a32 + k + 4);
      } else {
        avh[slot][s] = *(const bf16x8*)(ahi + k);
        avl[slot][s] = *(const bf16x8*)(alo + k);
      }
    }
  };
  load_chunk(0, 0);
  if (NC > 1) load_chunk(1, 1);

  // ---- pointwise operands (independent of the product): xproj gate pre-activations and c_{t-1}
  // branch-free (indices clamped) so the compiler issues every load before any wait
  float xv[SP_ITEMS][4], cv[SP_ITEMS];
#pragma unroll
  for (int q = 0; q < SP_ITEMS; ++q) {
    const int idx = min(tid + q * nthr, B * SP_UNITS - 1);
    const int b = idx >> 4, u = idx & 15;
    const float* xr = cd.xproj + ((size_t)t * B + b) * G + j * SP_GCOLS + u;
    xv[q][0] = xr[0]; xv[q][1] = xr[16]; xv[q][2] = xr[32]; xv[q][3] = xr[48];
    cv[q] = cp[(size_t)b * H + j * SP_UNITS + u];
  }
  __builtin_amdgcn_sched_barrier(0);   // every entry load ahead of the first MFMA

  f32x16 acc = {};
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int slot = c & 1;
    if constexpr (FIRST) {
#pragma unroll
      for (int s = 0; s < SP_KC; ++s) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = af[slot][s][0][e]; v[4 + e] = af[slot][s][1][e]; }
        sp_split8(v, avh[slot][s], avl[slot][s]);
      }
    }
#pragma unroll
    for (int s = 0; s < SP_KC; ++s)
      acc = mfma32_x3(avh[slot][s], avl[slot][s], bvh[slot][s], bvl[slot][s], acc);
    if (c + 2 < NC) {
      __builtin_amdgcn_sched_barrier(0);   // the ring slot is free only after its MFMAs
      load_chunk(c + 2, slot);
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    gl[row * LDSW + nt * 32 + (lane & 31)] = acc[r];
  }
  __syncthreads();

  // ---- fused LSTM cell for this workgroup's 16 units
  const bool save = cd.gates != nullptr && t >= cd.save_from;
#pragma unroll
  for (int q = 0; q < SP_ITEMS; ++q) {
    const int idx = tid + q * nthr;
    if (idx >= B * SP_UNITS) break;
    const int b = idx >> 4, u = idx & 15;
    const float* gr = gl + b * LDSW;
    const float gi = sigmoidf_(gr[u] + xv[q][0]);
    const float gf = sigmoidf_(gr[16 + u] + xv[q][1]);
    const float gg = tanhf_(gr[32 + u] + xv[q][2]);
    const float go = sigmoidf_(gr[48 + u] + xv[q][3]);
    const float c = gf * cv[q] + gi * gg;
    float h = go * tanhf_(c);
    // The planes must be the roundings of exactly what h32 stores.  Without this the compiler
    // contracts h - hi into fma(go, tanh(c), -hi) on the unrounded product, and the lo plane
    // comes out one ulp off the stored h (seen against lstm_ref's bit-for-bit check).
    asm volatile("" : "+v"(h));
    const size_t o = ((size_t)t * B + b) * H + j * SP_UNITS + u;
    bf16 hh, hl;
    sp_split(h, hh, hl);
    cd.c_seq[o] = c;
    cd.h_seq[o] = hh;
    cd.h_seq_lo[o] = hl;
    if (cd.h32) cd.h32[o] = h;
    if (save) {
      float* gp = cd.gates + ((size_t)(t - cd.save_from) * B + b) * G + j * SP_GCOLS;
      gp[u] = gi;
      gp[16 + u] = gf;
      gp[32 + u] = gg;
      gp[48 + u] = go;
    }
  }
}

// chain_ptrs: n_chains x 11 int64 values, the r2_lstm_fwd_tag_sp chain layout:
//   xproj, whh, h0 (fp32), c0, h_seq, c_seq, h32, gates, save_from, whh_lo, h_seq_lo
// One launch per step t in [t_begin, T).  Refusals (nothing launched): -1 n_chains outside 1..4 or
// B outside 1..128, -2 H not in {64, 128, 256}, -5 a whh_lo / h_seq_lo pointer missing.
extern "C" int r2_lstm_fwd_sp(const int64_t* chain_ptrs, int n_chains, int B, int T, int H,
                              int t_begin, void* stream) {
  if (n_chains < 1 || n_chains > SP_MAX_CHAINS || B < 1 || B > 128) return -1;
  if (H != 64 && H != 128 && H != 256) return -2;
  LstmSpArgs args;
  for (int c = 0; c < n_chains; ++c) {
    const int64_t* p = chain_ptrs + 11 * c;
    PChain& ch = args.ch[c];
    ch.xproj = (const float*)p[0]; ch.whh = (const bf16*)p[1]; ch.h0 = (const bf16*)p[2];
    ch.c0 = (const float*)p[3]; ch.h_seq = (bf16*)p[4]; ch.c_seq = (float*)p[5];
    ch.h32 = (float*)p[6]; ch.gates = (float*)p[7]; ch.save_from = (int)p[8]; ch.pad_ = 0;
    ch.whh_lo = (const bf16*)p[9]; ch.h_seq_lo = (bf16*)p[10];
    if (!ch.whh_lo || !ch.h_seq_lo) return -5;
  }
  for (int c = n_chains; c < SP_MAX_CHAINS; ++c) args.ch[c] = args.ch[0];
  args.B = B;
  dim3 grid(H / SP_UNITS, n_chains);
  dim3 block(128 * ((B + 31) / 32));   // 2 waves (N tiles) per 32-row M tile
  hipStream_t s = (hipStream_t)stream;
  for (int t = t_begin; t < T; ++t) {
    args.t = t;
#define R2_SP_STEP(HH)                                                                         \
    if (t == 0) hipLaunchKernelGGL((lstm_fwd_step_sp_kernel<HH, true>), grid, block, 0, s, args); \
    else hipLaunchKernelGGL((lstm_fwd_step_sp_kernel<HH, false>), grid, block, 0, s, args)
    switch (H) {
      case 64: R2_SP_STEP(64); break;
      case 128: R2_SP_STEP(128); break;
      default: R2_SP_STEP(256); break;
    }
#undef R2_SP_STEP
  }
  R2_CHECK_LAUNCH();
  return 0;
}
