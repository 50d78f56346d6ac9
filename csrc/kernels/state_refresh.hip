// Stored-state refresh (gfx950): the recurrent states the learner's forward pass just computed go
// back into the replay rows they belong to, and the launch measures how far the stored states had
// drifted (replay.state_refresh; the rule and its float64 oracle: state_refresh_ref.py).
//
// Reference: ReplayMemory.set_hs_cs (replay_memory.py), a host scatter nothing calls.  Here one
// bandwidth-bound launch for both nets, resolved on the device from the sampled starts alone:
//
//   item      one (net, chain step t, batch slot b) with ctx <= t <= t_hi[net], slot-minor, so the
//             items of consecutive waves read consecutive (H) rows of the chain's state arrays.
//             One wave per item, 4 waves per workgroup, grid-stride over the items.
//   row       the state of step t belongs to row offset j = t + dj[net] of the slot's window
//             (dj = the chain's first frame offset, + 1 with stored_state "pre"), wrapped inside the
//             slot's sub-ring.
//   owner     another slot b' of the same sub-ring reaches the same physical row at its own step
//             t' = (pos_b + t - pos_b') mod cap_e (dj cancels).  If t' is eligible and (t' > t, or
//             t' == t and b' < b) the item is not the owner and does nothing: every row is written
//             once, by the entry with the most context, ties to the smallest slot.  The lanes of
//             the wave test the B starts in parallel; no map of the replay exists.  cap_e >= T
//             keeps a slot from reaching one row twice.
//   value     [h | c], 2H floats: h = float(hi) + float(lo) (one fp32 add; lo absent in the bf16
//             engine), c the chain's fp32 cell state.  16-byte loads of c and of the stored row,
//             8-byte loads of each bf16 plane, 16-byte stores.
//   drift     per net: sum (new - old)^2 and sum new^2 for h and for c, and the rows owned.  A
//             lane forms d = new - old, fma(d, d, .), fma(new, new, .) over its 4 elements in
//             order, adds them to its row sums, the row sums to its running sums; wave_sum (xor
//             butterfly); the four waves through LDS as ((w0 + w1) + w2) + w3; partials[workgroup].
//             The last workgroup to take its ticket (nobody waits) adds the partials: thread (x, g)
//             takes value x of workgroups g, g + 16, ... in order, then value x's 16 chains in
//             order.  It writes out[0..9] and resets the ticket: no float atomics, no memset, the
//             same bits on every launch and under graph replay.  Hand-off as in r2_grad_sumsq: the
//             partials are agent-scope stores drained before the ticket's atomic add by the same
//             wave; the last arriver reads them with agent-scope loads.
//
// ``write`` = 0 ("measure") computes the same sums and stores nothing to the replay.
#include "../common.h"

namespace sr {
constexpr int NV = 10;        // on: dh, h, dc, c; tg: the same four; rows on, rows tg
constexpr int STRIDE = 16;    // floats per workgroup in the partials
// workgroups at most: 4 per CU of a whole 256-CU chip.  A partitioned or CU-masked device gets the
// same grid and runs more of them per CU in turn: the grid-stride loop and the final sum hold for
// any grid, and the drift bits depend on the grid alone, so they are the same on every device.
constexpr int MAXG = 1024;
}  // namespace sr

struct StateRefreshArgs {
  const int* starts;       // (B) sampled sequence starts
  const bf16* h[2];        // per net (steps, B, H): bf16, or the hi plane
  const bf16* h_lo[2];     // the lo plane (split precision) or null
  const float* c[2];       // (steps, B, H) fp32
  float* dst[2];           // hs_cs, target_hs_cs: (capacity, 2H) fp32
  float* out;              // sr::NV floats
  float* partials;         // gridDim.x * sr::STRIDE floats
  unsigned* ticket;        // 0 between launches
  long long capacity;
  int B, H, cap_e, ctx, write;
  int dj[2];               // row offset of step t minus t
  int t_hi[2];             // last eligible step (< ctx: none)
  int items0, items;       // items of the online net, of both
};

__global__ __launch_bounds__(256) void state_refresh_kernel(const StateRefreshArgs a) {
  __shared__ float red[4][sr::STRIDE];
  __shared__ float fin[16][sr::STRIDE];
  __shared__ int last;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int waves = (int)gridDim.x * 4;
  const int U = a.H >> 2;       // 16-byte units of h (and of c) per row
  float on[4] = {0.f, 0.f, 0.f, 0.f}, tg[4] = {0.f, 0.f, 0.f, 0.f};
  int n_on = 0, n_tg = 0;
  for (int it = (int)blockIdx.x * 4 + wv; it < a.items; it += waves) {
    const int net = it >= a.items0;
    const int k = it - (net ? a.items0 : 0);
    const int t = a.ctx + k / a.B, b = k % a.B;
    const int s = a.starts[b];
    if (s < 0 || s >= a.capacity) continue;       // never sampled: nothing to refresh
    const int pos = s % a.cap_e, base = s - pos;
    const int thi = net ? a.t_hi[1] : a.t_hi[0];
    bool beaten = false;
    for (int q = lane; q < a.B; q += 64) {
      const int s2 = a.starts[q];
      if (q == b || s2 < 0 || s2 >= a.capacity) continue;
      const int pos2 = s2 % a.cap_e;
      if (s2 - pos2 != base) continue;
      int t2 = (pos + t - pos2) % a.cap_e;
      if (t2 < 0) t2 += a.cap_e;
      beaten |= t2 >= a.ctx && t2 <= thi && (t2 > t || (t2 == t && q < b));
    }
    if (__ballot(beaten) != 0) continue;
    const long long row = base + (pos + t + (net ? a.dj[1] : a.dj[0])) % a.cap_e;   // inside the sub-ring
    float* d = (net ? a.dst[1] : a.dst[0]) + row * (2 * a.H);
    const size_t so = ((size_t)t * a.B + b) * a.H;
    const bf16* hs = (net ? a.h[1] : a.h[0]) + so;
    const bf16* hl0 = net ? a.h_lo[1] : a.h_lo[0];
    const bf16* hl = hl0 ? hl0 + so : nullptr;
    const float* cs = (net ? a.c[1] : a.c[0]) + so;
    float r[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int u = lane; u < 2 * U; u += 64) {
      const bool isc = u >= U;
      f32x4 nw;
      if (isc) {
        nw = *(const f32x4*)(cs + 4 * (u - U));
      } else {
        const bf16x4 hi = *(const bf16x4*)(hs + 4 * u);
#pragma unroll
        for (int e = 0; e < 4; ++e) nw[e] = (float)hi[e];
        if (hl) {
          const bf16x4 lo = *(const bf16x4*)(hl + 4 * u);
#pragma unroll
          for (int e = 0; e < 4; ++e) nw[e] += (float)lo[e];
        }
      }
      const f32x4 od = *(const f32x4*)(d + 4 * u);
      float dd = 0.f, nn = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float df = nw[e] - od[e];
        dd = __builtin_fmaf(df, df, dd);
        nn = __builtin_fmaf(nw[e], nw[e], nn);
      }
      r[0] += isc ? 0.f : dd;       // (the sums are >= 0: adding +0 changes no bit)
      r[1] += isc ? 0.f : nn;
      r[2] += isc ? dd : 0.f;
      r[3] += isc ? nn : 0.f;
      if (a.write) *(f32x4*)(d + 4 * u) = nw;
    }
    if (net) {
#pragma unroll
      for (int i = 0; i < 4; ++i) tg[i] += r[i];
      ++n_tg;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) on[i] += r[i];
      ++n_on;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    on[i] = wave_sum(on[i]);
    tg[i] = wave_sum(tg[i]);
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      red[wv][i] = on[i];
      red[wv][4 + i] = tg[i];
    }
    red[wv][8] = (float)n_on;       // (exact: a wave owns far fewer than 2^24 rows)
    red[wv][9] = (float)n_tg;
  }
  __syncthreads();
  if (wv == 0) {
    if (lane < sr::NV) {
      const float p = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
      __hip_atomic_store(a.partials + (size_t)blockIdx.x * sr::STRIDE + lane, p, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) {
      const unsigned tk = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last = tk == gridDim.x - 1;
    }
  }
  __syncthreads();
  if (!last) return;
  const int x = threadIdx.x & 15, g0 = threadIdx.x >> 4;
  float f = 0.f;
  if (x < sr::NV)
    for (unsigned g = g0; g < gridDim.x; g += 16)
      f += __hip_atomic_load(a.partials + (size_t)g * sr::STRIDE + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  fin[g0][x] = f;
  __syncthreads();
  if (threadIdx.x < sr::NV) {
    float t = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) t += fin[g][threadIdx.x];
    a.out[threadIdx.x] = t;
  }
  if (threadIdx.x == 0) __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// partials: >= r2_state_refresh_partials() floats; ticket: one word, 0 before the first launch (the
// kernel leaves it 0); out: 10 floats [on: sum dh^2, sum h^2, sum dc^2, sum c^2; tg: the same;
// rows on; rows tg].
extern "C" int r2_state_refresh_partials() { return sr::MAXG * sr::STRIDE; }

// starts: (B) int32.  Per net (on, tg): h (steps, B, H) bf16 -- with h_lo the hi / lo planes of
// split precision --, c (steps, B, H) fp32, steps chain steps.  hs_cs / target_hs_cs: (capacity, 2H)
// fp32, capacity a multiple of cap_e.  T = burn_in + learn; o_tg: the target chain's first frame
// offset; shift: 1 = stored_state "pre"; ctx: chain steps a state needs behind it; write: 0 =
// measure only.  Returns -1 for arguments it refuses (nothing launched).
extern "C" int r2_state_refresh(const int* starts, int B, int H, int T, int cap_e, int64_t capacity,
                                const bf16* h_on, const bf16* h_on_lo, const float* c_on, int steps_on,
                                const bf16* h_tg, const bf16* h_tg_lo, const float* c_tg, int steps_tg,
                                float* hs_cs, float* target_hs_cs, int o_tg, int shift, int ctx,
                                int write, float* out, float* partials, unsigned* ticket,
                                void* stream) {
  if (!starts || !h_on || !c_on || !h_tg || !c_tg || !hs_cs || !target_hs_cs || !out || !partials ||
      !ticket)
    return -1;
  if (B < 1 || H < 4 || (H & 3) || T < 1 || cap_e < T || capacity < cap_e || capacity % cap_e ||
      capacity > 0x7fffffffLL || (int64_t)B * T >= (1 << 24))
    return -1;
  if (o_tg < 0 || shift < 0 || shift > 1 || ctx < 0 || ctx > T - 1 || hs_cs == target_hs_cs) return -1;
  if (((uintptr_t)c_on | (uintptr_t)c_tg | (uintptr_t)hs_cs | (uintptr_t)target_hs_cs) & 15) return -1;
  if (((uintptr_t)h_on | (uintptr_t)h_on_lo | (uintptr_t)h_tg | (uintptr_t)h_tg_lo) & 7) return -1;
  StateRefreshArgs a{};
  a.starts = starts;
  a.h[0] = h_on; a.h_lo[0] = h_on_lo; a.c[0] = c_on; a.dst[0] = hs_cs;
  a.h[1] = h_tg; a.h_lo[1] = h_tg_lo; a.c[1] = c_tg; a.dst[1] = target_hs_cs;
  a.out = out; a.partials = partials; a.ticket = ticket;
  a.capacity = capacity;
  a.B = B; a.H = H; a.cap_e = cap_e; a.ctx = ctx; a.write = write != 0;
  const int steps[2] = {steps_on, steps_tg};
  int n[2];
  for (int c = 0; c < 2; ++c) {
    a.dj[c] = (c ? o_tg : 0) + shift;
    a.t_hi[c] = T - 1 - a.dj[c];
    n[c] = a.t_hi[c] >= ctx ? a.t_hi[c] - ctx + 1 : 0;
    if (n[c] > 0 && a.t_hi[c] >= steps[c]) return -1;       // the chain is shorter than its eligible steps
  }
  a.items0 = B * n[0];
  a.items = a.items0 + B * n[1];
  int grid = (a.items + 3) / 4;
  grid = grid < 1 ? 1 : (grid > sr::MAXG ? sr::MAXG : grid);
  hipLaunchKernelGGL(state_refresh_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
  R2_CHECK_LAUNCH();
  return 0;
}
