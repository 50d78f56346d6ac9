// Batched policy evaluator: the per-env-step bookkeeping of E evaluation envs in two launches
// around the environment step (pytorch_r2d2_amd/evaluator.py).
//
// The reference has no evaluator: it prints the returns of its exploring actors
// (actor.py:109-110).  Here E envs act on the online net alone (epsilon 0 by default) and every
// env records the returns of its first K episodes.  A per-env quota, not "the first N episodes to
// finish", which would favour short episodes.  Nothing of the replay is read or written: the two
// launches touch the evaluator's own buffers only, so evaluation can run between two learner
// steps without changing anything the learner or the actor sees.
//
//   eval_act_kernel   (one thread per env): epsilon-greedy action, the rule and the counter-based
//                     draws of actor.hip actor_pre_kernel step 5 (greedy = FIRST maximum).
//   <environment step on the device>
//   eval_post_kernel  (grid E): advance or reset the carried LSTM state of the one net, episode
//                     accounting into the (E, K) tables; the last workgroup to take its ticket
//                     does t += 1 and resets the ticket (optim.hip grad_sumsq_kernel's pattern),
//                     so there is no tail launch and graph replays need no memset.
#include "../common.h"

struct EvalArgs {
  const float* q;             // (E, A) online Q values of this step
  const float* eps;           // (E) epsilon of each env
  int64_t* act;               // (E) chosen actions (env input)
  const float* h_new;         // (E, H) next state from the LSTM step
  const float* c_new;
  float* h32;                 // (E, H) carried state (reset on done)
  float* c;
  bf16* h_bf;
  const uint8_t* env_done;    // (E) bool
  const float* env_finished;  // (E) return of the episode that just ended, where done
  float* ret;                 // (E, K) recorded returns
  int* ep_len;                // (E, K) recorded lengths
  int* len;                   // (E) steps of the running episode
  int* n_done;                // (E) episodes recorded, <= K
  int* total_done;            // (1) sum of n_done
  int64_t* counted_steps;     // (1) env steps of envs still inside their quota
  int64_t* t;                 // (1) evaluator step
  unsigned* ticket;           // (1) zero at first use
  unsigned long long seed;
  int E, A, H, K;
};

__global__ __launch_bounds__(64) void eval_act_kernel(const EvalArgs a) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= a.E) return;
  const long long t = *a.t;
  const float* q = a.q + (size_t)e * a.A;
  int greedy = 0;
  float bv = q[0];
  for (int i = 1; i < a.A; ++i)
    if (q[i] > bv) { bv = q[i]; greedy = i; }
  const float u = r2_uniform(a.seed, (uint64_t)t, 2 * (uint64_t)e);
  const int ra = min((int)(r2_uniform(a.seed, (uint64_t)t, 2 * (uint64_t)e + 1) * a.A), a.A - 1);
  a.act[e] = u < a.eps[e] ? ra : greedy;     // u >= 0: eps 0 never takes the random action
}

__global__ __launch_bounds__(64) void eval_post_kernel(const EvalArgs a) {
  const int e = blockIdx.x, tid = threadIdx.x;
  const bool dn = a.env_done[e] != 0;
  // recurrent state advances; an episode that ended restarts from zero state
  for (int i = tid; i < a.H; i += blockDim.x) {
    const size_t o = (size_t)e * a.H + i;
    const float h = dn ? 0.f : a.h_new[o];
    a.h32[o] = h;
    a.c[o] = dn ? 0.f : a.c_new[o];
    a.h_bf[o] = (bf16)h;
  }
  if (tid != 0) return;
  const int nd = a.n_done[e];
  const int L = a.len[e] + 1;
  if (nd < a.K) atomicAdd((unsigned long long*)a.counted_steps, 1ull);
  if (dn && nd < a.K) {
    const size_t slot = (size_t)e * a.K + nd;
    a.ret[slot] = a.env_finished[e];
    a.ep_len[slot] = L;
    a.n_done[e] = nd + 1;
    atomicAdd(a.total_done, 1);
  }
  a.len[e] = dn ? 0 : L;
  const unsigned k = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (k == gridDim.x - 1) {
    *a.t += 1;
    __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// each launch checks the sizes and the pointers it dereferences (the env's outputs do not exist
// yet when eval_act is launched)
static bool eval_dims_ok(const EvalArgs& a) {
  return a.E > 0 && a.A > 0 && a.A <= 64 && a.H > 0 && a.K > 0;
}
static bool eval_act_ok(const EvalArgs& a) {
  return eval_dims_ok(a) && a.q && a.eps && a.act && a.t;
}
static bool eval_post_ok(const EvalArgs& a) {
  return eval_dims_ok(a) && a.h_new && a.c_new && a.h32 && a.c && a.h_bf && a.env_done &&
         a.env_finished && a.ret && a.ep_len && a.len && a.n_done && a.total_done &&
         a.counted_steps && a.t && a.ticket;
}

extern "C" int r2_eval_act(const EvalArgs* a, void* stream) {
  if (!a || !eval_act_ok(*a)) return -1;
  hipLaunchKernelGGL(eval_act_kernel, dim3((a->E + 63) / 64), dim3(64), 0, (hipStream_t)stream, *a);
  R2_CHECK_LAUNCH();
  return 0;
}

extern "C" int r2_eval_post(const EvalArgs* a, void* stream) {
  if (!a || !eval_post_ok(*a)) return -1;
  hipLaunchKernelGGL(eval_post_kernel, dim3(a->E), dim3(64), 0, (hipStream_t)stream, *a);
  R2_CHECK_LAUNCH();
  return 0;
}

extern "C" int r2_eval_args_bytes() { return (int)sizeof(EvalArgs); }
