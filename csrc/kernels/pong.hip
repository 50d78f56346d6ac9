// A Pong-like game on the device, one launch per agent step for all E envs.
//
// The game is defined by pytorch_r2d2_amd/pong_ref.py (integers only: Q8 positions, counter-hash
// draws) and this kernel copies it bit for bit; it is a native game rendered at 84x84 gray, not
// the Atari 2600 one.  One workgroup per env, as in env.hip: thread 0 runs the action_repeat
// (<= 64) raw frames of the step (paddles, opponent, serve timer, ball, walls, swept paddle hit,
// points, the in-place reset of a finished episode) and leaves one record per shown frame in
// LDS -- ball pixel position, both paddle rows, both scores; after one barrier all 256 threads
// render the C stacked planes from the records, one 4-byte word of one row at a time, as 16-byte
// vectors (a plane is 7056 B = 441 vectors; W % 4 == 0, so a word lies in one row).  Every global
// write is a plain store by the env's own workgroup: no atomics, no cross-workgroup traffic, no
// host sync, graph-capturable.
#include "../common.h"

struct PongArgs {
  const long long* action;   // (E) actions of this step
  int* state;                // (E, 10) X Y VX VY PA PO SA SO TIMER T
  long long* k;              // (E) per-env RNG counter
  float* ep_return;          // (E)
  float* reward;             // (E) out
  bool* done;                // (E) out
  float* finished;           // (E) out: the episode return where done, else NaN
  uint8_t* frames;           // (E, C*84*84) out: the next observation
  unsigned long long seed;
  int E, A, C, H, W, action_repeat, points, max_steps, lapse;
};

namespace {
constexpr int kH = 84, kW = 84, kNS = 10, kMaxC = 8, kMaxPoints = 42;
constexpr int kQ = 256, kPadH = 8, kPadMin = 6, kPadMax = 82 - kPadH, kPadHome = 40;
constexpr int kYMin = 6 * kQ, kYMax = 80 * kQ, kFaceO = 6 * kQ, kFaceA = 78 * kQ, kXRight = 82 * kQ;
constexpr int kXServe = 41 * kQ, kYServe = 43 * kQ, kCentreRow = 44;
constexpr int kSpeed0 = 192, kSpeedUp = 24, kSpeedMax = 640, kAngle = 72, kSpin = 48, kServeVy = 72;
constexpr int kServeFrames = 16;
constexpr uint32_t kBg = 87, kLit = 236, kAgent = 147, kOpp = 148;
enum : unsigned long long { SALT_LAPSE = 1, SALT_SPIN = 2, SALT_SERVE = 3, SALT_DIR = 4 };

struct Rec { int bx, by, pa, po, sa, so; };

__device__ __forceinline__ uint32_t pong_draw(uint64_t seed, long long k, unsigned long long salt, int e) {
  // env.hip env_hash(seed, k, salt * 2^32 + e)
  return (uint32_t)(r2_mix64(seed ^ r2_mix64((uint64_t)k * 0x9E3779B97F4A7C15ull + ((salt << 32) + (uint64_t)e))) >> 32);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Four pixels of one row (a 4-byte word never straddles a row), byte j = column col0 + j.  The
// paddles' columns are bytes 0-1 of the word at column 4 and bytes 2-3 of the word at column 76.
__device__ __forceinline__ uint32_t pong_word(const Rec& r, int row, int col0) {
  constexpr uint32_t kBg4 = kBg * 0x01010101u, kLit4 = kLit * 0x01010101u;
  if (row < 6 || row >= 82) {
    if (row >= 4) return kLit4;
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = col0 + j;
      w |= ((col < r.so || col >= kW - r.sa) ? kLit : kBg) << (8 * j);
    }
    return w;
  }
  uint32_t w = kBg4;
  if (col0 == 4 && (unsigned)(row - r.po) < (unsigned)kPadH) w = (kBg4 & 0xFFFF0000u) | (kOpp * 0x0101u);
  if (col0 == 76 && (unsigned)(row - r.pa) < (unsigned)kPadH) w = (kBg4 & 0x0000FFFFu) | (kAgent * 0x01010000u);
  if ((unsigned)(row - r.by) < 2u) {
    const int d = r.bx - col0;   // the ball's two columns are bytes d and d + 1 of this word
    uint32_t m = 0;
    if ((unsigned)d < 4u) m |= 0xFFu << (8 * d);
    if ((unsigned)(d + 1) < 4u) m |= 0xFFu << (8 * (d + 1));
    w = (w & ~m) | (kLit4 & m);
  }
  return w;
}
}  // namespace

__global__ __launch_bounds__(256) void pong_env_step_kernel(const PongArgs a) {
  const int e = blockIdx.x, tid = threadIdx.x;
  __shared__ Rec s_rec[kMaxC];
  // Whether the opponent idles in raw frame f depends on the counter alone, not on the game: lane
  // f of the first wave draws it beside the others and a ballot hands thread 0 all of them, which
  // takes action_repeat hashes off its serial chain.  The wave loads the env's scalars first (one
  // address per load, all in flight together) so that thread 0 does not wait for them a second time.
  unsigned long long stays = 0;
  long long k = 0, act = 0;
  float ret0 = 0.f;
  int s[kNS] = {};
  int* st = a.state + (size_t)e * kNS;
  if (tid < 64) {
    k = a.k[e];
    act = a.action[e];
    ret0 = a.ep_return[e];
#pragma unroll
    for (int i = 0; i < kNS; ++i) s[i] = st[i];
    stays = __ballot(tid < a.action_repeat &&
                     (int)(pong_draw(a.seed, k + 1 + tid, SALT_LAPSE, e) & 255u) < a.lapse);
  }
  if (tid == 0) {
    int x = s[0], y = s[1], vx = s[2], vy = s[3], pa = s[4], po = s[5], sa = s[6], so = s[7];
    int timer = s[8], t = s[9];
    const int dy = (act == 2 || act == 4) ? -2 : ((act == 3 || act == 5) ? 2 : 0);
    const int first = a.action_repeat - a.C;
    int total = 0;
    bool on_points = false;
    for (int f = 0; f < a.action_repeat; ++f) {
      k += 1;
      pa = clampi(pa + dy, kPadMin, kPadMax);
      if (!((stays >> f) & 1ull)) {
        const int aim = vx < 0 ? (y >> 8) + 1 : kCentreRow;
        const int c = po + kPadH / 2;
        po = clampi(po + (aim > c ? 1 : (aim < c ? -1 : 0)), kPadMin, kPadMax);
      }
      if (timer > 0) {
        timer -= 1;
      } else {
        int x2 = x + vx, y2 = y + vy;
        if (y2 < kYMin) { y2 = 2 * kYMin - y2; vy = -vy; }
        else if (y2 > kYMax) { y2 = 2 * kYMax - y2; vy = -vy; }
        const int by = y2 >> 8;
        const bool hit_a = vx > 0 && x + 2 * kQ <= kFaceA && x2 + 2 * kQ > kFaceA && by + 1 >= pa && by <= pa + kPadH - 1;
        const bool hit_o = vx < 0 && x >= kFaceO && x2 < kFaceO && by + 1 >= po && by <= po + kPadH - 1;
        if (hit_a || hit_o) {
          const int av = vx < 0 ? -vx : vx;
          const int speed = av + kSpeedUp < kSpeedMax ? av + kSpeedUp : kSpeedMax;
          const int spin = ((int)(pong_draw(a.seed, k, SALT_SPIN, e) % 3u) - 1) * kSpin;
          const int top = hit_a ? pa : po;
          x2 = hit_a ? 2 * (kFaceA - 2 * kQ) - x2 : 2 * kFaceO - x2;
          vx = hit_a ? -speed : speed;
          vy = (((y2 + kQ - (top + kPadH / 2) * kQ) * kAngle) >> 8) + spin;
        }
        const bool pt_a = x2 + 2 * kQ <= 0, pt_o = x2 >= kXRight;
        if (pt_a || pt_o) {
          sa += pt_a;
          so += pt_o;
          total += pt_a ? 1 : -1;
          x2 = kXServe;
          y2 = kYServe;
          vx = pt_a ? -kSpeed0 : kSpeed0;
          vy = ((int)(pong_draw(a.seed, k, SALT_SERVE, e) % 5u) - 2) * kServeVy;
          timer = kServeFrames;
        }
        x = x2;
        y = y2;
      }
      if (f >= first) s_rec[f - first] = Rec{x >> 8, y >> 8, pa, po, sa, so};
      if (sa >= a.points || so >= a.points) { on_points = true; break; }
    }
    t += 1;
    const bool d = on_points || t >= a.max_steps;
    const float r = (float)total;
    const float ret = ret0 + r;
    a.reward[e] = r;
    a.done[e] = d;
    a.finished[e] = d ? ret : __builtin_nanf("");
    a.ep_return[e] = d ? 0.f : ret;
    if (d) {
      x = kXServe;
      y = kYServe;
      vx = (pong_draw(a.seed, k, SALT_DIR, e) & 1u) ? kSpeed0 : -kSpeed0;
      vy = ((int)(pong_draw(a.seed, k, SALT_SERVE, e) % 5u) - 2) * kServeVy;
      pa = po = kPadHome;
      sa = so = 0;
      timer = kServeFrames;
      t = 0;
      for (int p = 0; p < a.C; ++p) s_rec[p] = Rec{x >> 8, y >> 8, pa, po, sa, so};
    }
    st[0] = x; st[1] = y; st[2] = vx; st[3] = vy; st[4] = pa; st[5] = po; st[6] = sa; st[7] = so;
    st[8] = timer; st[9] = t;
    a.k[e] = k;
  }
  __syncthreads();
  constexpr int kVecs = kH * kW / 16;   // 441 vectors per plane
  u32x4* dst = reinterpret_cast<u32x4*>(a.frames + (size_t)e * a.C * (kH * kW));
  for (int v = tid; v < a.C * kVecs; v += blockDim.x) {
    const int p = v / kVecs;
    const Rec r = s_rec[p];
    const int byte0 = (v - p * kVecs) * 16;
    uint32_t w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int b = byte0 + q * 4;
      const int row = b / kW;
      w[q] = pong_word(r, row, b - row * kW);
    }
    dst[v] = u32x4{w[0], w[1], w[2], w[3]};
  }
}

extern "C" int r2_pong_args_bytes() { return (int)sizeof(PongArgs); }

extern "C" int r2_pong_env_step(const PongArgs* a, void* stream) {
  if (!a) return -1;
  if (a->E <= 0 || a->A != 6 || a->H != kH || a->W != kW) return -1;
  if (a->C < 1 || a->C > kMaxC || a->C > a->action_repeat || a->action_repeat > 64) return -1;
  if (a->points < 1 || a->points > kMaxPoints || a->max_steps <= 0 || a->lapse < 0 || a->lapse > 256) return -1;
  if (!a->action || !a->state || !a->k || !a->ep_return || !a->reward || !a->done || !a->finished || !a->frames)
    return -1;
  hipLaunchKernelGGL(pong_env_step_kernel, dim3(a->E), dim3(256), 0, (hipStream_t)stream, *a);
  R2_CHECK_LAUNCH();
  return 0;
}
