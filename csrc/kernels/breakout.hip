// A Breakout-like game on the device, one launch per agent step for all E envs.
//
// The game is defined by pytorch_r2d2_amd/breakout_ref.py (integers only: Q8 positions, pong_ref's
// counter-hash draws) and this kernel copies it bit for bit; it is a native game rendered at 84x84
// gray, not the Atari 2600 one.  The shape is pong.hip's.  One workgroup of 256 threads per env:
// the first wave loads the env's scalars with all loads in flight, lane f of it draws raw frame
// f's flicker bit and a ballot hands thread 0 all of them; thread 0 runs the action_repeat (<= 64)
// raw frames of the step with the six brick words in registers (paddle, serve timer, ball, walls,
// at most one brick, swept paddle hit, a lost life, the in-place reset of a finished episode) and
// leaves one record per shown frame in LDS -- ball pixel, paddle column, lives, the brick words,
// the blank flag; after one barrier all threads render the C stacked planes from the records, one
// 4-byte word of one row at a time, as 16-byte vectors (a plane is 7056 B = 441 vectors;
// W % 4 == 0, so a word lies in one row, and in the brick band a word is one brick or background).
// The render is most of the launch's time (profiles/breakout_env.txt), hence brk_vector's shape.
// Every global write is a plain store by the env's own workgroup: no atomics, no cross-workgroup
// traffic, no host sync, graph-capturable.
#include "../common.h"

struct BreakoutArgs {
  const long long* action;   // (E) actions of this step
  int* state;                // (E, 14) X Y VX VY PX LIVES TIMER T B0..B5
  long long* k;              // (E) per-env RNG counter
  float* ep_return;          // (E)
  float* reward;             // (E) out
  bool* done;                // (E) out
  float* finished;           // (E) out: the episode return where done, else NaN
  uint8_t* frames;           // (E, C*84*84) out: the next observation
  unsigned long long seed;
  int E, A, C, H, W, action_repeat, lives, max_steps, flicker;
};

namespace {
constexpr int kH = 84, kW = 84, kRows = 6, kCols = 19, kNS = 8 + kRows, kMaxC = 8, kMaxLives = 5;
constexpr int kQ = 256, kBrickTop = 16, kUpperRows = 4, kPlayLeft = 4, kPlayRight = 80;
constexpr int kPadW = 12, kPadRow = 78, kPadStep = 3, kPadMin = kPlayLeft, kPadMax = kPlayRight - kPadW;
constexpr int kPadHome = 36;
constexpr int kXMin = kPlayLeft * kQ, kXMax = (kPlayRight - 2) * kQ, kYMin = 6 * kQ, kYOut = kH * kQ;
constexpr int kFace = kPadRow * kQ, kXServe = 41 * kQ, kYServe = 40 * kQ, kServeVy = 160, kServeVx = 72;
constexpr int kSpeedUpper = 320, kSpeedUp = 8, kSpeedMax = 448, kAngle = 40, kSpin = 32, kServeFrames = 16;
constexpr uint32_t kFullRow = (1u << kCols) - 1u;
constexpr uint32_t kBg = 24, kWall = 142, kLife = 200, kPaddle = 110, kBall = 236;
// the brick rows' lumas 98 119 133 151 129 90, row r in byte r
constexpr unsigned long long kRowLuma = 98ull | (119ull << 8) | (133ull << 16) | (151ull << 24) |
                                        (129ull << 32) | (90ull << 40);
enum : unsigned long long { SALT_SPIN = 2, SALT_SERVE = 3, SALT_FLICKER = 6 };

struct alignas(16) Rec { int bx, by, px, lives; uint32_t b[kRows]; int blank, pad; };   // three 16-byte LDS reads

__device__ __forceinline__ uint32_t brk_draw(uint64_t seed, long long k, unsigned long long salt, int e) {
  // env.hip env_hash(seed, k, salt * 2^32 + e)
  return (uint32_t)(r2_mix64(seed ^ r2_mix64((uint64_t)k * 0x9E3779B97F4A7C15ull + ((salt << 32) + (uint64_t)e))) >> 32);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ int serve_vx(uint64_t seed, long long k, int e) {
  // -144 / -72 / 72 / 144 for draw % 4 = 0 / 1 / 2 / 3
  const int d = (int)(brk_draw(seed, k, SALT_SERVE, e) & 3u);
  return d < 2 ? (d - 2) * kServeVx : (d - 1) * kServeVx;
}

// One 16-byte vector of a plane: four 4-byte words, each within one row (W % 4 == 0), the vector
// within two rows.  The record is in registers (one copy per vector, as in pong.hip).  Every word
// first gets what its place alone decides (strip, walls, background); the bricks, the paddle and
// the ball are laid over it only by the vectors whose two rows can hold them, so most waves skip
// all three, and the brick words of the two rows are picked once per vector by a chain of selects
// (no register array is indexed).
__device__ __forceinline__ u32x4 brk_vector(const Rec& r, int byte0) {
  constexpr uint32_t kBg4 = kBg * 0x01010101u, kWall4 = kWall * 0x01010101u, kBall4 = kBall * 0x01010101u;
  constexpr uint32_t kLife4 = kLife * 0x01010101u;
  const int row0 = byte0 / kW, col0 = byte0 - row0 * kW;
  int row[4], col[4];
  uint32_t w[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = col0 + 4 * q;
    const bool wrap = c >= kW;
    row[q] = row0 + (wrap ? 1 : 0);
    col[q] = wrap ? c - kW : c;
    const bool side = (unsigned)(col[q] - kPlayLeft) >= (unsigned)(kPlayRight - kPlayLeft);
    w[q] = row[q] < 4 ? (col[q] < 4 * r.lives ? kLife4 : kBg4) : ((row[q] < 6 || side) ? kWall4 : kBg4);
  }
  if (row0 + 1 >= kBrickTop && row0 < kBrickTop + 2 * kRows) {
    uint32_t bw[2], l4[2];   // the standing bricks and the luma of rows row0 and row0 + 1
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int band = row0 + h - kBrickTop, br = band >> 1;   // outside the band no select matches
      uint32_t word = 0;
#pragma unroll
      for (int i = 0; i < kRows; ++i) word = (i == br && (unsigned)band < (unsigned)(2 * kRows)) ? r.b[i] : word;
      bw[h] = word & kFullRow;
      l4[h] = (uint32_t)((kRowLuma >> (8 * (br & 7))) & 0xFFull) * 0x01010101u;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool second = row[q] != row0;
      // columns 0-3 give bit 31 and columns 80-83 bit 19: no brick there
      if (((second ? bw[1] : bw[0]) >> (((unsigned)(col[q] - kPlayLeft) >> 2) & 31u)) & 1u) w[q] = second ? l4[1] : l4[0];
    }
  }
  if (row0 + 1 >= kPadRow && row0 < kPadRow + 2) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if ((unsigned)(row[q] - kPadRow) < 2u) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((unsigned)(col[q] + j - r.px) < (unsigned)kPadW) w[q] = (w[q] & ~(0xFFu << (8 * j))) | (kPaddle << (8 * j));
      }
    }
  }
  if ((unsigned)(row0 + 1 - r.by) < 3u) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if ((unsigned)(row[q] - r.by) < 2u) {
        const int d = r.bx - col[q];   // the ball's two columns are bytes d and d + 1 of this word
        uint32_t m = 0;
        if ((unsigned)d < 4u) m |= 0xFFu << (8 * d);
        if ((unsigned)(d + 1) < 4u) m |= 0xFFu << (8 * (d + 1));
        w[q] = (w[q] & ~m) | (kBall4 & m);
      }
    }
  }
  if (r.blank) return u32x4{0u, 0u, 0u, 0u};
  return u32x4{w[0], w[1], w[2], w[3]};
}
}  // namespace

__global__ __launch_bounds__(256) void breakout_env_step_kernel(const BreakoutArgs a) {
  const int e = blockIdx.x, tid = threadIdx.x;
  __shared__ Rec s_rec[kMaxC];
  // Whether the plane of raw frame f is blank depends on the counter alone, not on the game: lane
  // f of the first wave draws it beside the others and a ballot hands thread 0 all of them.  The
  // wave loads the env's scalars first (one address per load, all in flight together) so that
  // thread 0 does not wait for them a second time.
  unsigned long long blanks = 0;
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
    blanks = __ballot(tid < a.action_repeat &&
                      (int)(brk_draw(a.seed, k + 1 + tid, SALT_FLICKER, e) & 255u) < a.flicker);
  }
  if (tid == 0) {
    int x = s[0], y = s[1], vx = s[2], vy = s[3], px = s[4], lives = s[5], timer = s[6], t = s[7];
    uint32_t b[kRows];
#pragma unroll
    for (int i = 0; i < kRows; ++i) b[i] = (uint32_t)s[8 + i];
    const int dx = (act == 2 || act == 4) ? kPadStep : ((act == 3 || act == 5) ? -kPadStep : 0);
    const int first = a.action_repeat - a.C;
    int total = 0;
    bool over = false;
    for (int f = 0; f < a.action_repeat; ++f) {
      k += 1;
      px = clampi(px + dx, kPadMin, kPadMax);
      if (timer > 0) {
        timer -= 1;
      } else {
        const int y0 = y;
        x += vx;
        y += vy;
        if (x < kXMin) { x = 2 * kXMin - x; vx = -vx; }
        else if (x > kXMax) { x = 2 * kXMax - x; vx = -vx; }
        if (y < kYMin) { y = 2 * kYMin - y; vy = -vy; }
        // at most one brick: the leading row, the ball's left column first
        const int band = (vy < 0 ? (y >> 8) : (y >> 8) + 1) - kBrickTop;
        if ((unsigned)band < (unsigned)(2 * kRows)) {
          const int br = band >> 1;
          uint32_t word = 0;
#pragma unroll
          for (int i = 0; i < kRows; ++i) word = i == br ? b[i] : word;
          const int c0 = (x >> 8) - kPlayLeft, c1 = c0 + 1;      // columns of the play area
          const bool h0 = (unsigned)c0 < (unsigned)(kPlayRight - kPlayLeft) && ((word >> (c0 >> 2)) & 1u);
          const bool h1 = !h0 && (unsigned)c1 < (unsigned)(kPlayRight - kPlayLeft) && ((word >> (c1 >> 2)) & 1u);
          if (h0 || h1) {
            word &= ~(1u << ((h0 ? c0 : c1) >> 2));
#pragma unroll
            for (int i = 0; i < kRows; ++i) b[i] = i == br ? word : b[i];
            total += br < 2 ? 7 : (br < 4 ? 4 : 1);
            vy = -vy;
            if (br < kUpperRows && (vy < 0 ? -vy : vy) < kSpeedUpper) vy = vy < 0 ? -kSpeedUpper : kSpeedUpper;
          }
        }
        const int bx = x >> 8;
        if (vy > 0 && y0 + 2 * kQ <= kFace && y + 2 * kQ > kFace && bx + 1 >= px && bx <= px + kPadW - 1) {
          const int speed = vy + kSpeedUp < kSpeedMax ? vy + kSpeedUp : kSpeedMax;
          const int spin = ((int)(brk_draw(a.seed, k, SALT_SPIN, e) % 3u) - 1) * kSpin;
          y = 2 * (kFace - 2 * kQ) - y;
          vy = -speed;
          vx = (((x + kQ - (px + kPadW / 2) * kQ) * kAngle) >> 8) + spin;
        }
        if (y >= kYOut) {
          lives -= 1;
          x = kXServe;
          y = kYServe;
          vx = serve_vx(a.seed, k, e);
          vy = kServeVy;
          timer = kServeFrames;
        }
      }
      if (f >= first) {
        Rec* r = &s_rec[f - first];
        r->bx = x >> 8; r->by = y >> 8; r->px = px; r->lives = lives;
#pragma unroll
        for (int i = 0; i < kRows; ++i) r->b[i] = b[i];
        r->blank = (int)((blanks >> f) & 1ull);
      }
      uint32_t wall = 0;
#pragma unroll
      for (int i = 0; i < kRows; ++i) wall |= b[i];
      if (lives <= 0 || wall == 0) { over = true; break; }
    }
    t += 1;
    const bool d = over || t >= a.max_steps;
    const float r = (float)total;
    const float ret = ret0 + r;
    a.reward[e] = r;
    a.done[e] = d;
    a.finished[e] = d ? ret : __builtin_nanf("");
    a.ep_return[e] = d ? 0.f : ret;
    if (d) {
      x = kXServe;
      y = kYServe;
      vx = serve_vx(a.seed, k, e);
      vy = kServeVy;
      px = kPadHome;
      lives = a.lives;
      timer = kServeFrames;
      t = 0;
#pragma unroll
      for (int i = 0; i < kRows; ++i) b[i] = kFullRow;
      for (int p = 0; p < a.C; ++p) {
        Rec* r2 = &s_rec[p];
        r2->bx = x >> 8; r2->by = y >> 8; r2->px = px; r2->lives = lives;
#pragma unroll
        for (int i = 0; i < kRows; ++i) r2->b[i] = kFullRow;
        r2->blank = 0;
      }
    }
    st[0] = x; st[1] = y; st[2] = vx; st[3] = vy; st[4] = px; st[5] = lives; st[6] = timer; st[7] = t;
#pragma unroll
    for (int i = 0; i < kRows; ++i) st[8 + i] = (int)b[i];
    a.k[e] = k;
  }
  __syncthreads();
  constexpr int kVecs = kH * kW / 16;   // 441 vectors per plane
  u32x4* dst = reinterpret_cast<u32x4*>(a.frames + (size_t)e * a.C * (kH * kW));
  for (int v = tid; v < a.C * kVecs; v += blockDim.x) {
    const int p = v / kVecs;
    const Rec r = s_rec[p];
    dst[v] = brk_vector(r, (v - p * kVecs) * 16);
  }
}

extern "C" int r2_breakout_args_bytes() { return (int)sizeof(BreakoutArgs); }

extern "C" int r2_breakout_env_step(const BreakoutArgs* a, void* stream) {
  if (!a) return -1;
  if (a->E <= 0 || a->A != 6 || a->H != kH || a->W != kW) return -1;
  if (a->C < 1 || a->C > kMaxC || a->C > a->action_repeat || a->action_repeat > 64) return -1;
  if (a->lives < 1 || a->lives > kMaxLives || a->max_steps <= 0 || a->flicker < 0 || a->flicker > 256) return -1;
  if (!a->action || !a->state || !a->k || !a->ep_return || !a->reward || !a->done || !a->finished || !a->frames)
    return -1;
  hipLaunchKernelGGL(breakout_env_step_kernel, dim3(a->E), dim3(256), 0, (hipStream_t)stream, *a);
  R2_CHECK_LAUNCH();
  return 0;
}
