// Device-resident environments: CueRoom (environments/cue_room_env.py is the ONE host definition of the rule) stepped, auto-reset and
// rendered by one launch per worker group and step.  One workgroup per environment:
//   thread 0 reads the environment's state and its action, advances the state (position, episode step, return, episode index,
//   target), decides reward / done / truncated / success, starts the next episode where done, writes the result words and the new
//   state, and leaves the four numbers the picture depends on in LDS; after ONE barrier all threads fill the frame of the NEW state
//   with 4-byte stores (cell % 4 == 0: a word never straddles two cells).
// Only thread 0 of workgroup w ever touches state[w], once per launch: the state is read before anything overwrites it and advanced
// exactly once.  Integer arithmetic throughout (the two reward constants are the only floats; the return is a count of them), no
// atomics, no dependence on launch geometry: two calls from equal state give equal bytes.
// The episode draw is splitmix64 of splitmix64(stream) + episode in uint64 (cue_room_env.episode_draw).
// The completion word (optional) is a second, one-thread launch behind the step on the same stream: the workgroups of the step have
// no arrival counter (that would be an atomic), so "everything is written" is the stream's order; the store itself is the sampling
// kernels' hand-over (one system-scope fence, then a system-scope release store).
// CommandRoom (environments/command_room_env.py), further down, is the second task of the same shape; the two share splitmix64, the
// output record (EnvOut), the argument validation (env_check) and the publish launch (env_publish).
#include "etm_common.h"

namespace {
constexpr int CR_THREADS = 256;
constexpr int CR_MAX_GRID = 31, CR_MAX_CELL = 64;

struct CueState {                      // 32 bytes per environment (etm_cue_room_state_bytes)
  unsigned long long episode;
  int row, col, t, target, ret, pad;
};
static_assert(sizeof(CueState) == 32, "CueState is 32 bytes");

struct CueRule {
  int G, P, cue_steps, max_steps;
  unsigned long long stream0;          // seed + first worker id; environment w draws from stream0 + w
};

struct EnvOut {                        // the output record of every task here
  unsigned char *frames;               // environment w's frame at frames + w * pitch: [3, G P, G P] bytes
  long long pitch;
  float *rewards;                      // [W]
  unsigned char *flags;                // [W]: bit 0 done, bit 1 truncated, bit 2 success
  float *returns;                      // [W]: the return of the episode that ended (else 0)
  int *lengths;                        // [W]: its length (else 0)
  long long *masks;                    // [W]: bit a set when move a stays on the grid, for the frame written
};

// flat colours (R, G, B) of floor, goal, cue, agent, one byte per channel replicated over a 4-byte word (cue_room_env.PALETTE)
__device__ __constant__ unsigned cr_palette[4][3] = {{24u * 0x01010101u, 24u * 0x01010101u, 32u * 0x01010101u},
                                                     {64u * 0x01010101u, 160u * 0x01010101u, 64u * 0x01010101u},
                                                     {240u * 0x01010101u, 208u * 0x01010101u, 32u * 0x01010101u},
                                                     {224u * 0x01010101u, 48u * 0x01010101u, 48u * 0x01010101u}};

__device__ __forceinline__ unsigned long long cr_splitmix64(unsigned long long x) {
  unsigned long long z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ void cr_draw(CueState &s, unsigned long long stream, int G) {
  const unsigned long long h = cr_splitmix64(cr_splitmix64(stream) + s.episode);
  s.target = (int)(h & 3ull);
  int c = (int)((h >> 8) % (unsigned long long)(G * G - 4)) + 1;      // row-major, the corners skipped
  if (c >= G - 1) ++c;
  if (c >= G * (G - 1)) ++c;
  s.row = c / G;
  s.col = c % G;
  s.t = 0;
  s.ret = 0;
}

// corner k of cell (r, c): 0 top left, 1 top right, 2 bottom right, 3 bottom left; -1: no corner
__device__ __forceinline__ int cr_corner(int r, int c, int G) {
  if (r == 0) return c == 0 ? 0 : (c == G - 1 ? 1 : -1);
  if (r == G - 1) return c == G - 1 ? 2 : (c == 0 ? 3 : -1);
  return -1;
}

template <bool RESET>
__global__ __launch_bounds__(CR_THREADS) void cue_room_kernel(CueState *__restrict__ state, const long long *__restrict__ actions,
                                                              long long act_ld, const CueRule rule, const EnvOut out) {
  __shared__ int pic[4];               // agent row, agent column, target, cue visible
  const int w = blockIdx.x, G = rule.G;
  if (threadIdx.x == 0) {
    CueState s;
    float reward = 0.f;
    unsigned flag = 0;
    int ep_ret = 0, ep_len = 0;
    if (RESET) {
      s.episode = 0;
      s.pad = 0;
      cr_draw(s, rule.stream0 + (unsigned long long)w, G);
    } else {
      s = state[w];
      long long a = actions[(long long)w * act_ld];
      a = a < 0 ? 0 : (a > 3 ? 3 : a);                                 // (the host rule raises; the kernel never leaves the table)
      const int r = s.row + (a == 0 ? -1 : (a == 2 ? 1 : 0)), c = s.col + (a == 1 ? 1 : (a == 3 ? -1 : 0));
      if (r >= 0 && r < G && c >= 0 && c < G) {
        s.row = r;
        s.col = c;
      }
      s.t += 1;
      const int k = cr_corner(s.row, s.col, G);
      if (k >= 0) {
        const bool hit = k == s.target;
        if (hit) {
          reward = 1.f;
          s.ret += 1;
        }
        flag = 1u | (hit ? 4u : 0u);
      } else if (s.t >= rule.max_steps) {
        flag = 1u | 2u;
      }
      if (flag) {
        ep_ret = s.ret;
        ep_len = s.t;
        s.episode += 1;                                                // auto-reset: the frame below is the next episode's first
        cr_draw(s, rule.stream0 + (unsigned long long)w, G);
      }
    }
    state[w] = s;
    out.rewards[w] = reward;
    out.flags[w] = (unsigned char)flag;
    out.returns[w] = (float)ep_ret;
    out.lengths[w] = ep_len;
    out.masks[w] = (long long)((s.row > 0 ? 1 : 0) | (s.col < G - 1 ? 2 : 0) | (s.row < G - 1 ? 4 : 0) | (s.col > 0 ? 8 : 0));
    pic[0] = s.row;
    pic[1] = s.col;
    pic[2] = s.target;
    pic[3] = s.t < rule.cue_steps ? 1 : 0;
  }
  __syncthreads();
  const int ar = pic[0], ac = pic[1], target = pic[2], cue = pic[3];
  const int P = rule.P, side = G * P, row_words = side >> 2, plane_words = side * row_words;
  unsigned *dst = reinterpret_cast<unsigned *>(out.frames + (long long)w * out.pitch);
  for (int i = threadIdx.x; i < 3 * plane_words; i += CR_THREADS) {
    const int ch = i / plane_words, rem = i - ch * plane_words;
    const int y = rem / row_words, xw = rem - y * row_words;
    const int r = y / P, c = (xw << 2) / P;
    int colour = 0;
    const int k = cr_corner(r, c, G);
    if (k >= 0) colour = (cue && k == target) ? 2 : 1;
    if (r == ar && c == ac) colour = 3;
    dst[i] = cr_palette[colour][ch];
  }
}

// ---------------------------------------------------------------------------------------------------------------- CommandRoom
// environments/command_room_env.py is the ONE host definition of the rule: K commands shown one after the other (observation t of
// the episode shows command t / L while t % L < show_steps, L = show_steps + gap_steps), then executed from memory, one per step.
// Same shape as above: thread 0 advances the 32-byte state once and leaves three cell indices (mark, pointer, agent; -1: not drawn)
// in LDS, after one barrier all threads fill the frame.  The one float operation is the episode's return, float(n) * 0.1f.
constexpr int CMD_MAX_COMMANDS = 16;

struct CmdState {                      // 32 bytes per environment (etm_command_room_state_bytes)
  unsigned long long episode;
  unsigned long long commands;         // command j in bits [3 j, 3 j + 3)
  int row, col, t, n;
};
static_assert(sizeof(CmdState) == 32, "CmdState is 32 bytes");

struct CmdRule {
  int G, P, K, show_steps, L;
  unsigned long long stream0;
};

// flat colours of floor, mark, pointer, agent (command_room_env.PALETTE)
__device__ __constant__ unsigned cmd_palette[4][3] = {{20u * 0x01010101u, 24u * 0x01010101u, 40u * 0x01010101u},
                                                      {208u * 0x01010101u, 208u * 0x01010101u, 216u * 0x01010101u},
                                                      {48u * 0x01010101u, 176u * 0x01010101u, 232u * 0x01010101u},
                                                      {232u * 0x01010101u, 96u * 0x01010101u, 32u * 0x01010101u}};

__device__ __forceinline__ int cmd_dr(int a) { return a == 0 ? -1 : (a == 2 ? 1 : 0); }
__device__ __forceinline__ int cmd_dc(int a) { return a == 1 ? 1 : (a == 3 ? -1 : 0); }

// bit a set when move a (up, right, down, left, stay) keeps (r, c) on the grid
__device__ __forceinline__ unsigned cmd_valid(int r, int c, int G) {
  return (r > 0 ? 1u : 0u) | (c < G - 1 ? 2u : 0u) | (r < G - 1 ? 4u : 0u) | (c > 0 ? 8u : 0u) | 16u;
}

// (x >> 16) mod n for n = 3, 4 or 5 without a 64-bit division (a long software loop on one lane, K times per draw, while 255 threads
// wait at the barrier): the 48-bit value is hi 2^24 + lo with 24-bit halves, 2^24 = 1 mod 3 and mod 5 and 0 mod 4, so it is congruent
// to hi + lo (below 2^25) resp. lo, and the three divisors are constants.
__device__ __forceinline__ int cmd_pick(unsigned long long x, unsigned n) {
  const unsigned hi = (unsigned)(x >> 40), lo = (unsigned)(x >> 16) & 0xffffffu;
  return (int)(n == 3u ? (hi + lo) % 3u : (n == 4u ? lo & 3u : (hi + lo) % 5u));
}

__device__ __forceinline__ void cmd_draw(CmdState &s, unsigned long long stream, int G, int K) {
  const unsigned long long h = cr_splitmix64(cr_splitmix64(stream) + s.episode);
  const int start = (int)((h >> 8) % (unsigned long long)(G * G));
  s.row = start / G;
  s.col = start % G;
  s.t = 0;
  s.n = 0;
  int r = s.row, c = s.col;
  unsigned long long x = h, word = 0;
  for (int j = 0; j < K; ++j) {
    x = cr_splitmix64(x);
    const unsigned valid = cmd_valid(r, c, G);
    int pick = cmd_pick(x, (unsigned)__popc(valid));                      // the pick-th set bit of valid, from bit 0
    int a = 0;
    for (int b = 0; b < 5; ++b) {
      if (valid >> b & 1u) {
        if (pick == 0) a = b;
        --pick;
      }
    }
    word |= (unsigned long long)a << (3 * j);
    r += cmd_dr(a);
    c += cmd_dc(a);
  }
  s.commands = word;
}

template <bool RESET>
__global__ __launch_bounds__(CR_THREADS) void command_room_kernel(CmdState *__restrict__ state, const long long *__restrict__ actions,
                                                                  long long act_ld, const CmdRule rule, const EnvOut out) {
  __shared__ int pic[3];               // cell index (row-major) of the mark, the pointer and the agent; -1: not drawn
  const int w = blockIdx.x, G = rule.G, K = rule.K;
  const int show_len = K * rule.L;     // the first execute observation
  if (threadIdx.x == 0) {
    CmdState s;
    float reward = 0.f, ep_ret = 0.f;
    unsigned flag = 0;
    int ep_len = 0;
    if (RESET) {
      s.episode = 0;
      cmd_draw(s, rule.stream0 + (unsigned long long)w, G, K);
    } else {
      s = state[w];
      long long a = actions[(long long)w * act_ld];
      a = a < 0 ? 0 : (a > 4 ? 4 : a);                                 // (the host rule raises; the kernel never leaves the table)
      const int e = s.t - show_len;
      if (e >= 0) {                                                    // execute; an action on a show or gap observation is ignored
        const int cmd = e < K ? (int)(s.commands >> (3 * e) & 7ull) : -1;
        if ((int)a == cmd) {
          reward = 0.1f;
          s.row += cmd_dr(cmd);
          s.col += cmd_dc(cmd);
          s.n += 1;
          if (e == K - 1) flag = 1u | 4u;
        } else {
          flag = 1u;
        }
      }
      s.t += 1;
      if (flag) {
        ep_ret = (float)s.n * 0.1f;
        ep_len = s.t;
        s.episode += 1;                                                // auto-reset: the frame below is the next episode's first
        cmd_draw(s, rule.stream0 + (unsigned long long)w, G, K);
      }
    }
    state[w] = s;
    out.rewards[w] = reward;
    out.flags[w] = (unsigned char)flag;
    out.returns[w] = ep_ret;
    out.lengths[w] = ep_len;
    int mark = -1, pointer = -1, agent = -1;
    unsigned mask = 31u;
    if (s.t < show_len) {
      if (s.t % rule.L < rule.show_steps) {
        const int cmd = (int)(s.commands >> (3 * (s.t / rule.L)) & 7ull), mid = G >> 1;
        mark = mid * G + mid;
        if (cmd != 4) pointer = (mid + cmd_dr(cmd)) * G + mid + cmd_dc(cmd);
      }
    } else {
      agent = s.row * G + s.col;
      mask = cmd_valid(s.row, s.col, G);
    }
    out.masks[w] = (long long)mask;
    pic[0] = mark;
    pic[1] = pointer;
    pic[2] = agent;
  }
  __syncthreads();
  const int mark = pic[0], pointer = pic[1], agent = pic[2];
  const int P = rule.P, side = G * P, row_words = side >> 2, plane_words = side * row_words;
  unsigned *dst = reinterpret_cast<unsigned *>(out.frames + (long long)w * out.pitch);
  for (int i = threadIdx.x; i < 3 * plane_words; i += CR_THREADS) {
    const int ch = i / plane_words, rem = i - ch * plane_words;
    const int y = rem / row_words, xw = rem - y * row_words;
    const int cell = (y / P) * G + (xw << 2) / P;
    const int colour = cell == agent ? 3 : (cell == pointer ? 2 : (cell == mark ? 1 : 0));
    dst[i] = cmd_palette[colour][ch];
  }
}

__global__ void env_publish_kernel(long long *word, long long value) {
  __threadfence_system();
  __hip_atomic_store(word, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

inline bool cr_al(const void *p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

// What the tasks' entries validate alike, before anything is launched: pointers and their alignment, W, the geometry's frame
// size against the pitch.  -> 0 or ETM_EINVAL.
int env_check(bool reset, const void *state, const int64_t *actions, int64_t act_stride, const uint8_t *frames, int64_t frame_pitch,
              const float *rewards, const uint8_t *flags, const float *returns, const int32_t *lengths, const int64_t *masks,
              const int64_t *done_word, int W, int G, int P) {
  if (!state || !frames || !rewards || !flags || !returns || !lengths || !masks || W < 1) return ETM_EINVAL;
  if (!reset && (!actions || act_stride < 1 || !cr_al(actions, 8))) return ETM_EINVAL;
  if (!etm_cue_room_supported(G, P)) return ETM_EINVAL;
  if (!cr_al(state, 8) || !cr_al(frames, 4) || !cr_al(rewards, 4) || !cr_al(returns, 4) || !cr_al(lengths, 4) || !cr_al(masks, 8) ||
      !cr_al(done_word, 8))
    return ETM_EINVAL;
  const int64_t frame_bytes = 3ll * G * P * G * P;
  if (frame_pitch < frame_bytes || (frame_pitch & 3) != 0) return ETM_EINVAL;
  return 0;
}

// Behind a step's launch: its status, then (optionally) the completion word by a one-thread launch on the same stream.
int env_publish(int64_t *done_word, int64_t done_value, hipStream_t st) {
  int rc = etm_launch_status();
  if (rc || !done_word) return rc;
  hipLaunchKernelGGL(env_publish_kernel, dim3(1), dim3(1), 0, st, (long long *)done_word, (long long)done_value);
  return etm_launch_status();
}

int cr_launch(bool reset, void *state, const int64_t *actions, int64_t act_stride, uint8_t *frames, int64_t frame_pitch, float *rewards,
              uint8_t *flags, float *returns, int32_t *lengths, int64_t *masks, int64_t *done_word, int64_t done_value, int W, int G, int P,
              int cue_steps, int max_steps, int64_t stream0, void *stream) {
  (void)hipGetLastError();
  if (env_check(reset, state, actions, act_stride, frames, frame_pitch, rewards, flags, returns, lengths, masks, done_word, W, G, P) ||
      cue_steps < 1 || max_steps < 1)
    return ETM_EINVAL;
  const CueRule rule{G, P, cue_steps, max_steps, (unsigned long long)stream0};
  const EnvOut out{frames, (long long)frame_pitch, rewards, flags, returns, lengths, (long long *)masks};
  hipStream_t st = (hipStream_t)stream;
  if (reset)
    hipLaunchKernelGGL(cue_room_kernel<true>, dim3((unsigned)W), dim3(CR_THREADS), 0, st, (CueState *)state, (const long long *)nullptr, 0ll,
                       rule, out);
  else
    hipLaunchKernelGGL(cue_room_kernel<false>, dim3((unsigned)W), dim3(CR_THREADS), 0, st, (CueState *)state, (const long long *)actions,
                       (long long)act_stride, rule, out);
  return env_publish(done_word, done_value, st);
}

int cmd_launch(bool reset, void *state, const int64_t *actions, int64_t act_stride, uint8_t *frames, int64_t frame_pitch, float *rewards,
               uint8_t *flags, float *returns, int32_t *lengths, int64_t *masks, int64_t *done_word, int64_t done_value, int W, int G, int P,
               int K, int show_steps, int gap_steps, int64_t stream0, void *stream) {
  (void)hipGetLastError();
  if (env_check(reset, state, actions, act_stride, frames, frame_pitch, rewards, flags, returns, lengths, masks, done_word, W, G, P) ||
      !etm_command_room_supported(G, P, K) || show_steps < 1 || gap_steps < 0 ||
      (long long)K * ((long long)show_steps + gap_steps) + K > 0x7fffffffll)
    return ETM_EINVAL;
  const CmdRule rule{G, P, K, show_steps, show_steps + gap_steps, (unsigned long long)stream0};
  const EnvOut out{frames, (long long)frame_pitch, rewards, flags, returns, lengths, (long long *)masks};
  hipStream_t st = (hipStream_t)stream;
  if (reset)
    hipLaunchKernelGGL(command_room_kernel<true>, dim3((unsigned)W), dim3(CR_THREADS), 0, st, (CmdState *)state, (const long long *)nullptr,
                       0ll, rule, out);
  else
    hipLaunchKernelGGL(command_room_kernel<false>, dim3((unsigned)W), dim3(CR_THREADS), 0, st, (CmdState *)state,
                       (const long long *)actions, (long long)act_stride, rule, out);
  return env_publish(done_word, done_value, st);
}
}  // namespace

extern "C" int etm_cue_room_supported(int G, int P) {
  return G >= 3 && G <= CR_MAX_GRID && (G & 1) == 1 && P >= 4 && P <= CR_MAX_CELL && (P & 3) == 0 ? 1 : 0;
}

extern "C" int etm_command_room_supported(int G, int P, int K) {
  return etm_cue_room_supported(G, P) && K >= 1 && K <= CMD_MAX_COMMANDS ? 1 : 0;
}

extern "C" int64_t etm_command_room_state_bytes(int W) { return W < 1 ? 0 : (int64_t)W * (int64_t)sizeof(CmdState); }

extern "C" int etm_command_room_reset(void *state, uint8_t *frames, int64_t frame_pitch, float *rewards, uint8_t *flags, float *returns,
                                      int32_t *lengths, int64_t *masks, int64_t *done_word, int64_t done_value, int W, int G, int P,
                                      int K, int show_steps, int gap_steps, int64_t stream0, void *stream) {
  return cmd_launch(true, state, nullptr, 0, frames, frame_pitch, rewards, flags, returns, lengths, masks, done_word, done_value, W, G, P,
                    K, show_steps, gap_steps, stream0, stream);
}

extern "C" int etm_command_room_step(void *state, const int64_t *actions, int64_t act_stride, uint8_t *frames, int64_t frame_pitch,
                                     float *rewards, uint8_t *flags, float *returns, int32_t *lengths, int64_t *masks,
                                     int64_t *done_word, int64_t done_value, int W, int G, int P, int K, int show_steps, int gap_steps,
                                     int64_t stream0, void *stream) {
  return cmd_launch(false, state, actions, act_stride, frames, frame_pitch, rewards, flags, returns, lengths, masks, done_word,
                    done_value, W, G, P, K, show_steps, gap_steps, stream0, stream);
}

extern "C" int64_t etm_cue_room_state_bytes(int W) { return W < 1 ? 0 : (int64_t)W * (int64_t)sizeof(CueState); }

extern "C" int etm_cue_room_reset(void *state, uint8_t *frames, int64_t frame_pitch, float *rewards, uint8_t *flags, float *returns,
                                  int32_t *lengths, int64_t *masks, int64_t *done_word, int64_t done_value, int W, int G, int P,
                                  int cue_steps, int max_steps, int64_t stream0, void *stream) {
  return cr_launch(true, state, nullptr, 0, frames, frame_pitch, rewards, flags, returns, lengths, masks, done_word, done_value, W, G, P,
                   cue_steps, max_steps, stream0, stream);
}

extern "C" int etm_cue_room_step(void *state, const int64_t *actions, int64_t act_stride, uint8_t *frames, int64_t frame_pitch,
                                 float *rewards, uint8_t *flags, float *returns, int32_t *lengths, int64_t *masks, int64_t *done_word,
                                 int64_t done_value, int W, int G, int P, int cue_steps, int max_steps, int64_t stream0, void *stream) {
  return cr_launch(false, state, actions, act_stride, frames, frame_pitch, rewards, flags, returns, lengths, masks, done_word, done_value,
                   W, G, P, cue_steps, max_steps, stream0, stream);
}
