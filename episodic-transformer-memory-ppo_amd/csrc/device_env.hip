// Device-resident environments: grid-room tasks stepped, auto-reset and rendered by one launch per worker group and step.  ONE kernel
// skeleton (env_kernel) and one launcher (env_launch) serve every task; a task is a stateless struct of static functions that says
// what is its own -- state, rule words, draw, advance, picture, colour (CueRoom, CommandRoom, PathRoom and SpotRoom below; the ONE host
// definition of each rule is environments/cue_room_env.py, command_room_env.py, path_room_env.py resp. spot_room_env.py).
// What the skeleton keeps, whatever the task:
//   * one workgroup of 256 threads per environment, grid = W; no dependence on launch geometry, no atomics, no inline assembly: two
//     calls from equal state give equal bytes;
//   * only thread 0 of workgroup w touches state[w], once per launch: it reads the 32-byte state and the action, clamps the action
//     into the task's table (the host rule raises), advances, starts the next episode where the step ended one (the frame is then
//     the next episode's first), stores the state and writes the five result words and the mask;
//   * thread 0 leaves the few ints the picture depends on in LDS (at most 16 bytes); after exactly ONE __syncthreads() all threads
//     fill the frame of the NEW state with 4-byte vector stores from plain C++ (cell % 4 == 0: a word never straddles two cells);
//   * integer arithmetic throughout; a task's reward constant and its episode return are the only floats;
//   * the rule structs are kernel arguments, uniform per wave.
// The episode draw starts from env_hash: splitmix64 of splitmix64(stream) + episode in uint64 (environments/grid_room.episode_hash).
// The completion word (optional) is a second, one-thread launch behind the step on the same stream: the workgroups of the step have
// no arrival counter (that would be an atomic), so "everything is written" is the stream's order; the store itself is the sampling
// kernels' hand-over (one system-scope fence, then a system-scope release store).
#include "etm_common.h"

namespace {
constexpr int ENV_THREADS = 256;
constexpr int ENV_MAX_GRID = 31, ENV_MAX_CELL = 64;

struct EnvOut {                        // the output record of every task here
  unsigned char *frames;               // environment w's frame at frames + w * pitch: [3, G P, G P] bytes
  long long pitch;
  float *rewards;                      // [W]
  unsigned char *flags;                // [W]: bit 0 done, bit 1 truncated, bit 2 success
  float *returns;                      // [W]: the return of the episode that ended (else 0)
  int *lengths;                        // [W]: its length (else 0)
  long long *masks;                    // [W]: bit a set when move a stays on the grid, for the frame written
};

__device__ __forceinline__ unsigned long long env_splitmix64(unsigned long long x) {
  unsigned long long z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ unsigned long long env_hash(unsigned long long stream, unsigned long long episode) {
  return env_splitmix64(env_splitmix64(stream) + episode);
}

// (row, column) steps of the moves up, right, down, left (and stay: none)
__device__ __forceinline__ int env_dr(int a) { return a == 0 ? -1 : (a == 2 ? 1 : 0); }
__device__ __forceinline__ int env_dc(int a) { return a == 1 ? 1 : (a == 3 ? -1 : 0); }

// bit a set when move a (up, right, down, left) keeps (r, c) on the grid
__device__ __forceinline__ unsigned env_on_grid(int r, int c, int G) {
  return (r > 0 ? 1u : 0u) | (c < G - 1 ? 2u : 0u) | (r < G - 1 ? 4u : 0u) | (c > 0 ? 8u : 0u);
}

inline bool env_grid_ok(int G, int P) {
  return G >= 3 && G <= ENV_MAX_GRID && (G & 1) == 1 && P >= 4 && P <= ENV_MAX_CELL && (P & 3) == 0;
}

// ---------------------------------------------------------------------------------------------------------------- CueRoom
// The four corners are goals, one of them the episode's target, drawn in the cue colour in the first cue_steps observations.
// flat colours (R, G, B) of floor, goal, cue, agent, one byte per channel replicated over a 4-byte word (cue_room_env.PALETTE)
__device__ __constant__ unsigned cue_palette[4][3] = {{24u * 0x01010101u, 24u * 0x01010101u, 32u * 0x01010101u},
                                                      {64u * 0x01010101u, 160u * 0x01010101u, 64u * 0x01010101u},
                                                      {240u * 0x01010101u, 208u * 0x01010101u, 32u * 0x01010101u},
                                                      {224u * 0x01010101u, 48u * 0x01010101u, 48u * 0x01010101u}};

struct CueRoom {
  struct State {                       // 32 bytes per environment (etm_cue_room_state_bytes)
    unsigned long long episode;
    int row, col, t, target, ret, pad;
  };
  struct Rule {
    int G, P, cue_steps, max_steps;
    unsigned long long stream0;        // seed + first worker id; environment w draws from stream0 + w
  };
  static constexpr int ACTIONS = 4;
  static constexpr int PIC = 4;        // agent row, agent column, target, cue visible

  static bool rule_ok(const Rule &rule) { return rule.cue_steps >= 1 && rule.max_steps >= 1; }

  // corner k of cell (r, c): 0 top left, 1 top right, 2 bottom right, 3 bottom left; -1: no corner
  static __device__ __forceinline__ int corner(int r, int c, int G) {
    if (r == 0) return c == 0 ? 0 : (c == G - 1 ? 1 : -1);
    if (r == G - 1) return c == G - 1 ? 2 : (c == 0 ? 3 : -1);
    return -1;
  }

  static __device__ __forceinline__ void draw(State &s, unsigned long long stream, const Rule &rule) {
    const int G = rule.G;
    const unsigned long long h = env_hash(stream, s.episode);
    s.target = (int)(h & 3ull);
    int c = (int)((h >> 8) % (unsigned long long)(G * G - 4)) + 1;      // row-major, the corners skipped
    if (c >= G - 1) ++c;
    if (c >= G * (G - 1)) ++c;
    s.row = c / G;
    s.col = c % G;
    s.ret = 0;
  }

  // (the skeleton counts s.t up behind this: s.t + 1 is the step this action ends)
  static __device__ __forceinline__ void advance(State &s, int a, const Rule &rule, float &reward, unsigned &flag) {
    const int G = rule.G, r = s.row + env_dr(a), c = s.col + env_dc(a);
    if (r >= 0 && r < G && c >= 0 && c < G) {
      s.row = r;
      s.col = c;
    }
    const int k = corner(s.row, s.col, G);
    if (k >= 0) {
      const bool hit = k == s.target;
      if (hit) {
        reward = 1.f;
        s.ret += 1;
      }
      flag = 1u | (hit ? 4u : 0u);
    } else if (s.t + 1 >= rule.max_steps) {
      flag = 1u | 2u;
    }
  }

  static __device__ __forceinline__ float episode_return(const State &s) { return (float)s.ret; }

  static __device__ __forceinline__ void picture(const State &s, const Rule &rule, int *pic, unsigned &mask) {
    mask = env_on_grid(s.row, s.col, rule.G);
    pic[0] = s.row;
    pic[1] = s.col;
    pic[2] = s.target;
    pic[3] = s.t < rule.cue_steps ? 1 : 0;
  }

  static __device__ __forceinline__ unsigned colour(int r, int c, const int *pic, int G, int ch) {
    int colour = 0;
    const int k = corner(r, c, G);
    if (k >= 0) colour = (pic[3] && k == pic[2]) ? 2 : 1;
    if (r == pic[0] && c == pic[1]) colour = 3;
    return cue_palette[colour][ch];
  }
};

// ---------------------------------------------------------------------------------------------------------------- CommandRoom
// K commands shown one after the other (observation t of the episode shows command t / L while t % L < show_steps, L = show_steps +
// gap_steps), then executed from memory, one per step; an action on a show or gap observation is ignored.
constexpr int CMD_MAX_COMMANDS = 16;

// flat colours of floor, mark, pointer, agent (command_room_env.PALETTE)
__device__ __constant__ unsigned cmd_palette[4][3] = {{20u * 0x01010101u, 24u * 0x01010101u, 40u * 0x01010101u},
                                                      {208u * 0x01010101u, 208u * 0x01010101u, 216u * 0x01010101u},
                                                      {48u * 0x01010101u, 176u * 0x01010101u, 232u * 0x01010101u},
                                                      {232u * 0x01010101u, 96u * 0x01010101u, 32u * 0x01010101u}};

struct CommandRoom {
  struct State {                       // 32 bytes per environment (etm_command_room_state_bytes)
    unsigned long long episode;
    unsigned long long commands;       // command j in bits [3 j, 3 j + 3)
    int row, col, t, n;
  };
  struct Rule {
    int G, P, K, show_steps, gap_steps;
    unsigned long long stream0;
  };
  static constexpr int ACTIONS = 5;
  static constexpr int PIC = 3;        // cell index (row-major) of the mark, the pointer and the agent; -1: not drawn

  static bool rule_ok(const Rule &rule) {
    return rule.K >= 1 && rule.K <= CMD_MAX_COMMANDS && rule.show_steps >= 1 && rule.gap_steps >= 0 &&
           (long long)rule.K * ((long long)rule.show_steps + rule.gap_steps) + rule.K <= 0x7fffffffll;
  }

  // (x >> 16) mod n for n = 3, 4 or 5 without a 64-bit division (a long software loop on one lane, K times per draw, while 255 threads
  // wait at the barrier): the 48-bit value is hi 2^24 + lo with 24-bit halves, 2^24 = 1 mod 3 and mod 5 and 0 mod 4, so it is congruent
  // to hi + lo (below 2^25) resp. lo, and the three divisors are constants.
  static __device__ __forceinline__ int pick_of(unsigned long long x, unsigned n) {
    const unsigned hi = (unsigned)(x >> 40), lo = (unsigned)(x >> 16) & 0xffffffu;
    return (int)(n == 3u ? (hi + lo) % 3u : (n == 4u ? lo & 3u : (hi + lo) % 5u));
  }

  static __device__ __forceinline__ void draw(State &s, unsigned long long stream, const Rule &rule) {
    const int G = rule.G;
    const unsigned long long h = env_hash(stream, s.episode);
    const int start = (int)((h >> 8) % (unsigned long long)(G * G));
    s.row = start / G;
    s.col = start % G;
    s.n = 0;
    int r = s.row, c = s.col;
    unsigned long long x = h, word = 0;
    for (int j = 0; j < rule.K; ++j) {
      x = env_splitmix64(x);
      const unsigned valid = env_on_grid(r, c, G) | 16u;
      int pick = pick_of(x, (unsigned)__popc(valid));                      // the pick-th set bit of valid, from bit 0
      int a = 0;
      for (int b = 0; b < 5; ++b) {
        if (valid >> b & 1u) {
          if (pick == 0) a = b;
          --pick;
        }
      }
      word |= (unsigned long long)a << (3 * j);
      r += env_dr(a);
      c += env_dc(a);
    }
    s.commands = word;
  }

  static __device__ __forceinline__ int show_length(const Rule &rule) {    // the first execute observation
    return rule.K * (rule.show_steps + rule.gap_steps);
  }

  static __device__ __forceinline__ void advance(State &s, int a, const Rule &rule, float &reward, unsigned &flag) {
    const int K = rule.K, e = s.t - show_length(rule);
    if (e >= 0) {
      const int cmd = e < K ? (int)(s.commands >> (3 * e) & 7ull) : -1;
      if (a == cmd) {
        reward = 0.1f;
        s.row += env_dr(cmd);
        s.col += env_dc(cmd);
        s.n += 1;
        if (e == K - 1) flag = 1u | 4u;
      } else {
        flag = 1u;
      }
    }
  }

  static __device__ __forceinline__ float episode_return(const State &s) { return (float)s.n * 0.1f; }

  static __device__ __forceinline__ void picture(const State &s, const Rule &rule, int *pic, unsigned &mask) {
    const int G = rule.G, L = rule.show_steps + rule.gap_steps;
    int mark = -1, pointer = -1, agent = -1;
    mask = 31u;
    if (s.t < show_length(rule)) {
      if (s.t % L < rule.show_steps) {
        const int cmd = (int)(s.commands >> (3 * (s.t / L)) & 7ull), mid = G >> 1;
        mark = mid * G + mid;
        if (cmd != 4) pointer = (mid + env_dr(cmd)) * G + mid + env_dc(cmd);
      }
    } else {
      agent = s.row * G + s.col;
      mask = env_on_grid(s.row, s.col, G) | 16u;
    }
    pic[0] = mark;
    pic[1] = pointer;
    pic[2] = agent;
  }

  static __device__ __forceinline__ unsigned colour(int r, int c, const int *pic, int G, int ch) {
    const int cell = r * G + c;
    return cmd_palette[cell == pic[2] ? 3 : (cell == pic[1] ? 2 : (cell == pic[0] ? 1 : 0))][ch];
  }
};

// ---------------------------------------------------------------------------------------------------------------- PathRoom
// An invisible path of at most M moves (up, right, down) from an origin in column 0; a move onto a path cell pays the progress beyond
// the best index reached, the goal 10 tenths more, a move onto any other cell is a fall back to the origin (the cell is the mark of
// the next observation only).  Whether a cell is on the path, and its index, is a walk over the packed moves: integer adds.
constexpr int PATH_MAX_MOVES = 32;

// flat colours of floor, goal, mark, agent (path_room_env.PALETTE)
__device__ __constant__ unsigned path_palette[4][3] = {{28u * 0x01010101u, 28u * 0x01010101u, 36u * 0x01010101u},
                                                       {64u * 0x01010101u, 192u * 0x01010101u, 96u * 0x01010101u},
                                                       {232u * 0x01010101u, 64u * 0x01010101u, 200u * 0x01010101u},
                                                       {240u * 0x01010101u, 200u * 0x01010101u, 48u * 0x01010101u}};

struct PathRoom {
  struct State {                       // 32 bytes per environment (etm_path_room_state_bytes)
    unsigned long long episode;
    unsigned long long path;           // move j (0 up, 1 right, 2 down) in bits [2 j, 2 j + 2)
    int agent, t, best;                // a cell is row << 5 | column here (G <= 31): no division by G in the step
    unsigned places;                   // origin row in bits [0, 5), n in [5, 11), the goal cell in [11, 21), the mark cell + 1 in [21, 32)
  };
  struct Rule {
    int G, P, M, max_steps;
    unsigned long long stream0;
  };
  static constexpr int ACTIONS = 4;
  static constexpr int PIC = 3;        // cell index (row-major) of the goal, the mark and the agent; -1: not drawn

  static bool rule_ok(const Rule &rule) { return rule.M >= 1 && rule.M <= PATH_MAX_MOVES && rule.max_steps >= 1; }

  static __device__ __forceinline__ int origin_of(const State &s) { return (int)(s.places & 31u); }
  static __device__ __forceinline__ int moves_of(const State &s) { return (int)(s.places >> 5 & 63u); }
  static __device__ __forceinline__ int goal_of(const State &s) { return (int)(s.places >> 11 & 1023u); }

  // (x >> 16) mod n for n = 1, 2 or 3 without a 64-bit division, as CommandRoom::pick_of: 2^24 = 1 mod 3, and mod 2 is a bit
  static __device__ __forceinline__ int pick_of(unsigned long long x, int n) {
    const unsigned hi = (unsigned)(x >> 40), lo = (unsigned)(x >> 16) & 0xffffffu;
    return (int)(n == 3 ? (hi + lo) % 3u : (n == 2 ? lo & 1u : 0u));
  }

  static __device__ __forceinline__ void draw(State &s, unsigned long long stream, const Rule &rule) {
    const int G = rule.G;
    const unsigned long long h = env_hash(stream, s.episode);
    const int origin = (int)((h >> 8) % (unsigned long long)G);
    int r = origin, c = 0, previous = -1, n = 0;
    unsigned long long x = h, word = 0;
    for (int j = 0; j < rule.M && c < G - 1; ++j) {
      x = env_splitmix64(x);
      const int up = (r > 0 && previous != 2) ? 1 : 0, down = (r < G - 1 && previous != 0) ? 1 : 0;
      // the candidates (up, right, down) with up and / or down left out: entry pick is move pick, or pick + 1 where up is left out
      const int a = pick_of(x, 1 + up + down) + 1 - up;
      word |= (unsigned long long)a << (2 * j);
      r += env_dr(a);
      c += env_dc(a);
      previous = a;
      n = j + 1;
    }
    s.path = word;
    s.agent = origin << 5;
    s.best = 0;
    s.places = (unsigned)origin | (unsigned)n << 5 | (unsigned)(r << 5 | c) << 11;        // no mark
  }

  static __device__ __forceinline__ void advance(State &s, int a, const Rule &rule, float &reward, unsigned &flag) {
    const int G = rule.G, origin = origin_of(s), n = moves_of(s);
    const int r = (s.agent >> 5) + env_dr(a), c = (s.agent & 31) + env_dc(a);
    int k = 0;
    s.places &= 0x1fffffu;                                                 // the mark lasts one observation
    if (r >= 0 && r < G && c >= 0 && c < G) {
      const int target = r << 5 | c;
      int cell = origin << 5, index = cell == target ? 0 : -1;           // the path visits no cell twice: at most one match
      unsigned long long word = s.path;
      for (int j = 1; j <= n; ++j) {
        const int m = (int)(word & 3ull);
        word >>= 2;
        cell += env_dr(m) * 32 + env_dc(m);
        if (cell == target) index = j;
      }
      if (index >= 0) {
        s.agent = target;
        k = index > s.best ? index - s.best : 0;
        if (index > s.best) s.best = index;
        if (index == n) {
          k += 10;
          flag = 1u | 4u;
        }
      } else {                                                             // a fall: back to the origin, the cell marked
        s.agent = origin << 5;
        s.places |= (unsigned)(target + 1) << 21;
      }
    }
    if (!flag && s.t + 1 >= rule.max_steps) flag = 1u | 2u;
    reward = (float)k * 0.1f;
  }

  // (the agent stands on the goal only in the step that ends the episode there)
  static __device__ __forceinline__ float episode_return(const State &s) {
    return (float)(s.best + (s.agent == goal_of(s) ? 10 : 0)) * 0.1f;
  }

  static __device__ __forceinline__ int index_of(int cell, int G) { return (cell >> 5) * G + (cell & 31); }

  static __device__ __forceinline__ void picture(const State &s, const Rule &rule, int *pic, unsigned &mask) {
    const int G = rule.G, mark = (int)(s.places >> 21);
    mask = env_on_grid(s.agent >> 5, s.agent & 31, G);
    pic[0] = index_of(goal_of(s), G);
    pic[1] = mark ? index_of(mark - 1, G) : -1;
    pic[2] = index_of(s.agent, G);
  }

  static __device__ __forceinline__ unsigned colour(int r, int c, const int *pic, int G, int ch) {
    const int cell = r * G + c;
    return path_palette[cell == pic[2] ? 3 : (cell == pic[1] ? 2 : (cell == pic[0] ? 1 : 0))][ch];
  }
};

// ---------------------------------------------------------------------------------------------------------------- SpotRoom
// A coin, then an exit, in a room that is dark from observation light_steps on; N <= 4 spotlights sweep a lane each as a triangle
// wave and light the 3 x 3 block around their centre.  The agent is drawn only where a spotlight is on it, and that costs health.
// The picture depends on time: the state carries the wave's common offset (step, wave) counted up, so the step divides by nothing.
constexpr int SPOT_MAX_LIGHTS = 4, SPOT_MAX_HEALTH = 15;
constexpr int SPOT_COIN_TENTHS = 5, SPOT_EXIT_TENTHS = 10;
constexpr unsigned SPOT_NOT_DRAWN = 1023u, SPOT_NO_CENTRE = 0x6464u;      // (row 100, column 100: no cell is within 1 of it)

// flat colours of dark floor, lit floor, coin, exit, agent (spot_room_env.PALETTE)
__device__ __constant__ unsigned spot_palette[5][3] = {{12u * 0x01010101u, 12u * 0x01010101u, 20u * 0x01010101u},
                                                       {96u * 0x01010101u, 92u * 0x01010101u, 72u * 0x01010101u},
                                                       {248u * 0x01010101u, 208u * 0x01010101u, 40u * 0x01010101u},
                                                       {56u * 0x01010101u, 176u * 0x01010101u, 112u * 0x01010101u},
                                                       {224u * 0x01010101u, 64u * 0x01010101u, 200u * 0x01010101u}};

struct SpotRoom {
  struct State {                       // 32 bytes per environment (etm_spot_room_state_bytes)
    unsigned long long episode;
    unsigned long long spots;          // spotlight i in bits [12 i, 12 i + 12): axis 1, lane 5, phase 6
    int agent, t;                      // a cell is row << 5 | column here (G <= 31)
    unsigned places;                   // the coin cell in bits [0, 10), the exit cell in [10, 20), health LOST in [20, 24), coin taken in
                                       // bit 24, wave = ((t - light_steps) div spot_period) mod (2 G - 2) in [25, 31) (0 while t < light_steps)
    int rest;                          // (t - light_steps) mod spot_period: the steps the spotlights have rested (0 while t < light_steps)
  };
  struct Rule {
    int G, P, N, light_steps, spot_period, health, max_steps;
    unsigned long long stream0;
  };
  static constexpr int ACTIONS = 5;
  static constexpr int PIC = 3;        // [0]: agent, coin, exit cell in 10 bits each (1023: not drawn), bit 30: all floor lit;
                                       // [1], [2]: the four centres, row | column << 8 in 16 bits each (SPOT_NO_CENTRE: none)

  static bool rule_ok(const Rule &rule) {
    return rule.N >= 0 && rule.N <= SPOT_MAX_LIGHTS && rule.light_steps >= 1 && rule.spot_period >= 1 && rule.health >= 1 &&
           rule.health <= SPOT_MAX_HEALTH && rule.max_steps >= 1;
  }

  static __device__ __forceinline__ int coin_of(const State &s) { return (int)(s.places & 1023u); }
  static __device__ __forceinline__ int exit_of(const State &s) { return (int)(s.places >> 10 & 1023u); }
  static __device__ __forceinline__ int lost_of(const State &s) { return (int)(s.places >> 20 & 15u); }
  static __device__ __forceinline__ bool taken_of(const State &s) { return (s.places >> 24 & 1u) != 0; }
  static __device__ __forceinline__ int wave_of(const State &s) { return (int)(s.places >> 25 & 63u); }

  static __device__ __forceinline__ int cell_of(unsigned index, unsigned G) {      // row-major index -> row << 5 | column
    const unsigned r = index / G;
    return (int)(r << 5 | (index - r * G));
  }

  // the start, the coin and the exit are three remainders of 24-bit fields by G^2, G^2 - 1, G^2 - 2, a spotlight's lane and phase two
  // of 16-bit fields: 32-bit divisions all, and only where an episode starts
  static __device__ __forceinline__ void draw(State &s, unsigned long long stream, const Rule &rule) {
    const unsigned G = (unsigned)rule.G, cells = G * G;
    const unsigned long long h = env_hash(stream, s.episode);
    const unsigned start = ((unsigned)(h >> 8) & 0xffffffu) % cells;
    unsigned long long x = env_splitmix64(h);
    unsigned coin = ((unsigned)(x >> 16) & 0xffffffu) % (cells - 1u);    // entry of the cells without the start
    if (coin >= start) ++coin;
    x = env_splitmix64(x);
    unsigned leave = ((unsigned)(x >> 16) & 0xffffffu) % (cells - 2u);   // entry of the cells without the start and the coin
    const unsigned lo = start < coin ? start : coin, hi = start < coin ? coin : start;
    if (leave >= lo) ++leave;
    if (leave >= hi) ++leave;
    unsigned long long word = 0;
    for (int i = 0; i < rule.N; ++i) {
      x = env_splitmix64(x);
      const unsigned axis = (unsigned)(x >> 16) & 1u, lane = ((unsigned)(x >> 20) & 0xffffu) % G;
      const unsigned phase = ((unsigned)(x >> 40) & 0xffffu) % (2u * G - 2u);
      word |= (unsigned long long)(axis | lane << 1 | phase << 6) << (12 * i);
    }
    s.spots = word;
    s.agent = cell_of(start, G);
    s.places = (unsigned)cell_of(coin, G) | (unsigned)cell_of(leave, G) << 10;      // nothing lost, coin not taken, wave 0
    s.rest = 0;
  }

  // centre of spotlight i, row | column << 8, with the wave's common offset
  static __device__ __forceinline__ unsigned centre(unsigned long long spots, int i, int wave, int G) {
    const unsigned bits = (unsigned)(spots >> (12 * i)) & 0xfffu;
    int q = (int)(bits >> 6) + wave;                                       // both below 2 G - 2
    if (q >= 2 * G - 2) q -= 2 * G - 2;
    const unsigned pos = (unsigned)(q < G ? q : 2 * G - 2 - q), lane = bits >> 1 & 31u;
    return (bits & 1u) ? (pos | lane << 8) : (lane | pos << 8);
  }

  static __device__ __forceinline__ bool in_box(int r, int c, unsigned centre16) {
    return (unsigned)(r - (int)(centre16 & 255u) + 1) <= 2u && (unsigned)(c - (int)(centre16 >> 8 & 255u) + 1) <= 2u;
  }

  // whether a spotlight is on ``cell`` with the wave at ``wave`` (the caller knows that the spotlights are active)
  static __device__ __forceinline__ bool lit(const State &s, int cell, int wave, const Rule &rule) {
    bool on = false;
    for (int i = 0; i < rule.N; ++i) on = on || in_box(cell >> 5, cell & 31, centre(s.spots, i, wave, rule.G));
    return on;
  }

  // (the skeleton counts s.t up behind this: s.t + 1 is the observation this action leads to)
  static __device__ __forceinline__ void advance(State &s, int a, const Rule &rule, float &reward, unsigned &flag) {
    const int G = rule.G, r = (s.agent >> 5) + env_dr(a), c = (s.agent & 31) + env_dc(a);
    int k = 0;
    if (r >= 0 && r < G && c >= 0 && c < G) s.agent = r << 5 | c;
    if (s.agent == coin_of(s) && !taken_of(s)) {
      s.places |= 1u << 24;
      k += SPOT_COIN_TENTHS;
    }
    // the spotlights of observation t + 1: they rest spot_period observations on a cell, from observation light_steps on
    int wave = wave_of(s);
    if (s.t >= rule.light_steps) {
      s.rest += 1;
      if (s.rest >= rule.spot_period) {
        s.rest = 0;
        wave = wave + 1 >= 2 * G - 2 ? 0 : wave + 1;
        s.places = (s.places & ~(63u << 25)) | (unsigned)wave << 25;
      }
    }
    if (s.agent == exit_of(s) && taken_of(s)) {
      k += SPOT_EXIT_TENTHS;
      flag = 1u | 4u;
    } else if (s.t + 1 >= rule.light_steps && lit(s, s.agent, wave, rule)) {
      s.places += 1u << 20;
      k -= 1;
      if (lost_of(s) >= rule.health) flag = 1u;
    }
    if (!flag && s.t + 1 >= rule.max_steps) flag = 1u | 2u;
    reward = (float)k * 0.1f;
  }

  // (the agent stands on the exit with the coin taken only in the step that ends the episode there)
  static __device__ __forceinline__ float episode_return(const State &s) {
    const int taken = taken_of(s) ? 1 : 0;
    return (float)(SPOT_COIN_TENTHS * taken + (taken && s.agent == exit_of(s) ? SPOT_EXIT_TENTHS : 0) - lost_of(s)) * 0.1f;
  }

  static __device__ __forceinline__ void picture(const State &s, const Rule &rule, int *pic, unsigned &mask) {
    const int G = rule.G, wave = wave_of(s);
    const bool light = s.t < rule.light_steps;
    mask = env_on_grid(s.agent >> 5, s.agent & 31, G) | 16u;
    unsigned centres[SPOT_MAX_LIGHTS];
    for (int i = 0; i < SPOT_MAX_LIGHTS; ++i) centres[i] = (!light && i < rule.N) ? centre(s.spots, i, wave, G) : SPOT_NO_CENTRE;
    bool seen = light;
    for (int i = 0; i < SPOT_MAX_LIGHTS; ++i) seen = seen || in_box(s.agent >> 5, s.agent & 31, centres[i]);
    pic[0] = (int)((seen ? (unsigned)s.agent : SPOT_NOT_DRAWN) | (taken_of(s) ? SPOT_NOT_DRAWN : (unsigned)coin_of(s)) << 10 |
                   (unsigned)exit_of(s) << 20 | (light ? 1u << 30 : 0u));
    pic[1] = (int)(centres[0] | centres[1] << 16);
    pic[2] = (int)(centres[2] | centres[3] << 16);
  }

  // bits x .. x + 2 of a word whose bit k + 1 stands for row (column) k: the three rows (columns) around x; none for no centre
  static __device__ __forceinline__ unsigned span(unsigned x) { return x < 31u ? 7u << x : 0u; }

  // (the spans depend on the picture alone: the frame loop keeps them in registers, and a word costs two shifts and an AND per box)
  static __device__ __forceinline__ unsigned colour(int r, int c, const int *pic, int, int ch) {
    const unsigned places = (unsigned)pic[0], first = (unsigned)pic[1], second = (unsigned)pic[2], cell = (unsigned)(r << 5 | c);
    const unsigned on = (places >> 30 | ((span(first & 255u) >> (r + 1)) & (span(first >> 8 & 255u) >> (c + 1))) |
                         ((span(first >> 16 & 255u) >> (r + 1)) & (span(first >> 24) >> (c + 1))) |
                         ((span(second & 255u) >> (r + 1)) & (span(second >> 8 & 255u) >> (c + 1))) |
                         ((span(second >> 16 & 255u) >> (r + 1)) & (span(second >> 24) >> (c + 1)))) & 1u;
    int colour = (int)on;
    if (cell == (places >> 10 & 1023u)) colour = 2;
    if (cell == (places >> 20 & 1023u)) colour = 3;
    if (cell == (places & 1023u)) colour = 4;
    return spot_palette[colour][ch];
  }
};

// ---------------------------------------------------------------------------------------------------------------- the skeleton
template <class Task, bool RESET>
__global__ __launch_bounds__(ENV_THREADS) void env_kernel(typename Task::State *__restrict__ state, const long long *__restrict__ actions,
                                                          long long act_ld, const typename Task::Rule rule, const EnvOut out) {
  static_assert(sizeof(typename Task::State) == 32, "a task's state is 32 bytes");
  static_assert(Task::PIC <= 4, "at most 16 bytes of LDS");
  __shared__ int pic[Task::PIC];
  const int w = blockIdx.x, G = rule.G;
  if (threadIdx.x == 0) {
    typename Task::State s;
    float reward = 0.f, ep_ret = 0.f;
    unsigned flag = 0, mask;
    int ep_len = 0;
    const unsigned long long stream = rule.stream0 + (unsigned long long)w;
    if (RESET) {
      s = typename Task::State{};
      Task::draw(s, stream, rule);
    } else {
      s = state[w];
      long long a = actions[(long long)w * act_ld];
      a = a < 0 ? 0 : (a > Task::ACTIONS - 1 ? Task::ACTIONS - 1 : a);
      Task::advance(s, (int)a, rule, reward, flag);
      s.t += 1;
      if (flag) {
        ep_ret = Task::episode_return(s);
        ep_len = s.t;
        s.episode += 1;                                                  // auto-reset: the frame below is the next episode's first
        s.t = 0;
        Task::draw(s, stream, rule);
      }
    }
    state[w] = s;
    out.rewards[w] = reward;
    out.flags[w] = (unsigned char)flag;
    out.returns[w] = ep_ret;
    out.lengths[w] = ep_len;
    Task::picture(s, rule, pic, mask);
    out.masks[w] = (long long)mask;
  }
  __syncthreads();
  int p[Task::PIC];
  for (int k = 0; k < Task::PIC; ++k) p[k] = pic[k];
  const int P = rule.P, side = G * P, row_words = side >> 2, plane_words = side * row_words;
  unsigned *dst = reinterpret_cast<unsigned *>(out.frames + (long long)w * out.pitch);
  for (int i = threadIdx.x; i < 3 * plane_words; i += ENV_THREADS) {
    const int ch = i / plane_words, rem = i - ch * plane_words;
    const int y = rem / row_words, xw = rem - y * row_words;
    dst[i] = Task::colour(y / P, (xw << 2) / P, p, G, ch);
  }
}

__global__ void env_publish_kernel(long long *word, long long value) {
  __threadfence_system();
  __hip_atomic_store(word, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

inline bool env_al(const void *p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

// What every task's entries validate alike, before anything is launched: pointers and their alignment, W, the geometry's frame
// size against the pitch.  -> 0 or ETM_EINVAL.
int env_check(bool reset, const void *state, const int64_t *actions, int64_t act_stride, const EnvOut &out, const int64_t *done_word,
              int W, int G, int P) {
  if (!state || !out.frames || !out.rewards || !out.flags || !out.returns || !out.lengths || !out.masks || W < 1) return ETM_EINVAL;
  if (!reset && (!actions || act_stride < 1 || !env_al(actions, 8))) return ETM_EINVAL;
  if (!env_grid_ok(G, P)) return ETM_EINVAL;
  if (!env_al(state, 8) || !env_al(out.frames, 4) || !env_al(out.rewards, 4) || !env_al(out.returns, 4) || !env_al(out.lengths, 4) ||
      !env_al(out.masks, 8) || !env_al(done_word, 8))
    return ETM_EINVAL;
  const int64_t frame_bytes = 3ll * G * P * G * P;
  if (out.pitch < frame_bytes || (out.pitch & 3) != 0) return ETM_EINVAL;
  return 0;
}

// Behind a step's launch: its status, then (optionally) the completion word by a one-thread launch on the same stream.
int env_publish(int64_t *done_word, int64_t done_value, hipStream_t st) {
  int rc = etm_launch_status();
  if (rc || !done_word) return rc;
  hipLaunchKernelGGL(env_publish_kernel, dim3(1), dim3(1), 0, st, (long long *)done_word, (long long)done_value);
  return etm_launch_status();
}

// A reset or a step of W environments of one task: the shared checks, the task's own, the launch, the completion word.
template <class Task>
int env_launch(bool reset, void *state, const int64_t *actions, int64_t act_stride, const EnvOut &out, int64_t *done_word,
               int64_t done_value, int W, const typename Task::Rule &rule, void *stream) {
  (void)hipGetLastError();
  if (env_check(reset, state, actions, act_stride, out, done_word, W, rule.G, rule.P) || !Task::rule_ok(rule)) return ETM_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  typename Task::State *s = (typename Task::State *)state;
  if (reset)
    hipLaunchKernelGGL((env_kernel<Task, true>), dim3((unsigned)W), dim3(ENV_THREADS), 0, st, s, (const long long *)nullptr, 0ll, rule, out);
  else
    hipLaunchKernelGGL((env_kernel<Task, false>), dim3((unsigned)W), dim3(ENV_THREADS), 0, st, s, (const long long *)actions,
                       (long long)act_stride, rule, out);
  return env_publish(done_word, done_value, st);
}
}  // namespace

extern "C" int etm_cue_room_supported(int G, int P) { return env_grid_ok(G, P) ? 1 : 0; }

extern "C" int etm_command_room_supported(int G, int P, int K) { return env_grid_ok(G, P) && K >= 1 && K <= CMD_MAX_COMMANDS ? 1 : 0; }

extern "C" int etm_path_room_supported(int G, int P, int M) { return env_grid_ok(G, P) && M >= 1 && M <= PATH_MAX_MOVES ? 1 : 0; }

extern "C" int etm_spot_room_supported(int G, int P, int N, int H) {
  return env_grid_ok(G, P) && N >= 0 && N <= SPOT_MAX_LIGHTS && H >= 1 && H <= SPOT_MAX_HEALTH ? 1 : 0;
}

extern "C" int64_t etm_cue_room_state_bytes(int W) { return W < 1 ? 0 : (int64_t)W * (int64_t)sizeof(CueRoom::State); }

extern "C" int64_t etm_command_room_state_bytes(int W) { return W < 1 ? 0 : (int64_t)W * (int64_t)sizeof(CommandRoom::State); }

extern "C" int64_t etm_path_room_state_bytes(int W) { return W < 1 ? 0 : (int64_t)W * (int64_t)sizeof(PathRoom::State); }

extern "C" int64_t etm_spot_room_state_bytes(int W) { return W < 1 ? 0 : (int64_t)W * (int64_t)sizeof(SpotRoom::State); }

extern "C" int etm_cue_room_reset(void *state, uint8_t *frames, int64_t frame_pitch, float *rewards, uint8_t *flags, float *returns,
                                  int32_t *lengths, int64_t *masks, int64_t *done_word, int64_t done_value, int W, int G, int P,
                                  int cue_steps, int max_steps, int64_t stream0, void *stream) {
  const EnvOut out{frames, (long long)frame_pitch, rewards, flags, returns, lengths, (long long *)masks};
  return env_launch<CueRoom>(true, state, nullptr, 0, out, done_word, done_value, W,
                             CueRoom::Rule{G, P, cue_steps, max_steps, (unsigned long long)stream0}, stream);
}

extern "C" int etm_cue_room_step(void *state, const int64_t *actions, int64_t act_stride, uint8_t *frames, int64_t frame_pitch,
                                 float *rewards, uint8_t *flags, float *returns, int32_t *lengths, int64_t *masks, int64_t *done_word,
                                 int64_t done_value, int W, int G, int P, int cue_steps, int max_steps, int64_t stream0, void *stream) {
  const EnvOut out{frames, (long long)frame_pitch, rewards, flags, returns, lengths, (long long *)masks};
  return env_launch<CueRoom>(false, state, actions, act_stride, out, done_word, done_value, W,
                             CueRoom::Rule{G, P, cue_steps, max_steps, (unsigned long long)stream0}, stream);
}

extern "C" int etm_command_room_reset(void *state, uint8_t *frames, int64_t frame_pitch, float *rewards, uint8_t *flags, float *returns,
                                      int32_t *lengths, int64_t *masks, int64_t *done_word, int64_t done_value, int W, int G, int P,
                                      int K, int show_steps, int gap_steps, int64_t stream0, void *stream) {
  const EnvOut out{frames, (long long)frame_pitch, rewards, flags, returns, lengths, (long long *)masks};
  return env_launch<CommandRoom>(true, state, nullptr, 0, out, done_word, done_value, W,
                                 CommandRoom::Rule{G, P, K, show_steps, gap_steps, (unsigned long long)stream0}, stream);
}

extern "C" int etm_command_room_step(void *state, const int64_t *actions, int64_t act_stride, uint8_t *frames, int64_t frame_pitch,
                                     float *rewards, uint8_t *flags, float *returns, int32_t *lengths, int64_t *masks,
                                     int64_t *done_word, int64_t done_value, int W, int G, int P, int K, int show_steps, int gap_steps,
                                     int64_t stream0, void *stream) {
  const EnvOut out{frames, (long long)frame_pitch, rewards, flags, returns, lengths, (long long *)masks};
  return env_launch<CommandRoom>(false, state, actions, act_stride, out, done_word, done_value, W,
                                 CommandRoom::Rule{G, P, K, show_steps, gap_steps, (unsigned long long)stream0}, stream);
}

extern "C" int etm_path_room_reset(void *state, uint8_t *frames, int64_t frame_pitch, float *rewards, uint8_t *flags, float *returns,
                                   int32_t *lengths, int64_t *masks, int64_t *done_word, int64_t done_value, int W, int G, int P, int M,
                                   int max_steps, int64_t stream0, void *stream) {
  const EnvOut out{frames, (long long)frame_pitch, rewards, flags, returns, lengths, (long long *)masks};
  return env_launch<PathRoom>(true, state, nullptr, 0, out, done_word, done_value, W,
                              PathRoom::Rule{G, P, M, max_steps, (unsigned long long)stream0}, stream);
}

extern "C" int etm_path_room_step(void *state, const int64_t *actions, int64_t act_stride, uint8_t *frames, int64_t frame_pitch,
                                  float *rewards, uint8_t *flags, float *returns, int32_t *lengths, int64_t *masks, int64_t *done_word,
                                  int64_t done_value, int W, int G, int P, int M, int max_steps, int64_t stream0, void *stream) {
  const EnvOut out{frames, (long long)frame_pitch, rewards, flags, returns, lengths, (long long *)masks};
  return env_launch<PathRoom>(false, state, actions, act_stride, out, done_word, done_value, W,
                              PathRoom::Rule{G, P, M, max_steps, (unsigned long long)stream0}, stream);
}

extern "C" int etm_spot_room_reset(void *state, uint8_t *frames, int64_t frame_pitch, float *rewards, uint8_t *flags, float *returns,
                                   int32_t *lengths, int64_t *masks, int64_t *done_word, int64_t done_value, int W, int G, int P, int N,
                                   int light_steps, int spot_period, int health, int max_steps, int64_t stream0, void *stream) {
  const EnvOut out{frames, (long long)frame_pitch, rewards, flags, returns, lengths, (long long *)masks};
  return env_launch<SpotRoom>(true, state, nullptr, 0, out, done_word, done_value, W,
                              SpotRoom::Rule{G, P, N, light_steps, spot_period, health, max_steps, (unsigned long long)stream0}, stream);
}

extern "C" int etm_spot_room_step(void *state, const int64_t *actions, int64_t act_stride, uint8_t *frames, int64_t frame_pitch,
                                  float *rewards, uint8_t *flags, float *returns, int32_t *lengths, int64_t *masks, int64_t *done_word,
                                  int64_t done_value, int W, int G, int P, int N, int light_steps, int spot_period, int health,
                                  int max_steps, int64_t stream0, void *stream) {
  const EnvOut out{frames, (long long)frame_pitch, rewards, flags, returns, lengths, (long long *)masks};
  return env_launch<SpotRoom>(false, state, actions, act_stride, out, done_word, done_value, W,
                              SpotRoom::Rule{G, P, N, light_steps, spot_period, health, max_steps, (unsigned long long)stream0}, stream);
}
