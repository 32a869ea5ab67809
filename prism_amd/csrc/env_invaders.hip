// MinAtar Space Invaders (10 x 10 x 6 observations, 6 or 4 actions) on the games' shared frame (env_frame.h).  The rules are the
// table of DESIGN.md 7.6 -- a restatement of MinAtar v1, NOT checked against the `minatar` package.  A translation unit of its
// own: learner.hip's code object stays what it was.
//
// The 32-byte state record comes in through one broadcast load, lane 0 writes the new one.  MinAtar's three 10 x 10 maps are
// kept as what play can make of them: the aliens are a rigid 4 x 6 block (24 occupancy bits, an origin, a direction), a bullet
// map has at most one bullet per row (ten 4-bit fields x + 1, 0 = none).  Block and bullet rows stay PACKED in their words;
// every access is a shift of a scalar word, by a constant in the unrolled loops and by a wave-uniform count where the origin
// decides the bit -- never an indexed array, which would go to the private segment.  A board cell is six channels, which is no
// store unit: the image is 150 chunks, lane l owns chunks l, l + 64 and l + 128 (< 150) and looks the at most two cells of a
// chunk up in the packed state from its side; a step whose episode goes on builds one image and stores it twice.  No LDS, no
// private segment.
#include "env_frame.h"

namespace prism {

// stream key, apart from "TAU0" + sid, "PERM", "UNIF", "IDSA", "EGRD", "ENVB", Freeway's five and Asterix's two
constexpr uint64_t SI_KEY_COIN = 0x53504943ull;           // "SPIC": the sticky coin (the game draws nothing else)
constexpr int SI_CHANNELS = 6, SI_CELLS = 100;
constexpr int SI_CHUNKS = SI_CELLS * SI_CHANNELS / 4;     // 150 chunks of four elements
// the block: 4 rows x 6 columns, first placed at rows 0..3, columns 2..7
constexpr int SI_ROWS = 4, SI_COLS = 6, SI_FIRST_X = 2, SI_FIRST_Y = 0;
constexpr uint32_t SI_FULL_BLOCK = (1u << (SI_ROWS * SI_COLS)) - 1u;
// the three intervals: the cannon's cool-down, the aliens' shot, and the aliens' move at its slowest and fastest
constexpr int SI_SHOT_COOL_DOWN = 5, SI_ENEMY_SHOT_INTERVAL = 10, SI_ENEMY_MOVE_INTERVAL = 12, SI_MOVE_INTERVAL_MIN = 6;
constexpr uint64_t SI_BULLET_ROWS = (1ull << 40) - 1ull;  // ten 4-bit fields
static_assert(SI_CHUNKS <= 3 * WAVE && SI_CELLS * SI_CHANNELS % 4 == 0, "lane l takes chunks l, l + 64 and l + 128");
static_assert(SI_ROWS * SI_COLS == 24, "the block is bits 0..23 of word 0");

// The state record: PRISM_ENV_STATE_WORDS uint32 (include/prism_hip.h has the field map)
//   [0] block bit 6 r + c | (alien_x + 5) << 24 | alien_y << 28
//   [1] friendly bullet fields (x + 1, 0 = none) of rows 0..7   [2] ep_steps   [3] enemy bullet fields of rows 0..7
//   [4] t low   [5] t high   [6] bullet fields of rows 8, 9 and the cannon's small fields   [7] the aliens' small fields
struct SiState {
    uint32_t block;
    uint64_t fb, eb;          // bullet fields of row y in bits 4y..4y+3
    int alien_x, alien_y, dir_plus, pos, shot_timer, last_action;
    int move_timer, alien_shot_timer, move_interval, ramp_index;
    uint32_t ep_steps;
    uint64_t t;
};
// "Reset": last_action and t carry over; no draw
__host__ __device__ inline void si_reset(SiState &s) {
    s.block = SI_FULL_BLOCK, s.alien_x = SI_FIRST_X, s.alien_y = SI_FIRST_Y, s.dir_plus = 0;
    s.fb = s.eb = 0ull;
    s.pos = 5, s.shot_timer = 0;
    s.move_interval = s.move_timer = SI_ENEMY_MOVE_INTERVAL;
    s.alien_shot_timer = SI_ENEMY_SHOT_INTERVAL;
    s.ramp_index = 0;
    s.ep_steps = 0;
}
// an alien on board cell (y, x): block cell (r, c) stands on ((alien_y + r) mod 10, alien_x + c)
__host__ __device__ inline bool si_alien_at(uint32_t block, int alien_x, int alien_y, int y, int x) {
    int r = y - alien_y;
    r += r < 0 ? 10 : 0;
    const int c = x - alien_x;
    return r < SI_ROWS && c >= 0 && c < SI_COLS && ((block >> ((SI_COLS * r + c) & 31)) & 1u);
}
// bit c: block column c holds an alien
__host__ __device__ inline uint32_t si_columns(uint32_t block) {
    return (block | (block >> SI_COLS) | (block >> (2 * SI_COLS)) | (block >> (3 * SI_COLS))) & ((1u << SI_COLS) - 1u);
}
__host__ __device__ inline bool si_column_has(uint32_t cols, int alien_x, int x) {
    const int c = x - alien_x;
    return c >= 0 && c < SI_COLS && ((cols >> (c & 7)) & 1u);
}

// Rules (2) - (9) of the table for the game's action a (0..5, after the sticky coin): the new state, the reward added to
// `reward`, and whether the step is terminal.  Plain integer work on the packed words, host and device as si_reset is: a
// stand-alone host program can run the rules, the codec and the image under a sanitizer against recorded steps.
__host__ __device__ inline bool si_step(SiState &s, int a, float &reward) {
    // (2) the cannon: a bullet enters on row 9 (the row's field is the bullet: play never has one there before the shot)
    if (a == 5) {
        if (s.shot_timer == 0) {
            s.fb = (s.fb & ~(15ull << 36)) | ((uint64_t)(s.pos + 1) << 36);
            s.shot_timer = SI_SHOT_COOL_DOWN;
        }
    } else if (a == 1) {
        s.pos = s.pos > 0 ? s.pos - 1 : 0;
    } else if (a == 3) {
        s.pos = s.pos < 9 ? s.pos + 1 : 9;
    }
    // (3) friendly bullets one row up, (4) enemy bullets one row down: one shift of all ten fields each
    s.fb >>= 4;
    s.eb = (s.eb << 4) & SI_BULLET_ROWS;
    bool terminal = (int)((s.eb >> 36) & 15ull) == s.pos + 1;
    // (5) the aliens
    terminal = terminal || si_alien_at(s.block, s.alien_x, s.alien_y, 9, s.pos);
    const uint32_t cols = si_columns(s.block);          // (a move changes no block bit)
    if (s.move_timer == 0) {
        const int count = __builtin_popcount(s.block);
        s.move_timer = count < s.move_interval ? count : s.move_interval;
        if (s.dir_plus ? si_column_has(cols, s.alien_x, 9) : si_column_has(cols, s.alien_x, 0)) {
            s.dir_plus ^= 1;
            int r9 = 9 - s.alien_y;                       // the block row that stands on board row 9
            r9 += r9 < 0 ? 10 : 0;
            terminal = terminal || (r9 < SI_ROWS && ((s.block >> ((SI_COLS * r9) & 31)) & ((1u << SI_COLS) - 1u)));
            s.alien_y = s.alien_y == 9 ? 0 : s.alien_y + 1;
        } else {
            s.alien_x += s.dir_plus ? 1 : -1;
        }
        terminal = terminal || si_alien_at(s.block, s.alien_x, s.alien_y, 9, s.pos);
    }
    // (6) the aliens' shot: the nearest column that holds an alien, the lower column first on a tie; its alien of the
    // largest board row
    if (s.alien_shot_timer == 0) {
        s.alien_shot_timer = SI_ENEMY_SHOT_INTERVAL;
        int sx = -1;
#pragma unroll
        for (int d = 0; d < 10; ++d) {
            if (sx < 0 && s.pos - d >= 0 && si_column_has(cols, s.alien_x, s.pos - d)) sx = s.pos - d;
            if (d > 0 && sx < 0 && s.pos + d <= 9 && si_column_has(cols, s.alien_x, s.pos + d)) sx = s.pos + d;
        }
        if (sx >= 0) {                                    // (a block is never empty here)
            const uint32_t column = s.block >> ((sx - s.alien_x) & 7);
            int sy = -1;
#pragma unroll
            for (int r = 0; r < SI_ROWS; ++r) {
                int y = s.alien_y + r;
                y -= y > 9 ? 10 : 0;
                if ((column >> (SI_COLS * r)) & 1u) sy = y > sy ? y : sy;
            }
            s.eb = (s.eb & ~(15ull << (4 * sy))) | ((uint64_t)(sx + 1) << (4 * sy));
        }
    }
    // (7) kills: a cell that holds an alien and a friendly bullet loses both
#pragma unroll
    for (int y = 0; y < 10; ++y) {
        const int x = (int)((s.fb >> (4 * y)) & 15ull) - 1;
        if (x >= 0 && si_alien_at(s.block, s.alien_x, s.alien_y, y, x)) {
            int r = y - s.alien_y;
            r += r < 0 ? 10 : 0;
            s.block &= ~(1u << ((SI_COLS * r + x - s.alien_x) & 31));
            s.fb &= ~(15ull << (4 * y));
            reward += 1.f;
        }
    }
    // (8) timers
    s.shot_timer -= s.shot_timer > 0 ? 1 : 0;
    s.move_timer -= 1;
    s.alien_shot_timer -= 1;
    // (9) a cleared board: the next wave, faster while the interval allows
    if (s.block == 0u) {
        if (s.move_interval > SI_MOVE_INTERVAL_MIN) {
            s.move_interval -= 1;
            s.ramp_index += 1;
        }
        s.block = SI_FULL_BLOCK, s.alien_x = SI_FIRST_X, s.alien_y = SI_FIRST_Y;
    }
    return terminal;
}

// The six channels of board cell `cell` = 10 y + x in bits 0..5, looked up from the lane's side; 0 for a cell off the board.
__host__ __device__ inline uint32_t si_cell(const SiState &s, int cell) {
    const int y = (cell * 205) >> 11, x = cell - 10 * y;          // cell / 10 for cell < 1024
    const uint32_t alien = si_alien_at(s.block, s.alien_x, s.alien_y, y, x) ? 1u : 0u;
    const uint32_t want = (uint32_t)(x + 1);
    const uint32_t f = (uint32_t)(s.fb >> (4 * y)) & 15u, e = (uint32_t)(s.eb >> (4 * y)) & 15u;
    const uint32_t v = (y == 9 && x == s.pos ? 1u : 0u) | (alien << 1) | (alien << (s.dir_plus ? 3 : 2)) | (f == want ? 16u : 0u) |
                       (e == want ? 32u : 0u);
    return cell < SI_CELLS ? v : 0u;
}
// An image as a lane holds it: the four elements of chunk lane + 64 j in bits 4j..4j+3.
__host__ __device__ inline uint32_t si_image(const SiState &s, int lane) {
    uint32_t img = 0u;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int first = 4 * (lane + 64 * j);                    // the chunk's first element, 6 cell + channel
        const int cell = (first * 683) >> 12, ch = first - SI_CHANNELS * cell;          // first / 6 for first < 2048
        const uint32_t two = si_cell(s, cell) | (si_cell(s, cell + 1) << SI_CHANNELS);
        img |= ((two >> ch) & 15u) << (4 * j);
    }
    return img;
}
__host__ __device__ inline void si_pack(const SiState &s, uint32_t (&w)[PRISM_ENV_STATE_WORDS]) {
    w[0] = s.block | ((uint32_t)(s.alien_x + 5) << 24) | ((uint32_t)s.alien_y << 28);
    w[1] = (uint32_t)s.fb, w[2] = s.ep_steps, w[3] = (uint32_t)s.eb, w[4] = (uint32_t)s.t, w[5] = (uint32_t)(s.t >> 32);
    w[6] = (uint32_t)(s.fb >> 32) | ((uint32_t)(s.eb >> 32) << 8) | ((uint32_t)s.pos << 16) | ((uint32_t)s.shot_timer << 20) |
           ((uint32_t)s.dir_plus << 23) | ((uint32_t)s.last_action << 24);
    w[7] = (uint32_t)s.move_timer | ((uint32_t)s.alien_shot_timer << 4) | ((uint32_t)s.move_interval << 8) | ((uint32_t)s.ramp_index << 12);
}
__host__ __device__ inline void si_unpack(const uint32_t (&w)[PRISM_ENV_STATE_WORDS], SiState &s) {
    s.block = w[0] & SI_FULL_BLOCK, s.alien_x = (int)((w[0] >> 24) & 15u) - 5, s.alien_y = (int)(w[0] >> 28);
    s.fb = (uint64_t)w[1] | ((uint64_t)(w[6] & 255u) << 32);
    s.eb = (uint64_t)w[3] | ((uint64_t)((w[6] >> 8) & 255u) << 32);
    s.ep_steps = w[2];
    s.t = (uint64_t)w[4] | ((uint64_t)w[5] << 32);
    s.pos = (w[6] >> 16) & 15, s.shot_timer = (w[6] >> 20) & 7, s.dir_plus = (w[6] >> 23) & 1, s.last_action = (w[6] >> 24) & 7;
    s.move_timer = w[7] & 15, s.alien_shot_timer = (w[7] >> 4) & 15, s.move_interval = (w[7] >> 8) & 15, s.ramp_index = (w[7] >> 12) & 7;
}
// lane 0 writes the record: two ordinary 16-byte vector stores
__device__ __forceinline__ void si_store_state(uint32_t *rec, const SiState &s) {
    uint32_t w[PRISM_ENV_STATE_WORDS];
    si_pack(s, w);
    uint4 *p = reinterpret_cast<uint4 *>(rec);
    p[0] = make_uint4(w[0], w[1], w[2], w[3]);
    p[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

__global__ __launch_bounds__(ENV_THREADS) void env_invaders_reset_kernel(EnvArgs k) {
    int env, lane;
    if (!env_of_wave(k, env, lane)) return;
    SiState s;
    s.last_action = 0;
    s.t = 0;
    si_reset(s);
    env_store_image<SI_CHUNKS>(k.obs_next, k.obs_kind, env, lane, si_image(s, lane));
    if (lane == 0) si_store_state(k.state + (size_t)env * PRISM_ENV_STATE_WORDS, s);
}

__global__ __launch_bounds__(ENV_THREADS) void env_invaders_step_kernel(EnvArgs k) {
    int env, lane;
    if (!env_of_wave(k, env, lane)) return;
    uint32_t *rec = k.state + (size_t)env * PRISM_ENV_STATE_WORDS;
    const uint4 q0 = reinterpret_cast<const uint4 *>(rec)[0];
    const uint4 q1 = reinterpret_cast<const uint4 *>(rec)[1];
    const uint32_t w[PRISM_ENV_STATE_WORDS] = {uni(q0.x), uni(q0.y), uni(q0.z), uni(q0.w), uni(q1.x), uni(q1.y), uni(q1.z), uni(q1.w)};
    SiState s;
    si_unpack(w, s);

    // (the action's load is in flight while the coin is drawn)
    int a = env_action(k.actions, env, k.n_actions, k.status, lane);
    const double u = env_coin(k.u_in, k.seed, s.t, env, SI_KEY_COIN);
    // the 4-action set is n, l, r, f
    if (k.n_actions == 4) a = a == 2 ? 3 : (a == 3 ? 5 : a);
    a = env_sticky(a, u, k.sticky_p, s.last_action);

    float reward = 0.f;
    const bool terminal = si_step(s, a, reward);
    const bool truncated = env_count_step(s.ep_steps, s.t, k.step_limit, terminal);          // (10) counters and flags

    uint32_t img = si_image(s, lane);
    env_store_image<SI_CHUNKS>(k.next_obs, k.obs_kind, env, lane, img);          // what the step returned, before any reset
    if (terminal || truncated) {                                                 // (wave-uniform) only then is the acting image another one
        si_reset(s);
        img = si_image(s, lane);
    }
    env_store_image<SI_CHUNKS>(k.obs_next, k.obs_kind, env, lane, img);          // what to act on next
    if (lane == 0) si_store_state(rec, s);
    env_store_outcome(k, env, lane, reward, terminal, truncated);
}

}  // namespace prism

using namespace prism;

extern "C" int prism_env_invaders_reset(const prism_env_desc *d, prism_stream_t stream_) {
    const int rc = check_env(d, 4, "n_actions must be 4 or 6");
    if (rc != PRISM_OK) return rc;
    return env_launch(env_invaders_reset_kernel, env_args(d, 0), stream_);
}

extern "C" int prism_env_invaders_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, int32_t parity,
                                       prism_stream_t stream_) {
    const int rc = check_env(d, 4, "n_actions must be 4 or 6");
    if (rc != PRISM_OK) return rc;
    PRISM_CHECK_ARG(actions, "actions is null");
    PRISM_CHECK_ARG(parity == 0 || parity == 1, "parity must be 0 or 1");
    return env_launch(env_invaders_step_kernel, env_args(d, parity ^ 1, actions, u_in), stream_);
}
