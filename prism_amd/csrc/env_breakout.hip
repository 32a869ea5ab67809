// MinAtar Breakout (10 x 10 x 4 observations, 6 or 3 actions) on the games' shared frame (env_frame.h).  The rules are the table
// of DESIGN.md 7.3 -- a restatement of MinAtar v1, NOT checked against the `minatar` package.  A translation unit of its own:
// learner.hip's code object stays what it was.
//
// The 32-byte state record comes in through one broadcast load, lane 0 writes the new one.  Board cell (y, x) is four channels
// = one chunk: lane l looks cells l and l + 64 (< 100) up from its side.  No LDS, no private segment.
#include "env_frame.h"

namespace prism {

constexpr uint64_t ENV_KEY = 0x454E5642ull;          // "ENVB": apart from "TAU0" + sid, "PERM", "UNIF", "IDSA", "EGRD"
constexpr int ENV_CELLS = 100;
constexpr uint32_t ENV_FULL_BRICKS = (1u << 30) - 1;          // rows 1..3: bit 10 (y - 1) + x

// The state record: PRISM_ENV_STATE_WORDS uint32 (include/prism_hip.h has the field map of word 1)
//   [0] bricks   [1] packed small fields   [2] ep_steps   [3] 0   [4] t low   [5] t high   [6] 0   [7] 0
struct EnvState {
    uint32_t bricks;
    int pos, ball_x, ball_y, dir, last_x, last_y, strike, last_action;
    uint32_t ep_steps;
    uint64_t t;
};
__host__ __device__ inline uint32_t env_pack(const EnvState &s) {
    return (uint32_t)s.pos | ((uint32_t)s.ball_x << 4) | ((uint32_t)s.ball_y << 8) | ((uint32_t)s.dir << 12) |
           ((uint32_t)s.last_x << 16) | ((uint32_t)s.last_y << 20) | ((uint32_t)s.strike << 24) | ((uint32_t)s.last_action << 25);
}
__host__ __device__ inline void env_unpack(uint32_t w, EnvState &s) {
    s.pos = w & 15, s.ball_x = (w >> 4) & 15, s.ball_y = (w >> 8) & 15, s.dir = (w >> 12) & 3;
    s.last_x = (w >> 16) & 15, s.last_y = (w >> 20) & 15, s.strike = (w >> 24) & 1, s.last_action = (w >> 25) & 7;
}
// "Reset with side s": last_action and t carry over
__host__ __device__ inline void env_reset(EnvState &s, int side) {
    s.ball_y = 3;
    s.ball_x = side ? 9 : 0;
    s.dir = side ? 3 : 2;
    s.pos = 4;
    s.bricks = ENV_FULL_BRICKS;
    s.strike = 0;
    s.last_x = s.ball_x, s.last_y = s.ball_y;
    s.ep_steps = 0;
}
__host__ __device__ inline bool env_brick(uint32_t bricks, int y, int x) {
    return y >= 1 && y <= 3 && ((bricks >> (10 * (y - 1) + x)) & 1u);
}

// the four channels of board cell c = 10 y + x as bits 0..3
__device__ __forceinline__ uint32_t env_cell(const EnvState &s, int c) {
    const int y = c / 10, x = c - 10 * y;
    return (uint32_t)(y == 9 && x == s.pos) | ((uint32_t)(y == s.ball_y && x == s.ball_x) << 1) |
           ((uint32_t)(y == s.last_y && x == s.last_x) << 2) | ((uint32_t)env_brick(s.bricks, y, x) << 3);
}
// An image as a lane holds it: the four channels of cell lane in bits 0..3, of cell lane + 64 in bits 4..7.
__device__ __forceinline__ uint32_t env_image(const EnvState &s, int lane) { return env_cell(s, lane) | (env_cell(s, lane + 64) << 4); }
__device__ __forceinline__ void env_store_state(uint32_t *rec, const EnvState &s) {
    uint4 *p = reinterpret_cast<uint4 *>(rec);
    p[0] = make_uint4(s.bricks, env_pack(s), s.ep_steps, 0u);
    p[1] = make_uint4((uint32_t)s.t, (uint32_t)(s.t >> 32), 0u, 0u);
}

__global__ __launch_bounds__(ENV_THREADS) void env_breakout_reset_kernel(EnvArgs k) {
    int env, lane;
    if (!env_of_wave(k, env, lane)) return;
    const uint8_t *side_in = static_cast<const uint8_t *>(k.draws_in);
    int side;
    if (side_in) {
        side = (int)uni(side_in[env]) & 1;
    } else {
        uint32_t r[4];
        Philox(k.seed)(~0ull, ((uint64_t)env << 32) | ENV_KEY, r);
        side = (int)uni(r[3] & 1u);
    }
    EnvState s;
    s.last_action = 0;
    s.t = 0;
    env_reset(s, side);
    env_store_image<ENV_CELLS>(k.obs_next, k.obs_kind, env, lane, env_image(s, lane));
    if (lane == 0) env_store_state(k.state + (size_t)env * PRISM_ENV_STATE_WORDS, s);
}

__global__ __launch_bounds__(ENV_THREADS) void env_breakout_step_kernel(EnvArgs k) {
    int env, lane;
    if (!env_of_wave(k, env, lane)) return;
    uint32_t *rec = k.state + (size_t)env * PRISM_ENV_STATE_WORDS;
    const uint4 w0 = reinterpret_cast<const uint4 *>(rec)[0];
    const uint2 w1 = reinterpret_cast<const uint2 *>(rec)[2];
    EnvState s;
    s.bricks = uni(w0.x);
    env_unpack(uni(w0.y), s);
    s.ep_steps = uni(w0.z);
    s.t = (uint64_t)uni(w1.x) | ((uint64_t)uni(w1.y) << 32);

    int a = env_action(k.actions, env, k.n_actions, k.status, lane);          // (its load is in flight while the draws are made)

    // The draws of this step, from ONE Philox call: the sticky coin (words 0, 1) and the side (word 2) of the episode that
    // begins if this step ends one.  Not env_coin: that would be a second call.
    const uint8_t *side_in = static_cast<const uint8_t *>(k.draws_in);
    double u = 1.0;
    int side = 0;
    if (!(k.u_in && side_in)) {
        uint32_t r[4];
        Philox(k.seed)(s.t, ((uint64_t)env << 32) | ENV_KEY, r);
        u = u64_to_unit_double(uni(r[0]), uni(r[1]));
        side = (int)uni(r[2] & 1u);
    }
    if (k.u_in) u = env_given_coin(k.u_in, env);
    if (side_in) side = (int)uni(side_in[env]) & 1;

    if (k.n_actions == 3) a = a == 2 ? 3 : a;          // the 3-action set is n, l, r
    a = env_sticky(a, u, k.sticky_p, s.last_action);

    if (a == 1) s.pos = max(0, s.pos - 1);
    else if (a == 3) s.pos = min(9, s.pos + 1);
    const int bx = s.ball_x;
    s.last_x = s.ball_x, s.last_y = s.ball_y;
    int nx = s.ball_x + ((s.dir == 1 || s.dir == 2) ? 1 : -1);
    int ny = s.ball_y + (s.dir >= 2 ? 1 : -1);
    if (nx < 0 || nx > 9) {
        nx = nx < 0 ? 0 : 9;
        s.dir ^= 1;          // [1, 0, 3, 2]
    }
    bool toggle = false, terminal = false;
    float reward = 0.f;
    if (ny < 0) {
        ny = 0;
        s.dir ^= 3;          // [3, 2, 1, 0]
    } else if (env_brick(s.bricks, ny, nx)) {
        toggle = true;
        if (!s.strike) {
            reward = 1.f;
            s.strike = 1;
            s.bricks &= ~(1u << (10 * (ny - 1) + nx));
            ny = s.last_y;
            s.dir ^= 3;
        }
    } else if (ny == 9) {
        if (s.bricks == 0u) s.bricks = ENV_FULL_BRICKS;
        if (bx == s.pos) {
            s.dir ^= 3;
            ny = s.last_y;
        } else if (nx == s.pos) {
            s.dir ^= 2;      // [2, 3, 0, 1]
            ny = s.last_y;
        } else {
            terminal = true;
        }
    }
    if (!toggle) s.strike = 0;
    s.ball_x = nx, s.ball_y = ny;
    const bool truncated = env_count_step(s.ep_steps, s.t, k.step_limit, terminal);

    env_store_image<ENV_CELLS>(k.next_obs, k.obs_kind, env, lane, env_image(s, lane));          // what the step returned, before any reset
    if (terminal || truncated) env_reset(s, side);
    env_store_image<ENV_CELLS>(k.obs_next, k.obs_kind, env, lane, env_image(s, lane));          // what to act on next
    if (lane == 0) env_store_state(rec, s);
    env_store_outcome(k, env, lane, reward, terminal, truncated);
}

}  // namespace prism

using namespace prism;

extern "C" int prism_env_breakout_reset(const prism_env_desc *d, const uint8_t *first_side_in, prism_stream_t stream_) {
    const int rc = check_env(d, 3, "n_actions must be 3 or 6");
    if (rc != PRISM_OK) return rc;
    return env_launch(env_breakout_reset_kernel, env_args(d, 0, nullptr, nullptr, first_side_in), stream_);
}

extern "C" int prism_env_breakout_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, const uint8_t *side_in,
                                       int32_t parity, prism_stream_t stream_) {
    const int rc = check_env(d, 3, "n_actions must be 3 or 6");
    if (rc != PRISM_OK) return rc;
    PRISM_CHECK_ARG(actions, "actions is null");
    PRISM_CHECK_ARG(parity == 0 || parity == 1, "parity must be 0 or 1");
    return env_launch(env_breakout_step_kernel, env_args(d, parity ^ 1, actions, u_in, side_in), stream_);
}
