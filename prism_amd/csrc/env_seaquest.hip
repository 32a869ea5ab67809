// MinAtar Seaquest (10 x 10 x 10 observations, 6 actions) on the games' shared frame (env_frame.h).  The rules are the table of
// DESIGN.md 7.7 -- a restatement of MinAtar v1, NOT checked against the `minatar` package.  A translation unit of its own:
// learner.hip's code object stays what it was.
//
// Unlike the four games of the 8-word record this one keeps five ORDERED LISTS that grow and shrink (fish, enemy subs, enemy
// bullets, friendly bullets, divers); the record (PRISM_ENV_SEAQUEST_STATE_WORDS words) holds them as fixed-capacity arrays in
// list order, one 32-bit word per entry, an empty slot all zeros.  Lane i of the wave holds entry i of every list; the eight
// head words are wave-uniform (one broadcast load, scalar registers after readfirstlane).
//   * a rule that visits a long list (enemy subs, fish, enemy bullets) runs on all of its entries at once; where the list
//     order decides -- which of several enemies on a cell a bullet kills, which of several subs takes a bullet, the order of
//     the bullets the subs fire -- it is a ballot and the lowest / highest set lane of it;
//   * a rule that visits a short list (friendly bullets, divers: at most 4) walks it last to first with a wave-uniform
//     counter, one readlane per entry;
//   * removal zeroes the entry's lane; a stable compaction (ballot, prefix count, one lane permute) closes the holes;
//   * an append beyond a capacity is dropped and raises PRISM_ENV_STATUS_OVERFLOW.
// The image is built in 104 words of LDS per wave (one word per board cell, channel c in bit c: every entry ORs its own and
// its trail cell), then lane l stores the four-element chunks l, l + 64, l + 128 and l + 192 (< 250).  No per-lane array is
// indexed by a run-time value: no private segment.
#include "env_frame.h"

namespace prism {

// stream keys, apart from every other key of csrc/ and from each other
constexpr uint64_t SQ_KEY_COIN = 0x53515843ull;           // "SQXC": the sticky coin
constexpr uint64_t SQ_KEY_ENEMY = 0x53515845ull;          // "SQXE": side, kind and row of an enemy spawn
constexpr uint64_t SQ_KEY_DIVER = 0x53515844ull;          // "SQXD": side and row of a diver spawn
constexpr int SQ_CHANNELS = 10, SQ_CELLS = 100;
constexpr int SQ_CHUNKS = SQ_CELLS * SQ_CHANNELS / 4;     // 250 chunks of four elements
constexpr int SQ_CELL_WORDS = 104;                        // the board and a zero cell behind it (a chunk may end in cell 100)
// capacities (DESIGN.md 7.7 derives them) and where the arrays start in the record
constexpr int SQ_FISH = 32, SQ_SUBS = 32, SQ_EBULLETS = 32, SQ_FBULLETS = 4, SQ_DIVERS = 4;
constexpr int SQ_AT_FISH = 8, SQ_AT_SUBS = SQ_AT_FISH + SQ_FISH, SQ_AT_EBULLETS = SQ_AT_SUBS + SQ_SUBS;
constexpr int SQ_AT_FBULLETS = SQ_AT_EBULLETS + SQ_EBULLETS, SQ_AT_DIVERS = SQ_AT_FBULLETS + SQ_FBULLETS;
static_assert(SQ_AT_DIVERS + SQ_DIVERS == PRISM_ENV_SEAQUEST_STATE_WORDS && PRISM_ENV_SEAQUEST_STATE_WORDS % 4 == 0, "the record");
static_assert(SQ_FISH <= WAVE && SQ_SUBS <= WAVE && SQ_EBULLETS <= WAVE, "one lane per list entry");
static_assert(SQ_CHUNKS <= 4 * WAVE && SQ_CELLS * SQ_CHANNELS % 4 == 0, "lane l takes chunks l, l + 64, l + 128 and l + 192");
// the game's constants
constexpr int SQ_MAX_OXYGEN = 200, SQ_MAX_DIVERS = 6, SQ_SHOT_COOL_DOWN = 5, SQ_ENEMY_SHOT_INTERVAL = 10;
constexpr int SQ_ENEMY_SPAWN_SPEED = 20, SQ_DIVER_SPAWN_SPEED = 30, SQ_ENEMY_MOVE_SPEED = 5, SQ_DIVER_MOVE_INTERVAL = 5;
constexpr int SQ_MOVE_SPEED_MIN = 2;

// A list entry: x (bits 0-3) | y (4-7) | direction (8; 1: moves to +x) | move_timer (9-11) | shot_timer (12-15) | present (16)
constexpr uint32_t SQ_PRESENT = 1u << 16, SQ_X = 15u, SQ_DIR = 1u << 8, SQ_TIMER = 7u << 9, SQ_SHOT = 15u << 12;
constexpr uint32_t SQ_CELL = SQ_PRESENT | 255u;           // present, x and y: what "on the same cell" compares

// The head of the record: PRISM_ENV_SEAQUEST_STATE_WORDS uint32 (include/prism_hip.h has the field map)
//   [0] sub_x | sub_y << 4 | sub_or << 8 | surface << 9 | shot_timer << 10 | diver_count << 13 | last_action << 16 |
//       move_speed << 19 | ramp_index << 22
//   [1] (oxygen + 1) | e_spawn_speed << 8 | e_spawn_timer << 13 | d_spawn_timer << 18
//   [2] ep_steps   [4] t low   [5] t high   [3], [6], [7] zero
struct SqHead {
    int sub_x, sub_y, sub_or, surface, shot_timer, diver_count, last_action, move_speed, ramp_index;
    int oxygen, e_spawn_speed, e_spawn_timer, d_spawn_timer;
    uint32_t ep_steps;
    uint64_t t;
};
// lane i holds entry i of each list (zero beyond the list's end and beyond its capacity)
struct SqLists {
    uint32_t fish, subs, ebullets, fbullets, divers;
};
// "Reset": last_action and t carry over; no draw
__device__ __forceinline__ void sq_reset(SqHead &h, SqLists &l) {
    h.sub_x = 5, h.sub_y = 0, h.sub_or = 0, h.surface = 1, h.shot_timer = 0, h.diver_count = 0;
    h.oxygen = SQ_MAX_OXYGEN;
    h.e_spawn_speed = h.e_spawn_timer = SQ_ENEMY_SPAWN_SPEED;
    h.d_spawn_timer = SQ_DIVER_SPAWN_SPEED;
    h.move_speed = SQ_ENEMY_MOVE_SPEED;
    h.ramp_index = 0;
    h.ep_steps = 0;
    l.fish = l.subs = l.ebullets = l.fbullets = l.divers = 0u;
}

__device__ __forceinline__ uint64_t sq_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// entry i of a list, wave-uniform (i is)
__device__ __forceinline__ uint32_t sq_get(uint32_t v, int i) { return (uint32_t)__builtin_amdgcn_readlane((int)v, i); }
__device__ __forceinline__ int sq_count(uint32_t v) { return __builtin_popcountll(sq_ballot((v & SQ_PRESENT) != 0u)); }
// Stable compaction: the entries that are present move to lanes 0 .. k - 1 in their order, the zeros behind them.  Every lane
// sends its word to another lane (a permutation of all 64: present lanes to their prefix count, the others to k + their
// rank among the others), so every lane receives exactly one.
__device__ __forceinline__ uint32_t sq_compact(uint32_t v, int lane) {
    const bool there = (v & SQ_PRESENT) != 0u;
    const uint64_t m = sq_ballot(there);
    const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const int k = __builtin_popcountll(m);
    const int to = there ? below : k + (lane - below);
    return (uint32_t)__builtin_amdgcn_ds_permute(to << 2, (int)(there ? v : 0u));
}
// Append `word` behind the list's last entry (the list is compact); false where the list is full: the append is dropped.
__device__ __forceinline__ bool sq_append(uint32_t &v, uint32_t word, int capacity, int lane) {
    const int k = sq_count(v);
    if (k >= capacity) return false;
    v = lane == k ? word : v;
    return true;
}
__device__ __forceinline__ int sq_step_x(uint32_t e) { return (int)(e & SQ_X) + ((e & SQ_DIR) ? 1 : -1); }

// Rules 7 and 9 for one list of enemies, every entry at once.  An enemy on the sub's cell before or after its move is
// terminal; one that leaves the board is removed; one that moved onto a friendly bullet dies with the FIRST such bullet in
// list order.  Enemies are visited last to first, so of several that reach one cell the highest lane takes the first
// bullet, the next lane the next bullet: walking the (at most four) bullets in list order and giving each the highest lane
// still looking on its cell is that pairing.  `with_shot`: an enemy sub that is still there then fires or counts down.
__device__ __forceinline__ void sq_enemies(uint32_t &list, SqLists &l, const SqHead &h, bool with_shot, int lane, float &reward,
                                           bool &terminal, bool &overflow) {
    const uint32_t e = list;
    const bool there = (e & SQ_PRESENT) != 0u;
    const uint32_t sub_cell = SQ_PRESENT | (uint32_t)h.sub_x | ((uint32_t)h.sub_y << 4);
    bool hit = (e & SQ_CELL) == sub_cell;
    const bool moves = there && (e & SQ_TIMER) == 0u;
    const int x = moves ? sq_step_x(e) : (int)(e & SQ_X);
    const bool off = moves && (x < 0 || x > 9);
    uint32_t now = (e & ~(SQ_X | SQ_TIMER)) | ((uint32_t)x & SQ_X);
    now |= moves ? (uint32_t)h.move_speed << 9 : (e & SQ_TIMER) - (1u << 9);          // (a timer that is not 0 is >= 1)
    const bool on_sub = moves && !off && (now & SQ_CELL) == sub_cell;
    hit = hit || on_sub;
    terminal = terminal || sq_ballot(hit) != 0ull;
    const bool looks = moves && !off && !on_sub;
    bool dead = off;
#pragma unroll
    for (int k = 0; k < SQ_FBULLETS; ++k) {
        const uint32_t b = sq_get(l.fbullets, k);
        const uint64_t m = sq_ballot(looks && !dead && (b & SQ_PRESENT) != 0u && (now & SQ_CELL) == (b & SQ_CELL));
        if (m != 0ull) {
            const int top = 63 - __builtin_clzll(m);
            dead = dead || lane == top;
            l.fbullets = lane == k ? 0u : l.fbullets;
            reward += 1.f;
        }
    }
    const bool stays = there && !dead;
    if (with_shot) {
        const bool fires = stays && (now & SQ_SHOT) == 0u;
        now = fires ? now | ((uint32_t)SQ_ENEMY_SHOT_INTERVAL << 12) : now - (1u << 12);
        list = stays ? now : 0u;
        uint64_t fm = sq_ballot(fires);
        int ne = sq_count(l.ebullets);
        while (fm != 0ull) {                               // (wave-uniform) the subs that fire, last to first
            const int top = 63 - __builtin_clzll(fm);
            fm &= ~(1ull << top);
            const uint32_t from = sq_get(list, top);
            if (ne < SQ_EBULLETS) {
                l.ebullets = lane == ne ? SQ_PRESENT | (from & (255u | SQ_DIR)) : l.ebullets;
                ne += 1;
            } else {
                overflow = true;
            }
        }
    } else {
        list = stays ? now : 0u;
    }
    list = sq_compact(list, lane);
    l.fbullets = sq_compact(l.fbullets, lane);
}

// Rules 2 - 11 of the table for the game's action a (0..5, after the sticky coin).  side / kind / row of the two spawns come
// from `draw` (called only on a step that spawns).
template <class EnemyDraw, class DiverDraw>
__device__ __forceinline__ bool sq_step(SqHead &h, SqLists &l, int a, int lane, float &reward, bool &overflow, EnemyDraw enemy_draw,
                                        DiverDraw diver_draw) {
    bool terminal = false;
    // (2) an enemy enters unless a fish or a sub of its row moves the other way
    if (h.e_spawn_timer == 0) {
        uint32_t side, is_sub, row;
        enemy_draw(side, is_sub, row);
        const uint32_t want = SQ_PRESENT | (row << 4) | (side ? 0u : SQ_DIR), mask = SQ_PRESENT | (15u << 4) | SQ_DIR;
        const bool blocked = sq_ballot((l.fish & mask) == want || (l.subs & mask) == want) != 0ull;
        if (!blocked) {
            const uint32_t word = SQ_PRESENT | (side ? 0u : 9u) | (row << 4) | (side ? SQ_DIR : 0u) | ((uint32_t)h.move_speed << 9);
            const bool ok = is_sub ? sq_append(l.subs, word | ((uint32_t)SQ_ENEMY_SHOT_INTERVAL << 12), SQ_SUBS, lane)
                                   : sq_append(l.fish, word, SQ_FISH, lane);
            overflow = overflow || !ok;
        }
        h.e_spawn_timer = h.e_spawn_speed;
    }
    // (3) a diver enters
    if (h.d_spawn_timer == 0) {
        uint32_t side, row;
        diver_draw(side, row);
        const uint32_t word = SQ_PRESENT | (side ? 0u : 9u) | (row << 4) | (side ? SQ_DIR : 0u) | ((uint32_t)SQ_DIVER_MOVE_INTERVAL << 9);
        overflow = overflow || !sq_append(l.divers, word, SQ_DIVERS, lane);
        h.d_spawn_timer = SQ_DIVER_SPAWN_SPEED;
    }
    // (4) the player
    if (a == 5) {
        if (h.shot_timer == 0) {
            const uint32_t word = SQ_PRESENT | (uint32_t)h.sub_x | ((uint32_t)h.sub_y << 4) | (h.sub_or ? SQ_DIR : 0u);
            overflow = overflow || !sq_append(l.fbullets, word, SQ_FBULLETS, lane);
            h.shot_timer = SQ_SHOT_COOL_DOWN;
        }
    } else if (a == 1) {
        h.sub_x = h.sub_x > 0 ? h.sub_x - 1 : 0, h.sub_or = 0;
    } else if (a == 3) {
        h.sub_x = h.sub_x < 9 ? h.sub_x + 1 : 9, h.sub_or = 1;
    } else if (a == 2) {
        h.sub_y = h.sub_y > 0 ? h.sub_y - 1 : 0;
    } else if (a == 4) {
        h.sub_y = h.sub_y < 8 ? h.sub_y + 1 : 8;
    }
    // (5) friendly bullets, last to first: the first fish in list order on the bullet's cell dies with it, else the first sub
    {
        const int nb = sq_count(l.fbullets);
#pragma unroll
        for (int j = SQ_FBULLETS - 1; j >= 0; --j) {
            if (j < nb) {
                const uint32_t b = sq_get(l.fbullets, j);
                const int x = sq_step_x(b);
                uint32_t now = 0u;
                if (x >= 0 && x <= 9) {
                    now = (b & ~SQ_X) | (uint32_t)x;
                    const uint64_t mf = sq_ballot((l.fish & SQ_CELL) == (now & SQ_CELL));
                    if (mf != 0ull) {
                        l.fish = lane == __builtin_ctzll(mf) ? 0u : l.fish;
                        now = 0u, reward += 1.f;
                    } else {
                        const uint64_t ms = sq_ballot((l.subs & SQ_CELL) == (now & SQ_CELL));
                        if (ms != 0ull) {
                            l.subs = lane == __builtin_ctzll(ms) ? 0u : l.subs;
                            now = 0u, reward += 1.f;
                        }
                    }
                }
                l.fbullets = lane == j ? now : l.fbullets;
            }
        }
        l.fish = sq_compact(l.fish, lane), l.subs = sq_compact(l.subs, lane), l.fbullets = sq_compact(l.fbullets, lane);
    }
    // (6) divers, last to first: the order decides who is refused once six are aboard
    {
        const int nd = sq_count(l.divers);
#pragma unroll
        for (int j = SQ_DIVERS - 1; j >= 0; --j) {
            if (j < nd) {
                const uint32_t d = sq_get(l.divers, j);
                const uint32_t sub_cell = SQ_PRESENT | (uint32_t)h.sub_x | ((uint32_t)h.sub_y << 4);
                uint32_t now;
                if ((d & SQ_CELL) == sub_cell && h.diver_count < SQ_MAX_DIVERS) {
                    now = 0u, h.diver_count += 1;
                } else if ((d & SQ_TIMER) == 0u) {
                    const int x = sq_step_x(d);
                    now = (d & ~SQ_X) | ((uint32_t)x & SQ_X) | ((uint32_t)SQ_DIVER_MOVE_INTERVAL << 9);
                    if (x < 0 || x > 9) {
                        now = 0u;
                    } else if ((now & SQ_CELL) == sub_cell && h.diver_count < SQ_MAX_DIVERS) {
                        now = 0u, h.diver_count += 1;
                    }
                } else {
                    now = d - (1u << 9);
                }
                l.divers = lane == j ? now : l.divers;
            }
        }
        l.divers = sq_compact(l.divers, lane);
    }
    // (7) enemy subs
    sq_enemies(l.subs, l, h, true, lane, reward, terminal, overflow);
    // (8) enemy bullets, those of this step among them: on the sub's cell before or after the move is terminal
    {
        const uint32_t e = l.ebullets;
        const uint32_t sub_cell = SQ_PRESENT | (uint32_t)h.sub_x | ((uint32_t)h.sub_y << 4);
        const int x = sq_step_x(e);
        const bool stays = (e & SQ_PRESENT) != 0u && x >= 0 && x <= 9;
        const uint32_t now = stays ? (e & ~SQ_X) | (uint32_t)x : 0u;
        terminal = terminal || sq_ballot((e & SQ_CELL) == sub_cell || (now & SQ_CELL) == sub_cell) != 0ull;
        l.ebullets = sq_compact(now, lane);
    }
    // (9) enemy fish
    sq_enemies(l.fish, l, h, false, lane, reward, terminal, overflow);
    // (10) timers
    h.e_spawn_timer -= h.e_spawn_timer > 0 ? 1 : 0;
    h.d_spawn_timer -= h.d_spawn_timer > 0 ? 1 : 0;
    h.shot_timer -= h.shot_timer > 0 ? 1 : 0;
    // (11) oxygen, surfacing and the ramp
    terminal = terminal || h.oxygen < 0;
    if (h.sub_y > 0) {
        h.oxygen -= 1, h.surface = 0;
    } else if (!h.surface) {
        if (h.diver_count == 0) {
            terminal = true;
        } else {
            h.surface = 1;
            if (h.diver_count == SQ_MAX_DIVERS) {
                reward += h.oxygen < 0 ? -1.f : (float)(h.oxygen * 10 / SQ_MAX_OXYGEN);          // the floor of oxygen * 10 / 200
                h.diver_count = 0;
            } else {
                h.diver_count -= 1;
            }
            h.oxygen = SQ_MAX_OXYGEN;
            if (h.e_spawn_speed > 1 || h.move_speed > SQ_MOVE_SPEED_MIN) {
                if (h.move_speed > SQ_MOVE_SPEED_MIN && (h.ramp_index & 1)) h.move_speed -= 1;
                if (h.e_spawn_speed > 1) h.e_spawn_speed -= 1;
                h.ramp_index += 1;
            }
        }
    }
    return terminal;
}

// OR an entry's own cell (channel `ch`) and, where `trail`, the cell behind it (channel 3, only on the board) into the board
__device__ __forceinline__ void sq_draw(uint32_t *cells, uint32_t e, int ch, bool trail) {
    const int x = (int)(e & SQ_X), y = (int)((e >> 4) & 15u), back = (e & SQ_DIR) ? x - 1 : x + 1;
    if ((e & SQ_PRESENT) && x <= 9 && y <= 9) {          // (on the board in every state the codec accepts)
        atomicOr(&cells[10 * y + x], 1u << ch);
        if (trail && back >= 0 && back <= 9) atomicOr(&cells[10 * y + back], 1u << 3);
    }
}
// An image as a lane holds it: the four elements of chunk lane + 64 j in bits 4j .. 4j+3.  `cells` is this wave's LDS board.
// Channel 0 the sub, 1 the cell behind it, 2 friendly bullets, 3 trails, 4 enemy bullets, 5 fish, 6 enemy subs, 7 the oxygen
// gauge, 8 the diver gauge, 9 divers.
__device__ __forceinline__ uint32_t sq_image(uint32_t *cells, const SqHead &h, const SqLists &l, int lane) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");          // (the reads of an earlier image are done)
    __builtin_amdgcn_wave_barrier();
    cells[lane] = 0u;
    if (lane + 64 < SQ_CELL_WORDS) cells[lane + 64] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    sq_draw(cells, l.fish, 5, true);
    sq_draw(cells, l.subs, 6, true);
    sq_draw(cells, l.ebullets, 4, false);
    sq_draw(cells, l.fbullets, 2, false);
    sq_draw(cells, l.divers, 9, true);
    if (lane == 0 && h.sub_x <= 9 && h.sub_y <= 9) {
        const int back = h.sub_or ? h.sub_x - 1 : h.sub_x + 1;          // (on the board in every state the codec accepts)
        atomicOr(&cells[10 * h.sub_y + h.sub_x], 1u);
        if (back >= 0 && back <= 9) atomicOr(&cells[10 * h.sub_y + back], 2u);
    }
    if (lane < 10) {
        const int bar = h.oxygen < 0 ? 0 : h.oxygen * 10 / SQ_MAX_OXYGEN;
        const uint32_t bits = (lane < bar ? 1u << 7 : 0u) | (lane >= 9 - h.diver_count && lane <= 8 ? 1u << 8 : 0u);
        if (bits) atomicOr(&cells[90 + lane], bits);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    uint32_t img = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int chunk = lane + 64 * j;
        if (chunk < SQ_CHUNKS) {
            const int first = 4 * chunk;                              // the chunk's first element, 10 cell + channel
            const int cell = (first * 205) >> 11, ch = first - SQ_CHANNELS * cell;          // first / 10 for first < 1024
            const uint32_t two = cells[cell] | (cells[cell + 1] << SQ_CHANNELS);
            img |= ((two >> ch) & 15u) << (4 * j);
        }
    }
    return img;
}
// The record: lane 0 writes the head (two 16-byte stores), lane i entry i of every list: ordinary vector stores
__device__ __forceinline__ void sq_store_state(uint32_t *rec, const SqHead &h, const SqLists &l, int lane) {
    if (lane == 0) {
        const uint32_t w0 = (uint32_t)h.sub_x | ((uint32_t)h.sub_y << 4) | ((uint32_t)h.sub_or << 8) | ((uint32_t)h.surface << 9) |
                            ((uint32_t)h.shot_timer << 10) | ((uint32_t)h.diver_count << 13) | ((uint32_t)h.last_action << 16) |
                            ((uint32_t)h.move_speed << 19) | ((uint32_t)h.ramp_index << 22);
        const uint32_t w1 = (uint32_t)(h.oxygen + 1) | ((uint32_t)h.e_spawn_speed << 8) | ((uint32_t)h.e_spawn_timer << 13) |
                            ((uint32_t)h.d_spawn_timer << 18);
        uint4 *p = reinterpret_cast<uint4 *>(rec);
        p[0] = make_uint4(w0, w1, h.ep_steps, 0u);
        p[1] = make_uint4((uint32_t)h.t, (uint32_t)(h.t >> 32), 0u, 0u);
    }
    if (lane < SQ_FISH) rec[SQ_AT_FISH + lane] = l.fish;
    if (lane < SQ_SUBS) rec[SQ_AT_SUBS + lane] = l.subs;
    if (lane < SQ_EBULLETS) rec[SQ_AT_EBULLETS + lane] = l.ebullets;
    if (lane < SQ_FBULLETS) rec[SQ_AT_FBULLETS + lane] = l.fbullets;
    if (lane < SQ_DIVERS) rec[SQ_AT_DIVERS + lane] = l.divers;
}
__device__ __forceinline__ void sq_load_state(const uint32_t *rec, SqHead &h, SqLists &l, int lane) {
    const uint4 q0 = reinterpret_cast<const uint4 *>(rec)[0];
    const uint4 q1 = reinterpret_cast<const uint4 *>(rec)[1];
    const uint32_t w0 = uni(q0.x), w1 = uni(q0.y);
    h.sub_x = w0 & 15, h.sub_y = (w0 >> 4) & 15, h.sub_or = (w0 >> 8) & 1, h.surface = (w0 >> 9) & 1, h.shot_timer = (w0 >> 10) & 7;
    h.diver_count = (w0 >> 13) & 7, h.last_action = (w0 >> 16) & 7, h.move_speed = (w0 >> 19) & 7, h.ramp_index = (w0 >> 22) & 31;
    h.oxygen = (int)(w1 & 255u) - 1, h.e_spawn_speed = (w1 >> 8) & 31, h.e_spawn_timer = (w1 >> 13) & 31, h.d_spawn_timer = (w1 >> 18) & 31;
    h.ep_steps = uni(q0.z);
    h.t = (uint64_t)uni(q1.x) | ((uint64_t)uni(q1.y) << 32);
    l.fish = lane < SQ_FISH ? rec[SQ_AT_FISH + lane] : 0u;
    l.subs = lane < SQ_SUBS ? rec[SQ_AT_SUBS + lane] : 0u;
    l.ebullets = lane < SQ_EBULLETS ? rec[SQ_AT_EBULLETS + lane] : 0u;
    l.fbullets = lane < SQ_FBULLETS ? rec[SQ_AT_FBULLETS + lane] : 0u;
    l.divers = lane < SQ_DIVERS ? rec[SQ_AT_DIVERS + lane] : 0u;
}

__global__ __launch_bounds__(ENV_THREADS) void env_seaquest_reset_kernel(EnvArgs k) {
    __shared__ uint32_t board[ENV_PER_WG][SQ_CELL_WORDS];
    int env, lane;
    if (!env_of_wave(k, env, lane)) return;
    uint32_t *cells = board[uni(threadIdx.x >> 6)];
    SqHead h;
    SqLists l;
    h.last_action = 0;
    h.t = 0;
    sq_reset(h, l);
    env_store_image<SQ_CHUNKS>(k.obs_next, k.obs_kind, env, lane, sq_image(cells, h, l, lane));
    sq_store_state(k.state + (size_t)env * PRISM_ENV_SEAQUEST_STATE_WORDS, h, l, lane);
}

__global__ __launch_bounds__(ENV_THREADS) void env_seaquest_step_kernel(EnvArgs k) {
    __shared__ uint32_t board[ENV_PER_WG][SQ_CELL_WORDS];
    int env, lane;
    if (!env_of_wave(k, env, lane)) return;
    uint32_t *cells = board[uni(threadIdx.x >> 6)];
    uint32_t *rec = k.state + (size_t)env * PRISM_ENV_SEAQUEST_STATE_WORDS;
    SqHead h;
    SqLists l;
    sq_load_state(rec, h, l, lane);
    const uint64_t t0 = h.t;          // the counter of this step's draws

    // (the action's load is in flight while the coin is drawn)
    int a = env_action(k.actions, env, k.n_actions, k.status, lane);
    const double u = env_coin(k.u_in, k.seed, t0, env, SQ_KEY_COIN);
    // the minimal set is the same six actions
    a = env_sticky(a, u, k.sticky_p, h.last_action);

    float reward = 0.f;
    bool overflow = false;
    const uint8_t *given = k.draws_in ? static_cast<const uint8_t *>(k.draws_in) + (size_t)env * 5 : nullptr;
    // a given row outside 1..8 is taken into it (a guard: the host checks what it stages)
    auto enemy_draw = [&](uint32_t &side, uint32_t &is_sub, uint32_t &row) {
        if (given) {
            side = uni(given[0]) & 1u, is_sub = uni(given[1]) & 1u, row = 1u + ((uni(given[2]) + 7u) & 7u);
        } else {
            uint32_t r[4];
            Philox(k.seed)(t0, ((uint64_t)env << 32) | SQ_KEY_ENEMY, r);
            side = uni(r[0]) & 1u;
            is_sub = (uint32_t)(((uint64_t)uni(r[1]) * 3ull) >> 32) == 0u ? 1u : 0u;
            row = 1u + (uni(r[2]) >> 29);
        }
    };
    auto diver_draw = [&](uint32_t &side, uint32_t &row) {
        if (given) {
            side = uni(given[3]) & 1u, row = 1u + ((uni(given[4]) + 7u) & 7u);
        } else {
            uint32_t r[4];
            Philox(k.seed)(t0, ((uint64_t)env << 32) | SQ_KEY_DIVER, r);
            side = uni(r[0]) & 1u;
            row = 1u + (uni(r[1]) >> 29);
        }
    };
    const bool terminal = sq_step(h, l, a, lane, reward, overflow, enemy_draw, diver_draw);
    if (overflow && lane == 0) atomicOr(k.status, (uint32_t)PRISM_ENV_STATUS_OVERFLOW);
    const bool truncated = env_count_step(h.ep_steps, h.t, k.step_limit, terminal);          // (12) counters and flags

    uint32_t img = sq_image(cells, h, l, lane);
    env_store_image<SQ_CHUNKS>(k.next_obs, k.obs_kind, env, lane, img);          // what the step returned, before any reset
    if (terminal || truncated) {                                                 // (wave-uniform) only then is the acting image another one
        sq_reset(h, l);
        img = sq_image(cells, h, l, lane);
    }
    env_store_image<SQ_CHUNKS>(k.obs_next, k.obs_kind, env, lane, img);          // what to act on next
    sq_store_state(rec, h, l, lane);
    env_store_outcome(k, env, lane, reward, terminal, truncated);
}

}  // namespace prism

using namespace prism;

extern "C" int prism_env_seaquest_reset(const prism_env_desc *d, prism_stream_t stream_) {
    const int rc = check_env(d, 6, "n_actions must be 6");
    if (rc != PRISM_OK) return rc;
    return env_launch(env_seaquest_reset_kernel, env_args(d, 0), stream_);
}

extern "C" int prism_env_seaquest_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, const uint8_t *draws_in,
                                       int32_t parity, prism_stream_t stream_) {
    const int rc = check_env(d, 6, "n_actions must be 6");
    if (rc != PRISM_OK) return rc;
    PRISM_CHECK_ARG(actions, "actions is null");
    PRISM_CHECK_ARG(parity == 0 || parity == 1, "parity must be 0 or 1");
    return env_launch(env_seaquest_step_kernel, env_args(d, parity ^ 1, actions, u_in, draws_in), stream_);
}
