// g2048_play.h -- the game-slot core of the kernels that play complete games of a network in one launch (policy_play_kernel,
// tpolicy_play_kernel, qnet_play_kernel): what a launch's games need, one slot's state, how idle slots take the next games from
// the ticket counter, and everything that happens to a slot once its action is chosen. Device code, included by those three
// files (and, for the direction table alone, by g2048_qnet_collect.hip). The kernels differ in the forward pass before it, in how many slots a wavefront owns, and in where a
// slot's state lives between moves: policy_play_kernel keeps a Game in registers, the other two have none to spare and park it
// in LDS (PlaySlots), loading and storing it around the move.
//
// The games do not depend on which wavefront or slot plays them: a game's draws are keyed by (seed, domain, its own move index,
// id_base + its index) alone. Nothing here waits on another wavefront: no spin, no grid barrier.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/g2048.h"
#include "g2048_board.h"
#include "g2048_rng.h"

namespace g2048 {

// What every game launch needs. The kernels that park their slots in LDS copy it there too (inside their own argument
// struct), and the slot lanes read it after the forward, when registers are free: the forward alone takes most of the 106
// scalar registers, and these would be two dozen more held across it.
struct PlayArgs {
    unsigned long long *ticket;                      // the next game index not yet taken (zeroed before the launch)
    uint4 *boards;
    uint32_t *score;
    size_t n;
    uint64_t seed, id_base;
    int32_t *moves_out, *valid_out, *invalid_out;
    int4 *milestone_out;
    double *reward_out;                              // may be null
    uint8_t *alive_out, *actions_out;                // actions_out may be null
    int max_moves;
};

struct Game {                                        // one slot's state while its game is live
    Board board;
    uint32_t score;
    size_t index;                                    // which game of the launch
    int32_t moves, valid;
    int32_t milestone[8];                            // the move at which tiles 64 .. 8192 first appeared, -1 = not yet
    double reward;                                   // the env rewards summed in move order
};

// Slots parked in LDS, one column per slot; a slot lane reads and writes only its own.
template <int S>
struct PlaySlots {
    uint4 board[S];                                  // the empty board while the slot is idle: the forward reads it either way
    int4 milestone[2][S];
    double reward[S];
    unsigned long long game[S];
    uint32_t score[S];
    int32_t moves[S], valid[S];
    uint32_t active[S];

    __device__ void clear(int s)
    {
        board[s] = make_uint4(0u, 0u, 0u, 0u);
        active[s] = 0u;
    }
    __device__ Game load(int s) const
    {
        const uint4 b = board[s];
        const int4 m0 = milestone[0][s], m1 = milestone[1][s];
        return Game{Board{{b.x, b.y, b.z, b.w}}, score[s], (size_t)game[s], moves[s], valid[s], {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w},
                    reward[s]};
    }
    __device__ void store(int s, const Game &v)         // what a move changes; `game` and `active` are set when the game starts
    {
        board[s] = make_uint4(v.board.w[0], v.board.w[1], v.board.w[2], v.board.w[3]);
        milestone[0][s] = make_int4(v.milestone[0], v.milestone[1], v.milestone[2], v.milestone[3]);
        milestone[1][s] = make_int4(v.milestone[4], v.milestone[5], v.milestone[6], v.milestone[7]);
        reward[s] = v.reward;
        score[s] = v.score;
        moves[s] = v.moves;
        valid[s] = v.valid;
    }
};

__device__ const uint32_t kPlayDirTable[G2048_DIR_TABLE_WORDS] = G2048_DIR_TABLE_INIT;

// the direction table into the block's LDS (the block has at least G2048_DIR_TABLE_WORDS threads; a barrier follows at the caller)
__device__ inline void load_dir_table(uint4 (&s_dir)[G2048_DIR_TABLE_WORDS / 4], unsigned thread)
{
    if (thread < G2048_DIR_TABLE_WORDS) reinterpret_cast<uint32_t *>(s_dir)[thread] = kPlayDirTable[thread];
}

// The wavefront's idle slots (lanes with `idle` set) take the next games from the ticket counter: one atomicAdd per wavefront
// for all of them, the indices spread over the lanes by an mbcnt prefix. True on a lane that got a game, `game` its index
// (written on such a lane only); `drained` (wavefront-uniform) once the queue has no game left, after which the caller need
// not ask again. All lanes of the wavefront call it together.
__device__ inline bool claim_games(const PlayArgs &par, int lane, bool idle, size_t &game, bool &drained)
{
    const uint64_t mask = __ballot(idle);
    if (mask == 0ull) return false;
    const uint32_t cnt = (uint32_t)__popcll(mask);
    unsigned long long got = 0ull;
    if (lane == 0) got = atomicAdd(par.ticket, (unsigned long long)cnt);
    const uint64_t base = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(got >> 32)) << 32) |
                          __builtin_amdgcn_readfirstlane((uint32_t)got);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    drained = base + cnt >= par.n;
    const bool won = idle && base + rank < par.n;
    if (won) game = (size_t)(base + rank);
    return won;
}

__device__ inline Game start_game(const PlayArgs &par, size_t game)
{
    const uint4 b = par.boards[game];
    return Game{Board{{b.x, b.y, b.z, b.w}}, par.score[game], game, 0, 0, {-1, -1, -1, -1, -1, -1, -1, -1}, 0.0};
}

// claim_games for slots parked in LDS: a lane that got a game fills its slot. Returns whether the lane's slot is live now.
template <int S>
__device__ inline bool refill_slots(PlaySlots<S> &slots, const PlayArgs &par, int lane, bool slot_lane, bool active, bool &drained)
{
    size_t game;
    if (!drained && claim_games(par, lane, slot_lane && !active, game, drained)) {
        slots.store(lane, start_game(par, game));
        slots.game[lane] = game;
        slots.active[lane] = 1u;
        active = true;
    }
    return active;
}

// The action of a policy with probabilities p for game `id` at its move t (the PPO actor and the transformer policy): the
// argmax over the valid moves, or a sample among the valid moves (masked) or among all four (unmasked).
__device__ inline uint32_t policy_action(float4 p, uint32_t mask, uint32_t mode, uint64_t seed, int32_t t, uint64_t id)
{
    if (mode == G2048_PLAY_POLICY_GREEDY) {                  // argmax over the valid moves, ties to the lowest index
        const uint32_t m = mask ? mask : 15u;                // (no valid move: all four, as sample_action does)
        float best = 0.0f;
        uint32_t a = 4u;
#pragma unroll
        for (int k = 3; k >= 0; --k) {
            const float v = k == 0 ? p.x : k == 1 ? p.y : k == 2 ? p.z : p.w;
            if (((m >> k) & 1u) && (a == 4u || v >= best)) { a = (uint32_t)k; best = v; }
        }
        return a;
    }
    const Keys kp = rng_keys(seed, DOM_POLICY, (uint64_t)t);
    float pa;
    return sample_action(p.x, p.y, p.z, p.w, mode == G2048_PLAY_POLICY_MASKED ? mask : 15u, rng_draw(kp.k0, kp.k1, id, 0u), pa);
}

// The game makes move `a`: the env step, the action byte, score, reward sum, milestones and counters. True when that ended
// the game (done, or max_moves reached): its results are written and the slot is free.
__device__ inline bool play_move(Game &s, uint32_t a, const PlayArgs &par, const uint4 *s_dir)
{
    const int32_t t = s.moves;
    const Keys ks = rng_keys(par.seed, DOM_STEP, (uint64_t)t);
    const uint4 s0 = s_dir[2u * a], s1 = s_dir[2u * a + 1u];
    const StepOut o = step_board_sel(s.board, DirSel{s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w},
                                     rng_draw(ks.k0, ks.k1, par.id_base + s.index, 0u));
    if (par.actions_out) par.actions_out[s.index * (size_t)par.max_moves + (size_t)t] = (uint8_t)a;
    s.board = o.board;
    s.score += o.gain;
    s.reward += o.reward;
    const int32_t maxcode = (int32_t)(o.flags >> G2048_FLAG_MAXCODE_SHIFT);
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (s.milestone[k] < 0 && maxcode >= 6 + k) s.milestone[k] = t;       // tiles 64 .. 8192, as g2048_track_episodes records them
    s.valid += (o.flags & G2048_FLAG_VALID) ? 1 : 0;
    s.moves = t + 1;
    const bool done = (o.flags & G2048_FLAG_DONE) != 0u;
    if (!done && s.moves != par.max_moves) return false;
    const size_t g = s.index;
    par.boards[g] = make_uint4(s.board.w[0], s.board.w[1], s.board.w[2], s.board.w[3]);
    par.score[g] = s.score;
    par.moves_out[g] = s.moves;
    par.valid_out[g] = s.valid;
    par.invalid_out[g] = s.moves - s.valid;
    par.milestone_out[2 * g] = make_int4(s.milestone[0], s.milestone[1], s.milestone[2], s.milestone[3]);
    par.milestone_out[2 * g + 1] = make_int4(s.milestone[4], s.milestone[5], s.milestone[6], s.milestone[7]);
    if (par.reward_out) par.reward_out[g] = s.reward;
    par.alive_out[g] = done ? 0 : 1;
    return true;
}

// play_move for a slot parked in LDS: load, move, then store the state back or clear the slot
template <int S>
__device__ inline void play_slot_move(PlaySlots<S> &slots, int lane, Game &s, uint32_t a, const PlayArgs &par, const uint4 *s_dir)
{
    if (play_move(s, a, par, s_dir)) slots.clear(lane);
    else slots.store(lane, s);
}

}  // namespace g2048
