// g2048_expectimax.hip -- libg2048_search_hip.so (include/g2048_search.h): the expectimax agent, a decision per board and complete
// games in one launch. A library of its own because the main library's export table is closed (ABI 5). The value function and
// its order of operations are g2048_expectimax.h's; the game bookkeeping is g2048_play.h's.
//
//   decide_wave              one wavefront, one board. Every lane makes the root's four moves (the board is the wavefront's, so
//                            this is the same work in every lane, and a few hundred instructions) and numbers the (action, cell,
//                            tile) successors of the valid ones 0 .. items-1 without gaps, at most 120. Lane l takes successors l
//                            and l + 64: it places the tile and runs the remaining depth - 1 plies as nested loops in its own
//                            registers (ex_value<depth - 1>: no recursion, no stack, no run-time indexed array), and writes the
//                            product 0.9 / 0.1 x value to LDS under the successor's number. Numbering without gaps matters: a
//                            mid-game board has 4 to 6 empty cells, so 30 to 50 successors, which is one round with most lanes
//                            busy; a fixed 32 slots per action would leave two lanes in three idle and always take two rounds.
//                            Then lanes 0..3 each add one action's terms in cell order -- the fixed-order f64 sum of the
//                            definition, which is what makes the device agree with a CPU restatement bit for bit -- and divide;
//                            the four quotients go through LDS to every lane, which all pick the same action. The work is f64
//                            VALU and integer SWAR on registers; LDS carries 1 KiB of terms per wavefront, so neither LDS nor
//                            registers bound the occupancy. Lanes of a wavefront finish their subtrees at different times (the
//                            subtree sizes differ); nothing waits on another wavefront.
//   expectimax_actions_kernel  four wavefronts a block, wavefront w of block k decides board 4 k + w; wavefronts past n read the
//                            empty board (no valid move, no successor), pass the same two barriers and store nothing.
//   expectimax_play_kernel   one wavefront a block, one game in flight per wavefront: lane 0 owns the Game of g2048_play.h
//                            (claim_games, start_game, play_move: ticket refill, env step, milestones, reward sum, alive, the
//                            recorded actions), broadcasts its board, the wavefront decides, lane 0 moves. A wavefront leaves
//                            when its game is over and the queue is empty.
// Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/g2048_search.h"
#include "g2048_board.h"
#include "g2048_expectimax.h"
#include "g2048_host.h"
#include "g2048_play.h"

namespace {

using namespace g2048;

constexpr int kWavesPerBlock = 4;

// The decision for board b (wavefront-uniform) under the caller's mask; s_term / s_c: this wavefront's kExMaxItems and 4 doubles
// of LDS, s_c left holding the four values. Every wavefront of the block calls it the same number of times (two barriers).
template <int D>
__device__ __forceinline__ uint32_t decide_wave(const Board &b, uint32_t caller_mask, ExThr t, int lane, double *s_term, double *s_c)
{
    const ExRoot r = ex_root(b, caller_mask);
#pragma unroll 1
    for (uint32_t i = (uint32_t)lane; i < r.items; i += 64u) s_term[i] = ex_root_term<D>(r, i, t);
    __syncthreads();
    if (lane < 4) s_c[lane] = ex_root_chance(r, (uint32_t)lane, s_term);
    __syncthreads();
    return ex_pick(s_c[0], s_c[1], s_c[2], s_c[3]);
}

template <int D>
__global__ __launch_bounds__(64 * kWavesPerBlock) void expectimax_actions_kernel(const uint4 *__restrict__ boards, const uint8_t *__restrict__ mask4,
                                                                                 uint8_t *__restrict__ actions, double *__restrict__ values,
                                                                                 ExThr t, size_t n)
{
    __shared__ double s_term[kWavesPerBlock][kExMaxItems];
    __shared__ double s_c[kWavesPerBlock][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t i = (size_t)blockIdx.x * kWavesPerBlock + (size_t)wave;
    const bool live = i < n;
    Board b = {{0u, 0u, 0u, 0u}};                    // past n: the empty board has no valid move, so no successor
    uint32_t m = 0u;
    if (live) {
        const uint4 v = boards[i];
        b = Board{{v.x, v.y, v.z, v.w}};
        m = mask4 ? (uint32_t)mask4[i] : 15u;
    }
    const uint32_t a = decide_wave<D>(b, m, t, lane, s_term[wave], s_c[wave]);
    if (live && lane == 0) {
        actions[i] = (uint8_t)a;
        if (values) {
#pragma unroll
            for (int k = 0; k < 4; ++k) values[4 * i + (size_t)k] = s_c[wave][k];
        }
    }
}

template <int D>
__global__ __launch_bounds__(64) void expectimax_play_kernel(ExThr t, const PlayArgs par)
{
    __shared__ double s_term[kExMaxItems];
    __shared__ double s_c[4];
    __shared__ uint4 s_dir[G2048_DIR_TABLE_WORDS / 4];
    const int lane = threadIdx.x;
    load_dir_table(s_dir, threadIdx.x);
    __syncthreads();

    Game game{};
    bool active = false, drained = false;           // active: lane 0's; drained: wave-uniform, the queue has no game left
    for (;;) {
        if (!drained && claim_games(par, lane, lane == 0 && !active, game.index, drained)) {
            game = start_game(par, game.index);
            active = true;
        }
        if (__ballot(active) == 0ull) break;
        Board b;
#pragma unroll
        for (int w = 0; w < 4; ++w) b.w[w] = __builtin_amdgcn_readfirstlane(game.board.w[w]);
        const uint32_t a = decide_wave<D>(b, 15u, t, lane, s_term, s_c);
        if (lane == 0) active = !play_move(game, a, par, s_dir);
    }
}

template <class F>
auto with_depth(int depth, F &&f)
{
    switch (depth) {
        case 1: return f(int_c<1>{});
        case 2: return f(int_c<2>{});
        default: return f(int_c<3>{});
    }
}

// what both entry points check of the search's own settings: G2048_OK, or the error as `entry`'s
int check_search(const char *entry, int depth, int early_thr, int mid_thr)
{
    if (depth < 1 || depth > G2048_EXPECTIMAX_MAX_DEPTH)
        return fail(G2048_ERR_ARG, "%s: depth must be 1 .. %d", entry, G2048_EXPECTIMAX_MAX_DEPTH);
    if (early_thr < 0 || mid_thr < 0) return fail(G2048_ERR_ARG, "%s: negative threshold", entry);
    return G2048_OK;
}

}  // namespace

extern "C" {

const char *g2048_search_last_error(void) { return g_err; }

int g2048_search_abi_version(void) { return G2048_SEARCH_ABI_VERSION; }

int g2048_expectimax_actions(const void *boards, const uint8_t *mask4_or_null, uint8_t *actions_out, double *values_out_or_null, int depth,
                             int early_thr, int mid_thr, size_t n, void *stream)
{
    const char *entry = "g2048_expectimax_actions";
    if (n == 0) return G2048_OK;
    if (!boards || !actions_out) return fail(G2048_ERR_ARG, "%s: null pointer", entry);
    if (!aligned(boards, 16) || !aligned(values_out_or_null, 8))
        return fail(G2048_ERR_ARG, "%s: misaligned pointer (boards: 16 bytes; values: 8)", entry);
    if (const int rc = check_search(entry, depth, early_thr, mid_thr)) return rc;
    const size_t blocks = (n + kWavesPerBlock - 1) / kWavesPerBlock;
    if (blocks > 0x7fffffffu) return fail(G2048_ERR_ARG, "%s: n too large for one launch", entry);
    const ExThr t{(uint32_t)early_thr, (uint32_t)mid_thr};
    with_depth(depth, [&](auto D) {
        hipLaunchKernelGGL(expectimax_actions_kernel<decltype(D)::value>, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0,
                           static_cast<hipStream_t>(stream), static_cast<const uint4 *>(boards), mask4_or_null, actions_out, values_out_or_null, t, n);
    });
    return check_launch(entry);
}

size_t g2048_play_expectimax_workspace(size_t n_games) { return ticket_workspace_bytes(n_games); }

int g2048_play_expectimax_games(void *boards_inout, uint32_t *score_inout, int depth, int early_thr, int mid_thr, int32_t *moves_out,
                                int32_t *valid_out, int32_t *invalid_out, int32_t *milestone_move_out, double *reward_sum_out_or_null,
                                uint8_t *alive_out, uint8_t *actions_out_or_null, int max_moves, uint64_t seed, uint64_t game_id_base,
                                size_t n_games, uint32_t max_waves, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n_games == 0) return G2048_OK;
    // (the agent has no weights: the boards stand in for check_play_args' blob pointer)
    if (const int rc = check_play_args("g2048_play_expectimax", boards_inout, score_inout, boards_inout, moves_out, valid_out, invalid_out,
                                       milestone_move_out, reward_sum_out_or_null, alive_out, max_moves, n_games, workspace, workspace_bytes))
        return rc;
    if (const int rc = check_search("g2048_play_expectimax_games", depth, early_thr, mid_thr)) return rc;
    // auto: as many wavefronts as the chip holds at once (every later one would only find the queue empty)
    const size_t cap = max_waves ? (size_t)max_waves : (size_t)device_cus() * with_depth(depth, [](auto D) {
        return resident_per_cu(expectimax_play_kernel<decltype(D)::value>, 64);
    });
    if (cap == 0) return fail(G2048_ERR_HIP, "g2048_play_expectimax_games: no HIP device (occupancy query failed)");
    const size_t waves = std::min(std::min(n_games, cap), (size_t)0x7fffffffu);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const PlayArgs args{static_cast<unsigned long long *>(workspace), static_cast<uint4 *>(boards_inout), score_inout, n_games, seed,
                        game_id_base, moves_out, valid_out, invalid_out, reinterpret_cast<int4 *>(milestone_move_out), reward_sum_out_or_null,
                        alive_out, actions_out_or_null, max_moves};
    const ExThr t{(uint32_t)early_thr, (uint32_t)mid_thr};
    if (const int rc = reset_play_buffers("g2048_play_expectimax", workspace, actions_out_or_null, n_games, max_moves, s)) return rc;
    with_depth(depth, [&](auto D) {
        hipLaunchKernelGGL(expectimax_play_kernel<decltype(D)::value>, dim3((unsigned)waves), dim3(64), 0, s, t, args);
    });
    return check_launch("g2048_play_expectimax_games");
}

}  // extern "C"
