// g2048_qnet_collect.hip -- libg2048_collect_hip.so (include/g2048_collect.h): the hybrid agent's experience collection, the
// acting half of train_agent (agents/hybrid.py:1098-1127: select_action -> env.step -> remember, `steps` times for every
// environment) in ONE kernel launch that writes every transition straight into the prioritized replay ring (g2048_per.h). A
// library of its own because the main library's export table is closed (ABI 5); the forward pass, select_action and the planned
// decision are the main library's text, shared as g2048_qnet_forward.h, so a board's Q-values and its action are the bits
// g2048_qnet_forward / g2048_qnet_select_actions / g2048_qnet_beam_actions give.
//
//   qnet_collect_kernel   qnet_play_kernel's shape (g2048_qnet.hip) without its queue. A wavefront owns the 32 FIXED environments
//                         32 wave + lane (no ticket counter; environments past n read as the empty board and store nothing) and
//                         loops over the steps in lockstep: grids from the slots' boards in LDS, the shared forward, Q of the boards
//                         16..31 from lanes 0..15 to lanes 16..31, then each slot lane picks its action, steps its board
//                         (step_board_sel with the STEP-domain draw of (step index, id): g2048_step's), writes ring entry
//                         k = t n + i with plain stores -- 32 consecutive entries per array per wavefront and step -- and parks the
//                         board it goes on from: the next board, or fresh_board of the two EPISODE-domain draws when the step set
//                         DONE or the episode reached max_episode_steps (g2048_step's G2048_STEP_AUTO_RESET board). The forward
//                         leaves no registers over, so a slot's state (board, score, moves: 24 bytes) is parked in LDS round it and
//                         the launch arguments are read from LDS as well. One block barrier, after the prologue; no wavefront waits
//                         on another; no atomics.
//   per_max_kernel        (g2048_per_max.h) the priority M of every entry, as g2048_per_push finds it: a memset and one small
//                         launch in front, skipped for an empty ring. Three stream operations a call at the most.
// Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "../../include/g2048_collect.h"
#include "g2048_board.h"
#include "g2048_host.h"
#include "g2048_per_max.h"
#include "g2048_play.h"
#include "g2048_qnet_forward.h"
#include "g2048_rng.h"

namespace {

using namespace g2048;

// What a launch needs, copied to LDS in the prologue (inside CollectBeamArgs for the beam variant) and read from there after
// the forward, when registers are free.
struct CollectArgs {
    uint4 *boards;                                   // [n] in and out
    uint32_t *score;
    int32_t *moves;
    uint4 *states, *next_states;                     // the ring, [capacity] each
    uint8_t *actions;
    float *rewards;
    uint8_t *dones;
    float *priorities;
    uint8_t *flags_stream;                           // [steps][n], may be null
    const uint32_t *max_bits;                        // the bits of M (per_max_kernel); null for an empty ring: 1.0
    size_t n, capacity, start;                       // start = (head + size) % capacity: the slot of transition 0
    uint64_t seed, step_index0, id_base;
    float epsilon;
    int steps, max_episode_steps;
};

// The beam variant's two settings ride behind in a struct of their own, as QBeamPlayArgs does, so that without BEAM the kernel
// does not carry them.
struct CollectBeamArgs {
    CollectArgs c;
    uint32_t width, threshold;
};
template <bool BEAM> using CArgs = std::conditional_t<BEAM, CollectBeamArgs, CollectArgs>;
__device__ inline const CollectArgs &collect_args(const CollectArgs &a) { return a; }
__device__ inline const CollectArgs &collect_args(const CollectBeamArgs &a) { return a.c; }

// Slots parked in LDS, one column per slot; a slot lane reads and writes only its own.
struct CollectSlots {
    uint4 board[kWaveBoards];                        // the empty board for an environment past n: the forward reads it either way
    uint32_t score[kWaveBoards];
    int32_t moves[kWaveBoards];
};

template <bool BF16, bool BEAM>
__global__ __launch_bounds__(64 * kWaves, 2) void qnet_collect_kernel(const unsigned char *__restrict__ weights, int ff, int layers, const CArgs<BEAM> args)
{
    __shared__ CArgs<BEAM> all_args;
    __shared__ LookaheadLds<kWaveBoards> look[BEAM ? kWaves : 1];     // (not referenced without BEAM, and then not allocated)
    const CollectArgs &par = collect_args(all_args);
    __shared__ float lds[kWaves][kGrid][kWaveBoards];
    __shared__ CollectSlots wave_slots[kWaves];
    __shared__ uint4 s_dir[G2048_DIR_TABLE_WORDS / 4];
    const Layout lay(BF16, ff, layers);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), g = lane >> 4, col = lane & 15;
    CollectSlots &slots = wave_slots[wave];
    float (*grid)[kWaveBoards] = lds[wave];
    const size_t env0 = ((size_t)blockIdx.x * kWaves + (size_t)wave) * kWaveBoards;
    load_dir_table(s_dir, threadIdx.x);
    for (int i = lane; i < kGrid * kWaveBoards; i += 64) (&grid[0][0])[i] = 0.0f;
    if (lane < kWaveBoards) {
        const CollectArgs &in = collect_args(args);
        const size_t env = env0 + (size_t)lane;
        const bool live = env < in.n;
        slots.board[lane] = live ? in.boards[env] : make_uint4(0u, 0u, 0u, 0u);
        slots.score[lane] = live ? in.score[env] : 0u;
        slots.moves[lane] = live ? in.moves[env] : 0;
    }
    if (threadIdx.x == 0) all_args = args;
    __syncthreads();                                 // par, s_dir and the slots are there; the only block barrier
    if (env0 >= par.n) return;                       // the last block's surplus wavefronts
    const bool slot_lane = lane < kWaveBoards && env0 + (size_t)lane < par.n;

#pragma unroll 1
    for (int t = 0; t < par.steps; ++t) {
        // The blob's address is made opaque once per step as well as once per conv position (QNET_FORWARD_), as qnet_play_kernel
        // makes it once per move: otherwise every load of the forward that does not depend on the board is hoisted out of the
        // step loop and held in registers across it, which the forward has none to spare for.
        const unsigned char *W = weights;
        asm volatile("" : "+s"(W));
        const float *P = reinterpret_cast<const float *>(W + lay.params());

        QNET_GRID_(reinterpret_cast<const uint32_t *>(slots.board)[(16 * e + col) * 4 + g])
        wave_sync();                                 // the grids are there
        QNET_FORWARD_(BF16)

        // Q of slot s to lane s: q[0] of lanes 0..15 stays, q[1] of lane c goes to lane 16 + c
        float qs[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float up = __shfl(q[1][k], col);
            qs[k] = lane < 16 ? q[0][k] : up;
        }

        if (slot_lane) {
            const uint4 bw = slots.board[lane];
            const Board board{{bw.x, bw.y, bw.z, bw.w}};
            const size_t env = env0 + (size_t)lane;
            const uint64_t index = par.step_index0 + (uint64_t)t, id = par.id_base + env;
            const uint32_t mask = valid_mask_env(board);
            uint32_t a = exploit_action(qs[0], qs[1], qs[2], qs[3], mask);
            if constexpr (BEAM) {
                if (lookahead_planned(board, all_args.threshold)) {
                    LookaheadColumn<kWaveBoards> column{look[wave], lane};
                    a = lookahead_action(board, all_args.width, 0.0, nullptr, column);
                }
            }
            const float epsilon = par.epsilon;
            if (epsilon > 0.0f) {                    // (epsilon 0 never explores: no draw)
                bool explored;
                a = select_action(a, board, mask, epsilon, rng_keys(par.seed, DOM_POLICY, index), id, explored);
            }
            const Keys ks = rng_keys(par.seed, DOM_STEP, index);
            const uint4 s0 = s_dir[2u * a], s1 = s_dir[2u * a + 1u];
            const StepOut o = step_board_sel(board, DirSel{s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w}, rng_draw(ks.k0, ks.k1, id, 0u));

            // transition k lands behind the size + k entries before it: k < capacity, so one conditional subtraction wraps it
            const size_t k = (size_t)t * par.n + env;
            size_t slot = par.start + k;
            slot = slot >= par.capacity ? slot - par.capacity : slot;
            par.states[slot] = bw;
            par.next_states[slot] = make_uint4(o.board.w[0], o.board.w[1], o.board.w[2], o.board.w[3]);     // before any reset
            par.actions[slot] = (uint8_t)a;
            par.rewards[slot] = (float)o.reward;
            par.dones[slot] = (uint8_t)(o.flags & G2048_FLAG_DONE);
            par.priorities[slot] = par.max_bits ? __uint_as_float(*par.max_bits) : 1.0f;
            if (par.flags_stream) par.flags_stream[k] = (uint8_t)o.flags;

            Board cur = o.board;
            uint32_t score = slots.score[lane] + o.gain;
            int32_t moves = slots.moves[lane] + 1;
            if ((o.flags & G2048_FLAG_DONE) || (par.max_episode_steps > 0 && moves >= par.max_episode_steps)) {
                const Keys ke = rng_keys(par.seed, DOM_EPISODE, index);
                cur = fresh_board(rng_draw(ke.k0, ke.k1, id, 0u), rng_draw(ke.k0, ke.k1, id, 1u));
                score = 0u;
                moves = 0;
            }
            slots.board[lane] = make_uint4(cur.w[0], cur.w[1], cur.w[2], cur.w[3]);
            slots.score[lane] = score;
            slots.moves[lane] = moves;
        }
        wave_sync();                                 // the next step's grids see this step's boards
    }

    if (slot_lane) {
        const size_t env = env0 + (size_t)lane;
        par.boards[env] = slots.board[lane];
        par.score[env] = slots.score[lane];
        par.moves[env] = slots.moves[lane];
    }
}

}  // namespace

extern "C" {

const char *g2048_collect_last_error(void) { return g_err; }

int g2048_collect_abi_version(void) { return G2048_COLLECT_ABI_VERSION; }

size_t g2048_qnet_collect_workspace(size_t n)
{
    (void)n;
    return 64;
}

int g2048_qnet_collect(void *boards_inout, uint32_t *score_inout, int32_t *moves_inout, const void *packed, int dim_ff, int n_layers,
                       uint32_t opts, float epsilon, int beam_width, int search_depth, int threshold, uint64_t seed, uint64_t step_index0,
                       uint64_t env_id_base, size_t n, int steps, int max_episode_steps, void *states, void *next_states, uint8_t *actions,
                       float *rewards, uint8_t *dones, float *priorities, size_t capacity, size_t size, size_t head,
                       uint8_t *flags_stream_out_or_null, void *workspace, void *stream)
{
    const char *entry = "g2048_qnet_collect";
    if (n == 0) return G2048_OK;
    if (!boards_inout || !score_inout || !moves_inout || !packed || !states || !next_states || !actions || !rewards || !dones || !priorities ||
        !workspace)
        return fail(G2048_ERR_ARG, "%s: null pointer", entry);
    if (!aligned(boards_inout, 16) || !aligned(packed, 16) || !aligned(states, 16) || !aligned(next_states, 16) || !aligned(score_inout, 4) ||
        !aligned(moves_inout, 4) || !aligned(rewards, 4) || !aligned(priorities, 4) || !aligned(workspace, 4))
        return fail(G2048_ERR_ARG, "%s: misaligned pointer (boards, weights, states: 16 bytes; scores, counts, rewards, priorities, "
                                   "workspace: 4)", entry);
    if (const int rc = check_encoder_net(entry, (int)opts, "opts (precision)", dim_ff, n_layers)) return rc;
    if (!good_epsilon(epsilon)) return fail(G2048_ERR_ARG, "%s: epsilon must lie in [0, 1]", entry);
    const bool beam = beam_width != 0;
    if (beam) {
        if (const int rc = check_beam_settings(entry, beam_width, search_depth, threshold)) return rc;
        if (search_depth == 1)
            return fail(G2048_ERR_ARG, "%s: search_depth 1 asks the network about every candidate and is not collected in one launch; use "
                                       "the stepwise form (g2048_qnet_beam_expand, g2048_qnet_forward, g2048_qnet_beam_actions)", entry);
    }
    if (steps < 1) return fail(G2048_ERR_ARG, "%s: steps must be at least 1", entry);
    if (max_episode_steps < 0) return fail(G2048_ERR_ARG, "%s: max_episode_steps must be 0 (no cap) or positive", entry);
    if (size > capacity || head >= capacity) return fail(G2048_ERR_ARG, "%s: size must be at most capacity and head below it", entry);
    if (n > capacity / (size_t)steps)
        return fail(G2048_ERR_ARG, "%s: more transitions than the buffer's capacity (steps x n = %d x %zu, capacity %zu)", entry, steps, n, capacity);
    const size_t blocks = (n + kBlockBoards - 1) / kBlockBoards;
    if (blocks > 0x7fffffffu) return fail(G2048_ERR_ARG, "%s: n too large for one launch", entry);
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t *max_bits = static_cast<uint32_t *>(workspace);
    if (size) {
        if (const int rc = per_max_enqueue("g2048_qnet_collect: hipMemsetAsync", priorities, capacity, size, head, max_bits, s)) return rc;
    }
    const CollectArgs base{static_cast<uint4 *>(boards_inout), score_inout, moves_inout, static_cast<uint4 *>(states),
                           static_cast<uint4 *>(next_states), actions, rewards, dones, priorities, flags_stream_out_or_null,
                           size ? max_bits : nullptr, n, capacity, (head + size) % capacity, seed, step_index0, env_id_base, epsilon, steps,
                           max_episode_steps};
    with_bools(opts == G2048_POLICY_BF16, beam, [&](auto BF16, auto BEAM) {
        CArgs<decltype(BEAM)::value> args;
        if constexpr (decltype(BEAM)::value) args = CollectBeamArgs{base, (uint32_t)beam_width, (uint32_t)threshold};
        else args = base;
        hipLaunchKernelGGL((qnet_collect_kernel<decltype(BF16)::value, decltype(BEAM)::value>), dim3((unsigned)blocks), dim3(64 * kWaves), 0, s,
                           static_cast<const unsigned char *>(packed), dim_ff, n_layers, args);
    });
    return check_launch(entry);
}

}  // extern "C"
