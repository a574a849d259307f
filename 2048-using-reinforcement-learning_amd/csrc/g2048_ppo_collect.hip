// g2048_ppo_collect.hip -- libg2048_ppo_collect_hip.so (include/g2048_ppo_collect.h): the PPO agent's experience collection, the
// acting loop of train.py:55-90 (PPOAgent.get_action under the env's valid-move mask -> Game2048Env.step -> auto-reset, `steps`
// times for every environment) in ONE kernel launch that writes every trajectory row g2048.RolloutCollector keeps. A library of
// its own because the main library's export table is closed (ABI 5); the layers of the actor and the critic are the main
// library's text, shared as g2048_policy_forward.h, and the env step's constants are g2048_step_table.h's, so a board's
// probabilities, its value and its step are the bits g2048_policy_forward and g2048_rollout_step give.
//
//   ppo_collect_kernel   policy_play_kernel's shape (g2048_policy.hip) without its queue. One wavefront is one block and owns the
//                        S = 16 E FIXED environments S block + lane (E = 2 in f32, 4 in bf16; no ticket counter; environments
//                        past n read as the empty board and store nothing) and loops over the steps in lockstep. Per step: the
//                        slot lanes store the observation and the valid-move mask of the board they hold (row t) and write the
//                        board to LDS, every lane reads the dword its layer-1 B operand needs, the wavefront runs the shared
//                        layers for the actor and then for the critic, lanes 0..15 write probabilities and values to LDS, and
//                        each slot lane samples its action, steps its board (rollout_step_kernel's statements) and stores its
//                        trajectory entries: S consecutive entries per array, wavefront and step. Board and score stay in
//                        registers; row `steps` of the observations and masks follows the last step. All slots of a wavefront
//                        are at the same step, so the three RNG key pairs are wavefront-uniform. No atomics, no workspace, no
//                        wavefront waits on another.
// Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "../../include/g2048_ppo_collect.h"
#include "g2048_board.h"
#include "g2048_host.h"
#include "g2048_policy_forward.h"
#include "g2048_rng.h"

namespace {

using namespace g2048;

#include "g2048_step_table.h"

// What a launch needs; the kernel reads it from the kernel-argument segment where it uses it.
struct PpoCollectArgs {
    uint4 *boards;                                   // [n] in and out
    uint32_t *score;
    uint8_t *actions;                                // [steps][n] each, down to state_max
    float *prob;
    void *reward;                                    // float, or double under G2048_STEP_REWARD_F64
    uint8_t *flags;
    float *value;                                    // null without a critic
    uint4 *next_boards;                              // may be null
    uint8_t *state_max;                              // may be null
    void *obs;                                       // [steps + 1][n][16], may be null
    uint8_t *mask;                                   // [steps + 1][n], may be null
    const unsigned long long *counter;               // may be null
    uint64_t seed, step_index0, id_base;
    size_t n;
    int steps;
    uint32_t opts;                                   // G2048_STEP_REWARD_F64 | obs kind << G2048_ROLLOUT_OBS_SHIFT
};

// The blob's address is made opaque once per step, as qnet_collect_kernel makes its own: otherwise the loads of the layers that do
// not depend on the board are hoisted out of the step loop and held in registers across it. What goes through the statement is a
// zero OFFSET, not the pointer: behind an opaque pointer the compiler no longer knows the address space, every fragment load
// becomes a flat load, and a flat load is waited for with vmcnt(0) -- one memory round trip per fragment (docs/LOG.md R35).
__device__ __forceinline__ const unsigned char *opaque_blob(const unsigned char *blob)
{
    uint32_t zero = 0u;
    asm volatile("" : "+s"(zero));
    return blob + zero;
}

template <bool BF16, int E, bool CRITIC>
__global__ __launch_bounds__(64) void ppo_collect_kernel(const unsigned char *__restrict__ actor, const unsigned char *__restrict__ critic,
                                                         const PpoCollectArgs par)
{
    constexpr int S = 16 * E;
    using P = Packed<BF16>;
    __shared__ uint4 s_board[S];
    __shared__ float4 s_prob[S];
    __shared__ float s_value[CRITIC ? S : 1];
    __shared__ uint4 s_dir[kStepTableWords / 4];             // selector words + the reward's f64 constants + the observation values
    const float *const s_obs = reinterpret_cast<const StepTable *>(s_dir)->obs;
    const TenthFromLds tenth{reinterpret_cast<const StepTable *>(s_dir)};
    const uint2 table_word = step_table_word();
    const int lane = threadIdx.x, h = lane >> 4, col = lane & 15;
    const size_t env = (size_t)blockIdx.x * S + (size_t)lane;
    const bool slot_lane = lane < S, live = slot_lane && env < par.n;
    Board board = {{0u, 0u, 0u, 0u}};                        // an environment past n: the empty board, the forward reads it either way
    uint32_t score = 0u;
    if (live) {
        const uint4 b = par.boards[env];
        board = Board{{b.x, b.y, b.z, b.w}};
        score = par.score[env];
    }
    // the index may come from a device counter so that a captured hipGraph of a collect can be replayed
    const uint64_t index0 = par.step_index0 + (par.counter ? (uint64_t)*par.counter : 0ull);
    step_table_store(s_dir, table_word);
    const uint64_t id = par.id_base + env;
    const uint32_t kind = (par.opts >> G2048_ROLLOUT_OBS_SHIFT) & 3u;

#pragma unroll 1
    for (int t = 0;; ++t) {
        // row t of the observations and masks is the board the environment goes on from: row 0 the board the call starts from,
        // row `steps` the one it ends on
        const uint32_t mask = valid_mask_env(board);
        if (live) {
            const size_t row = (size_t)t * par.n + env;
            if (par.mask) par.mask[row] = (uint8_t)mask;
            if (par.obs) store_observation(par.obs, row, board, kind, s_obs);
        }
        if (t == par.steps) break;

        // slot lanes -> LDS -> each lane's B-operand dword of every tile
        if (slot_lane) s_board[lane] = make_uint4(board.w[0], board.w[1], board.w[2], board.w[3]);
        __syncthreads();
        f4 x[E][2];
#pragma unroll
        for (int e = 0; e < E; ++e) board_operand(reinterpret_cast<const uint32_t *>(s_board)[(16 * e + col) * 4 + h], x[e]);
        {
            const unsigned char *W = opaque_blob(actor);
            const float *bias = reinterpret_cast<const float *>(W + P::kBias);
            POLICY_LAYERS_(BF16, E, W, bias, lane, h, x, out);
            if (h == 0) {
#pragma unroll
                for (int e = 0; e < E; ++e) s_prob[16 * e + col] = softmax4(out[e][0]);
            }
        }
        if constexpr (CRITIC) {                              // the same wavefront, after the actor; the value does not feed the action
            const unsigned char *W = opaque_blob(critic);
            const float *bias = reinterpret_cast<const float *>(W + P::kBias);
            POLICY_LAYERS_(BF16, E, W, bias, lane, h, x, out);
            if (h == 0) {
#pragma unroll
                for (int e = 0; e < E; ++e) s_value[16 * e + col] = out[e][0][0];
            }
        }
        __syncthreads();

        if (live) {                                          // rollout_step_kernel's statements, for entry i = t n + env
            const uint64_t index = index0 + (uint64_t)t;
            const Keys kp = rng_keys(par.seed, DOM_POLICY, index), ks = rng_keys(par.seed, DOM_STEP, index), ke = rng_keys(par.seed, DOM_EPISODE, index);
            const float4 p = s_prob[lane];
            float pa;
            const uint32_t a = sample_action(p.x, p.y, p.z, p.w, mask, rng_draw(kp.k0, kp.k1, id, 0u), pa);
            const uint4 si = s_dir[2u * a], so = s_dir[2u * a + 1u];
            const StepOut o = step_board_sel(board, DirSel{si.x, si.y, si.z, si.w, so.x, so.y, so.z, so.w}, rng_draw(ks.k0, ks.k1, id, 0u), tenth);
            const size_t i = (size_t)t * par.n + env;
            if (par.next_boards) par.next_boards[i] = make_uint4(o.board.w[0], o.board.w[1], o.board.w[2], o.board.w[3]);     // before any reset
            if (par.state_max) par.state_max[i] = (uint8_t)max_code(board);
            board = o.board;
            score += o.gain;
            if (o.flags & G2048_FLAG_DONE) {
                board = fresh_board(rng_draw(ke.k0, ke.k1, id, 0u), rng_draw(ke.k0, ke.k1, id, 1u));
                score = 0u;
            }
            par.actions[i] = (uint8_t)a;
            par.prob[i] = pa;
            if (par.opts & G2048_STEP_REWARD_F64) static_cast<double *>(par.reward)[i] = o.reward;
            else static_cast<float *>(par.reward)[i] = (float)o.reward;
            par.flags[i] = (uint8_t)o.flags;
            if constexpr (CRITIC) par.value[i] = s_value[lane];
        }
    }

    if (live) {
        par.boards[env] = make_uint4(board.w[0], board.w[1], board.w[2], board.w[3]);
        par.score[env] = score;
    }
}

}  // namespace

extern "C" {

const char *g2048_ppo_collect_last_error(void) { return g_err; }

int g2048_ppo_collect_abi_version(void) { return G2048_PPO_COLLECT_ABI_VERSION; }

int g2048_ppo_collect(void *boards_inout, uint32_t *score_inout, const void *actor_packed, const void *critic_packed_or_null,
                      uint8_t *actions_out, float *prob_out, void *reward_out, uint8_t *flags_out, float *value_out_or_null,
                      void *obs_out_or_null, uint8_t *mask4_out_or_null, void *next_boards_out_or_null, uint8_t *state_maxcode_out_or_null,
                      uint64_t seed, uint64_t step_index0, const unsigned long long *step_counter_or_null, uint64_t env_id_base, size_t n,
                      int steps, uint32_t opts, void *stream)
{
    const char *entry = "g2048_ppo_collect";
    if (n == 0) return G2048_OK;
    if (!boards_inout || !score_inout || !actor_packed || !actions_out || !prob_out || !reward_out || !flags_out)
        return fail(G2048_ERR_ARG, "%s: null pointer", entry);
    if (!critic_packed_or_null != !value_out_or_null)
        return fail(G2048_ERR_ARG, "%s: critic_packed and value_out must both be given or both be NULL", entry);
    const uint32_t kind = (opts >> G2048_ROLLOUT_OBS_SHIFT) & 3u, precision = (opts >> G2048_PPO_COLLECT_PRECISION_SHIFT) & 0xfu;
    if (opts & ~(G2048_STEP_REWARD_F64 | G2048_STEP_AUTO_RESET | (3u << G2048_ROLLOUT_OBS_SHIFT) | (0xfu << G2048_PPO_COLLECT_PRECISION_SHIFT)))
        return fail(G2048_ERR_ARG, "%s: unknown opts 0x%x", entry, opts);
    if (kind > G2048_OBS_BF16) return fail(G2048_ERR_ARG, "%s: unknown observation dtype in opts", entry);
    if (!good_precision((int)precision)) return fail(G2048_ERR_ARG, "%s: unknown precision in opts", entry);
    if (!aligned(boards_inout, 16) || !aligned(actor_packed, 16) || !aligned(critic_packed_or_null, 16) || !aligned(obs_out_or_null, 16) ||
        !aligned(next_boards_out_or_null, 16) || !aligned(reward_out, (opts & G2048_STEP_REWARD_F64) ? 8 : 4) ||
        !aligned(step_counter_or_null, 8) || !aligned(score_inout, 4) || !aligned(prob_out, 4) || !aligned(value_out_or_null, 4))
        return fail(G2048_ERR_ARG, "%s: misaligned pointer (boards, next boards, weights, obs: 16 bytes; f64 reward, counter: 8; scores, "
                                   "prob, value, f32 reward: 4)", entry);
    if (steps < 1) return fail(G2048_ERR_ARG, "%s: steps must be at least 1", entry);
    const bool bf16 = precision == G2048_POLICY_BF16;
    const size_t slots = 16 * (size_t)(bf16 ? kTilesBF16 : kTilesF32);
    const size_t blocks = (n + slots - 1) / slots;
    if (blocks > 0x7fffffffu) return fail(G2048_ERR_ARG, "%s: n too large for one launch", entry);
    const PpoCollectArgs args{static_cast<uint4 *>(boards_inout), score_inout, actions_out, prob_out, reward_out, flags_out, value_out_or_null,
                              static_cast<uint4 *>(next_boards_out_or_null), state_maxcode_out_or_null, obs_out_or_null, mask4_out_or_null,
                              step_counter_or_null, seed, step_index0, env_id_base, n, steps, opts};
    const auto *a = static_cast<const unsigned char *>(actor_packed);
    const auto *c = static_cast<const unsigned char *>(critic_packed_or_null);
    with_precision(bf16, [&](auto BF16, auto E) {
        with_bool(c != nullptr, [&](auto CRITIC) {
            hipLaunchKernelGGL((ppo_collect_kernel<decltype(BF16)::value, decltype(E)::value, decltype(CRITIC)::value>), dim3((unsigned)blocks),
                               dim3(64), 0, static_cast<hipStream_t>(stream), a, c, args);
        });
    });
    return check_launch(entry);
}

}  // extern "C"
