// g2048_tpolicy_collect.hip -- libg2048_tpolicy_collect_hip.so (include/g2048_tpolicy_collect.h): the transformer policy's
// experience collection, the acting loop of train.py:55-90 (the policy's probabilities sampled under the env's valid-move mask ->
// Game2048Env.step -> auto-reset, `steps` times for every environment) in ONE kernel launch that writes every trajectory row
// g2048.RolloutCollector keeps. A library of its own because the main library's export table is closed (ABI 5); the forward is the
// main library's text, shared as g2048_tpolicy_forward.h, and the env step's constants are g2048_step_table.h's, so a board's
// probabilities, its value and its step are the bits g2048_tpolicy_forward and g2048_rollout_step give.
//
//   tpolicy_collect_kernel   tpolicy_forward_kernel's geometry (g2048_tpolicy.hip): a block of four wavefronts, 16 boards -- here the
//                            16 FIXED environments 16 block + s, slot s on lane s of wavefront 0, its board one of the four of
//                            wavefront s / 4 (no ticket counter; environments past n read as the empty board and store nothing).
//                            The block loops over the steps in lockstep. Per step: the slot lanes store the observation and the
//                            valid-move mask of the board they hold (row t); after a barrier every wavefront reads the cell bytes
//                            of its four boards from LDS and the block runs the shared forward; the head tile lands on lanes 0..15
//                            of wavefront 0 with column = slot, the value on lanes 16..31, from where the slot lane reads it across
//                            the lanes; each slot lane samples its action, steps its board (rollout_step_kernel's statements) and
//                            stores its trajectory entries while wavefronts 1..3 wait at the next step's barrier. The forward
//                            leaves no registers over (226 / 245 VGPRs), so a slot's board and score are parked in LDS between the
//                            steps, as tpolicy_play_kernel parks its slots, and so are the launch arguments. Row `steps` of the observations and masks follows the
//                            last step. All slots of a block are at the same step, so the three RNG key pairs are block-uniform.
//                            No atomics, no workspace, no block waits on another.
// Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "../../include/g2048_tpolicy_collect.h"
#include "g2048_board.h"
#include "g2048_host.h"
#include "g2048_rng.h"
#include "g2048_tpolicy_forward.h"

namespace {

using namespace g2048;

#include "g2048_step_table.h"

// What a launch needs, passed by value; the kernel parks it in LDS (s_par) and reads a field where it uses it.
struct TpolicyCollectArgs {
    uint4 *boards;                                   // [n] in and out
    uint32_t *score;
    uint8_t *actions;                                // [steps][n] each, down to state_max
    float *prob;
    void *reward;                                    // float, or double under G2048_STEP_REWARD_F64
    uint8_t *flags;
    float *value;                                    // may be null
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

// The blob's address is made opaque once per step, as ppo_collect_kernel makes its own (g2048_ppo_collect.hip): otherwise the loads
// of the forward that do not depend on the board (the embedding, the head biases) are hoisted out of the step loop and held in
// registers across it, which the forward has none to spare for. What goes through the statement is a zero OFFSET, not the pointer:
// behind an opaque pointer the compiler no longer knows the address space, every fragment load becomes a flat load, and a flat
// load is waited for with vmcnt(0) -- one memory round trip per fragment (docs/LOG.md R35).
// Only the bf16 instantiation does it. The f32 one has the registers for what is hoisted (254 VGPRs, no scratch), and with the
// offset its feed-forward loop loads the weight fragments one at a time, each waited for with vmcnt(0), where without it the loop
// keeps up to six in flight as tpolicy_forward_kernel's does: 729 against 598 us a step at dim_ff 2,048 (docs/LOG.md R36). The bf16
// one compiles to 36 bytes of scratch without the offset, and its loop loads one at a time either way; that is its open loss.
__device__ __forceinline__ const unsigned char *opaque_blob(const unsigned char *blob)
{
    uint32_t zero = 0u;
    asm volatile("" : "+s"(zero));
    return blob + zero;
}

constexpr int kSlots = kWaves * kE;

template <bool BF16>
__global__ __launch_bounds__(64 * kWaves, 2) void tpolicy_collect_kernel(const unsigned char *__restrict__ weights, int ff, int layers,
                                                                       const TpolicyCollectArgs args)
{
    // The arguments arrive as a by-value struct; wavefront 0, their only reader inside the step loop, keeps a copy in LDS and reads a
    // field where it uses it, through an offset made opaque once per step. Read from the argument segment they are loop invariants
    // held in SGPRs across the forward: that build spilled 22 - 24 SGPRs to VGPR lanes, and it issued the weight fragments of fc1, fc2
    // and the heads one at a time, each waited for with vmcnt(0), where this one keeps two in flight as tpolicy_forward_kernel does
    // (docs/LOG.md R36 has both builds' rates).
    __shared__ TpolicyCollectArgs s_par;
    __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
    __shared__ uint4 s_board[kSlots];                        // a slot's board and score between the steps; the encoder's input
    __shared__ uint32_t s_score[kSlots];
    __shared__ uint4 s_dir[kStepTableWords / 4];             // selector words + the reward's f64 constants + the observation values
    const float *const s_obs = reinterpret_cast<const StepTable *>(s_dir)->obs;
    const TenthFromLds tenth{reinterpret_cast<const StepTable *>(s_dir)};
    const Layout lay(BF16, ff, layers);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), g = lane >> 4, col = lane & 15;
    const bool slot_lane = wave == 0 && lane < kSlots;
    const size_t env = (size_t)blockIdx.x * kSlots + (size_t)lane;
    const bool live = slot_lane && env < args.n;
    if (threadIdx.x == 0) s_par = args;                      // (wavefront 0's own write precedes its reads: no barrier)
    if (wave == 0) {                                         // the table's only reader; its own write precedes its reads
        const uint2 table_word = step_table_word();
        uint4 b = make_uint4(0u, 0u, 0u, 0u);                // an environment past n: the empty board, the forward reads it either way
        uint32_t score = 0u;
        if (live) {
            b = args.boards[env];
            score = args.score[env];
        }
        step_table_store(s_dir, table_word);
        if (slot_lane) {
            s_board[lane] = b;
            s_score[lane] = score;
        }
    }
    const uint32_t kind = (args.opts >> G2048_ROLLOUT_OBS_SHIFT) & 3u;

#pragma unroll 1
    for (int t = 0;; ++t) {
        const TpolicyCollectArgs &par = *reinterpret_cast<const TpolicyCollectArgs *>(opaque_blob(reinterpret_cast<const unsigned char *>(&s_par)));
        // row t of the observations and masks is the board the environment goes on from: row 0 the board the call starts from,
        // row `steps` the one it ends on
        if (live) {
            const uint4 b = s_board[lane];
            const Board board{{b.x, b.y, b.z, b.w}};
            const uint32_t mask = valid_mask_env(board);
            const size_t row = (size_t)t * par.n + env;
            if (par.mask) par.mask[row] = (uint8_t)mask;
            if (par.obs) store_observation(par.obs, row, board, kind, s_obs);
        }
        if (t == args.steps) break;                          // (block-uniform, from the argument segment: every wavefront reads it)
        __syncthreads();                                     // the slots' boards are there

        const unsigned char *W = BF16 ? opaque_blob(weights) : weights;      // (opaque_blob has the reason for the difference)
        const float *P = reinterpret_cast<const float *>(W + lay.params());
#define TPOLICY_SLOT_CELL_ reinterpret_cast<const uint8_t *>(s_board)[(kE * wave + e) * 16 + col]
        TPOLICY_ENCODER_(BF16, TPOLICY_SLOT_CELL_);
        TPOLICY_DENSE_(BF16);
        if (wave != 0) continue;                             // to the next step's barrier, where wavefront 0 joins after its slots' steps
        TPOLICY_HEADS_(BF16);
        const float value = __shfl(z[0], kSlots + col);      // the critic's row: register 0 of lanes 16..31, column = slot

        if (live) {                                          // rollout_step_kernel's statements, for entry i = t n + env
            // the index may come from a device counter so that a captured hipGraph of a collect can be replayed
            const uint64_t index = par.step_index0 + (par.counter ? (uint64_t)*par.counter : 0ull) + (uint64_t)t;
            const uint64_t id = par.id_base + env;
            const Keys kp = rng_keys(par.seed, DOM_POLICY, index), ks = rng_keys(par.seed, DOM_STEP, index), ke = rng_keys(par.seed, DOM_EPISODE, index);
            const uint4 b = s_board[lane];
            Board board{{b.x, b.y, b.z, b.w}};
            uint32_t score = s_score[lane];
            const uint32_t mask = valid_mask_env(board);
            const float4 p = softmax4(z);
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
            if (par.value) par.value[i] = value;
            s_board[lane] = make_uint4(board.w[0], board.w[1], board.w[2], board.w[3]);
            s_score[lane] = score;
        }
    }

    if (live) {
        args.boards[env] = s_board[lane];
        args.score[env] = s_score[lane];
    }
}

}  // namespace

extern "C" {

const char *g2048_tpolicy_collect_last_error(void) { return g_err; }

int g2048_tpolicy_collect_abi_version(void) { return G2048_TPOLICY_COLLECT_ABI_VERSION; }

int g2048_tpolicy_collect(void *boards_inout, uint32_t *score_inout, const void *packed, int dim_ff, int n_layers, uint8_t *actions_out,
                          float *prob_out, void *reward_out, uint8_t *flags_out, float *value_out_or_null, void *obs_out_or_null,
                          uint8_t *mask4_out_or_null, void *next_boards_out_or_null, uint8_t *state_maxcode_out_or_null, uint64_t seed,
                          uint64_t step_index0, const unsigned long long *step_counter_or_null, uint64_t env_id_base, size_t n, int steps,
                          uint32_t opts, void *stream)
{
    const char *entry = "g2048_tpolicy_collect";
    if (n == 0) return G2048_OK;
    if (!boards_inout || !score_inout || !packed || !actions_out || !prob_out || !reward_out || !flags_out)
        return fail(G2048_ERR_ARG, "%s: null pointer", entry);
    if (!aligned(boards_inout, 16) || !aligned(packed, 16) || !aligned(obs_out_or_null, 16) || !aligned(next_boards_out_or_null, 16) ||
        !aligned(reward_out, (opts & G2048_STEP_REWARD_F64) ? 8 : 4) || !aligned(step_counter_or_null, 8) || !aligned(score_inout, 4) ||
        !aligned(prob_out, 4) || !aligned(value_out_or_null, 4))
        return fail(G2048_ERR_ARG, "%s: misaligned pointer (boards, next boards, weights, obs: 16 bytes; f64 reward, counter: 8; scores, "
                                   "prob, value, f32 reward: 4)", entry);
    if (steps < 1) return fail(G2048_ERR_ARG, "%s: steps must be at least 1", entry);
    const uint32_t kind = (opts >> G2048_ROLLOUT_OBS_SHIFT) & 3u, precision = (opts >> G2048_TPOLICY_COLLECT_PRECISION_SHIFT) & 0xfu;
    if (opts & ~(G2048_STEP_REWARD_F64 | G2048_STEP_AUTO_RESET | (3u << G2048_ROLLOUT_OBS_SHIFT) | (0xfu << G2048_TPOLICY_COLLECT_PRECISION_SHIFT)))
        return fail(G2048_ERR_ARG, "%s: unknown opts 0x%x", entry, opts);
    if (kind > G2048_OBS_BF16) return fail(G2048_ERR_ARG, "%s: unknown observation dtype in opts", entry);
    if (const int rc = check_encoder_net(entry, (int)precision, "precision in opts", dim_ff, n_layers)) return rc;
    const size_t blocks = (n + kSlots - 1) / kSlots;
    if (blocks > 0x7fffffffu) return fail(G2048_ERR_ARG, "%s: n too large for one launch", entry);
    const TpolicyCollectArgs args{static_cast<uint4 *>(boards_inout), score_inout, actions_out, prob_out, reward_out, flags_out,
                                  value_out_or_null, static_cast<uint4 *>(next_boards_out_or_null), state_maxcode_out_or_null,
                                  obs_out_or_null, mask4_out_or_null, step_counter_or_null, seed, step_index0, env_id_base, n, steps, opts};
    with_bool(precision == G2048_POLICY_BF16, [&](auto BF16) {
        hipLaunchKernelGGL(tpolicy_collect_kernel<decltype(BF16)::value>, dim3((unsigned)blocks), dim3(64 * kWaves), 0,
                           static_cast<hipStream_t>(stream), static_cast<const unsigned char *>(packed), dim_ff, n_layers, args);
    });
    return check_launch(entry);
}

}  // extern "C"
