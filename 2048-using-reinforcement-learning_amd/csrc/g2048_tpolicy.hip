// g2048_tpolicy.hip -- the reference's transformer policy (models/transformer.py:4-40, eval mode) on the matrix cores of
// gfx950, one launch per forward pass (C-ABI: include/g2048.h, g2048_tpolicy_*).
//
//   pack_matrix_kernel          (g2048_mfma.h) one weight matrix [rows][K] (plus, for the two heads, a second one stacked under
//                               it) into 1 KiB MFMA fragments: a lane's A operand is one 16-byte load.
//   tpolicy_pack_params_kernel  the embedding, every bias, the LayerNorm weights and their eps into the blob's f32 section.
//   tpolicy_forward_kernel      Linear(1,64) -> L x TransformerEncoderLayer(64, 4 heads, dim_ff, relu, post-norm) -> flatten ->
//                               Linear(1024,128)+ReLU -> Linear(128,64)+ReLU -> {Linear(64,4)+softmax | Linear(64,1)}.
//   tpolicy_play_kernel         complete games of that policy: the same forward for a block's 16 game slots, then sampling, the
//                               env step and the bookkeeping per slot with the game-slot core of g2048_play.h
//                               (g2048_play_tpolicy_games).
//
// Layout of the computation. A block of four wavefronts owns 16 boards, a wavefront four of them. In the encoder a board is one
// MFMA column tile: tokens are the N dimension, and the activation x is held transposed as 16-feature row tiles, register r of
// lane l (g = l >> 4, c = l & 15) = x[feature 16 t + 4 g + r][token c]. As in g2048_policy.hip that register is, as it stands,
// the B operand of the next projection (the packed weights carry the k permutation), so the encoder never leaves the VGPRs:
//   Q_h, K_h   = W . x          the usual product, result [d = 4 g + r][token c];
//   V_h^T      = x^T . Wv^T     the SAME registers as the A operand and the SAME weight fragment as the B operand (for the
//                               16x16 MFMAs lane l supplies A[c][g] and B[g][c], so a tile is its own transpose's operand);
//                               result [token 4 g + r][d = c];
//   S^T        = K^T . Q        A = the K_h registers, B = the Q_h registers (both sum over d = 4 g + r): [key 4 g + r][query c];
//   softmax    over the keys: 4 registers and two cross-lane steps (lanes xor 16, xor 32), in f32;
//   O_h        = V . P^T        A = the V_h^T registers, B = the P^T registers (both sum over key = 4 g + r): [d][query], which
//                               is row tile h of the concatenated heads, the B operand of out_proj.
// The three 16 x 16 x 16 attention products run on the f32 MFMA in BOTH precisions. The feed-forward pair is fused over
// 32-feature slices of relu(W1 x + b1): a slice is made and consumed at once, so dim_ff costs no registers. LayerNorm sums its
// 64 features over 16 registers and the same two cross-lane steps; statistics, softmax and residual adds are f32.
// fc1 sums over (token, feature) of one board, so there the boards become the N dimension: the four wavefronts write their
// encoder outputs to LDS as [board][token][feature], and each wavefront computes two of fc1's eight row tiles for all 16 boards
// (no split-K). fc2 (one row tile per wavefront) and the head tile (actor rows 0..3, critic row 4; wavefront 0) exchange their
// small activations through LDS the same way. Every output is one lane's fixed-order accumulation: it does not depend on n,
// on the board's place in the batch or on the launch geometry. Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <algorithm>

#include "../../include/g2048.h"
#include "g2048_board.h"
#include "g2048_host.h"
#include "g2048_mfma.h"
#include "g2048_play.h"
#include "g2048_rng.h"
#include "g2048_tpolicy_forward.h"
#include "g2048_tpolicy_layout.h"

namespace {

using namespace g2048;

// ------------------------------------------------------------------------------------------------ shapes and layouts --
// the shapes and the plain f32 layout: g2048_tpolicy_layout.h; the packed layout (Layout): g2048_tpolicy_forward.h

// ------------------------------------------------------------------------------------------------------------- pack --
// (the matrices: pack_matrix_kernel, g2048_mfma.h)
__global__ __launch_bounds__(256) void tpolicy_pack_params_kernel(const float *__restrict__ plain, int ff, int layers, int count,
                                                                   float *__restrict__ out)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= count) return;
    const Layout lay(false, ff, layers);
    int src = -1;
    if (i < 2 * kD) src = kPlainEmb + i;
    else if (i < 2 * kD + layers * lay.layer_params()) {
        const int l = (i - 2 * kD) / lay.layer_params(), j = (i - 2 * kD) % lay.layer_params();
        const int base = kPlainLayer0 + l * pl_layer(ff);
        if (j < 3 * kD) src = base + kPlInB + j;
        else if (j < 4 * kD) src = base + kPlOutB + (j - 3 * kD);
        else if (j < 4 * kD + ff) src = base + pl_b1(ff) + (j - 4 * kD);
        else if (j < 5 * kD + ff) src = base + pl_b2(ff) + (j - 4 * kD - ff);
        else if (j < 9 * kD + ff + 2) src = base + pl_norm(ff) + (j - 5 * kD - ff);
    } else {
        const int j = i - 2 * kD - layers * lay.layer_params(), base = kPlainLayer0 + layers * pl_layer(ff);
        if (j < kFc1) src = base + kPlFc1B + j;
        else if (j < kFc1 + kFc2) src = base + kPlFc2B + (j - kFc1);
        else if (j < kFc1 + kFc2 + 4) src = base + kPlActB + (j - kFc1 - kFc2);
        else if (j == kFc1 + kFc2 + 4) src = base + kPlCriB;
    }
    out[i] = src >= 0 ? plain[src] : 0.0f;
}

// ---------------------------------------------------------------------------------------------------------- forward --
// kWaves, kE, the LDS strides, project64 / add_norm / dense_lds and the forward's three macros TPOLICY_ENCODER_, TPOLICY_DENSE_ and
// TPOLICY_HEADS_: g2048_tpolicy_forward.h, which the experience collector (g2048_tpolicy_collect.hip) expands too

// Two blocks per compute unit (2 x 68.25 KiB of LDS, two wavefronts per SIMD): asking for that keeps the kernel under 256
// registers without scratch (f32 226, bf16 245 VGPRs) and is 8 % (f32) to 25 % (bf16) faster than one wavefront per SIMD with
// 298 (profiles/r08_tpolicy_rate.txt).
template <bool BF16>
__global__ __launch_bounds__(64 * kWaves, 2) void tpolicy_forward_kernel(const uint8_t *__restrict__ boards, const unsigned char *__restrict__ W,
                                                                       float4 *__restrict__ probs, float *__restrict__ value, size_t n,
                                                                       int ff, int layers)
{
    __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
    const Layout lay(BF16, ff, layers);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const float *P = reinterpret_cast<const float *>(W + lay.params());
    const size_t env0 = (size_t)blockIdx.x * 16;

    // boards past n read as empty
#define TPOLICY_GLOBAL_CELL_ (env0 + (size_t)(kE * wave + e) < n ? boards[(env0 + (size_t)(kE * wave + e)) * 16 + col] : (uint8_t)0)
    TPOLICY_ENCODER_(BF16, TPOLICY_GLOBAL_CELL_);
    TPOLICY_DENSE_(BF16);
    if (wave != 0) return;
    TPOLICY_HEADS_(BF16);
    const size_t env = env0 + col;
    if (env >= n) return;
    if (g == 0) probs[env] = softmax4(z);
    else if (g == 1 && value) value[env] = z[0];
}

// --------------------------------------------------------------------------------------------------- complete games --
// Complete games of the transformer policy, as policy_play_kernel (g2048_policy.hip) plays the PPO actor's, with the game-slot
// core of g2048_play.h. A block keeps the forward kernel's geometry: four wavefronts, 16 boards -- here 16 game slots, slot s on
// lane s of wavefront 0, its board one of the four of wavefront s / 4. Per move: every wavefront reads the cell bytes of its four
// slots' boards from LDS (an idle slot holds the empty board) and the block runs the shared forward; the head tile lands on lanes
// 0..15 of wavefront 0 with column = slot, so each slot lane has its own logits in registers, takes the softmax, picks its action
// (policy_action) and makes the move (play_slot_move). The forward leaves no registers over (226 / 245 VGPRs), so a slot's state
// (PlaySlots, 80 bytes a slot) is parked in LDS between moves and loaded after the forward, and the launch arguments are read
// from LDS too (PlayArgs). Idle slots are refilled once per move (refill_slots: one atomicAdd per block). Wavefront 0 publishes
// the mask of live slots through LDS under the move's first barrier: the block leaves when no slot is live, which after a refill
// attempt means the queue is empty. With kSkipIdleWave a wavefront whose four slots are all idle skips its encoder
// (wave-uniformly; it still reaches every barrier); that is switched off, not having been measured.
constexpr int kSlots = kWaves * kE;
constexpr bool kSkipIdleWave = false;                // built, and the games tested with it on; off until an A/B at the tail shows it faster

template <bool BF16>
__global__ __launch_bounds__(64 * kWaves, 2) void tpolicy_play_kernel(const unsigned char *__restrict__ weights, int ff, int layers, uint32_t mode,
                                                                    const PlayArgs args)
{
    __shared__ PlayArgs par;                         // (not enough on its own to stay out of scratch: see the opaque blob address)
    __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
    __shared__ PlaySlots<kSlots> slots;
    __shared__ uint4 s_dir[G2048_DIR_TABLE_WORDS / 4];
    __shared__ uint32_t s_live;                      // bit s: slot s plays this move (written by wavefront 0 before the barrier)
    const Layout lay(BF16, ff, layers);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), g = lane >> 4, col = lane & 15;
    const bool slot_lane = wave == 0 && lane < kSlots;
    load_dir_table(s_dir, threadIdx.x);
    if (slot_lane) slots.clear(lane);
    if (threadIdx.x == 0) par = args;
    __syncthreads();                                 // par and s_dir are there
    bool drained = false;                            // (wavefront 0) block-uniform: the queue has no game left

    for (;;) {
        if (wave == 0) {
            const bool active = refill_slots(slots, par, lane, slot_lane, slot_lane && slots.active[lane] != 0u, drained);
            const uint64_t live = __ballot(active);
            if (lane == 0) s_live = (uint32_t)live;
        }
        __syncthreads();                             // the slots' boards and s_live are there
        const uint32_t live = s_live;
        if (live == 0u) break;                       // block-uniform: every slot idle after a refill attempt = the queue is empty

        // The blob's address is made opaque once per move. Otherwise every load of the forward that does not depend on the
        // board (the embedding, the head biases) is hoisted out of the move loop and held in registers across it, which the
        // forward has none to spare for: without this line the kernel compiles to 48 (f32) / 64 (bf16) bytes of scratch per lane,
        // with it to none (profiles/r09_tpolicy_play_resource_usage.txt).
        const unsigned char *W = weights;
        asm volatile("" : "+s"(W));
        const float *P = reinterpret_cast<const float *>(W + lay.params());

        if (!kSkipIdleWave || ((live >> (kE * wave)) & ((1u << kE) - 1u)) != 0u) {
#define TPOLICY_SLOT_CELL_ reinterpret_cast<const uint8_t *>(slots.board)[(kE * wave + e) * 16 + col]
            TPOLICY_ENCODER_(BF16, TPOLICY_SLOT_CELL_);
        }
        // fc1 reads all 16 board columns of lds. A wavefront that skipped its encoder left its four columns as they were (on the
        // first move: never written, possibly NaN). That is sound only because an MFMA column depends on nothing but its own
        // column of B, through fc1, fc2 and the heads alike, and an idle slot's column is never read by a slot lane: anything
        // that mixes columns here (a reduction over boards, say) would have to write the idle columns first.
        TPOLICY_DENSE_(BF16);
        if (wave != 0) continue;                     // to the next move's barrier, where wavefront 0 joins after its slots' steps
        TPOLICY_HEADS_(BF16);

        if (slot_lane && slots.active[lane] != 0u) {
            Game game = slots.load(lane);
            const uint32_t a = policy_action(softmax4(z), valid_mask_env(game.board), mode, par.seed, game.moves,
                                             par.id_base + game.index);
            play_slot_move(slots, lane, game, a, par, s_dir);
        }
    }
}

}  // namespace

extern "C" {

size_t g2048_tpolicy_packed_bytes(int precision, int dim_ff, int n_layers)
{
    if (!good_precision(precision) || !good_encoder_shape(dim_ff, n_layers)) return 0;
    return Layout(precision == G2048_POLICY_BF16, dim_ff, n_layers).bytes();
}

int g2048_tpolicy_pack(const float *plain_f32, int dim_ff, int n_layers, int precision, void *packed_out, void *stream)
{
    if (!plain_f32 || !packed_out) return fail(G2048_ERR_ARG, "g2048_tpolicy_pack: null pointer");
    if (!aligned(plain_f32, 4) || !aligned(packed_out, 16)) return fail(G2048_ERR_ARG, "g2048_tpolicy_pack: misaligned pointer");
    if (const int rc = check_encoder_net("g2048_tpolicy_pack", precision, "precision", dim_ff, n_layers)) return rc;
    const bool bf16 = precision == G2048_POLICY_BF16;
    const Layout lay(bf16, dim_ff, n_layers);
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto *out = static_cast<unsigned char *>(packed_out);
    // one launch per matrix: rows x K into the fragments from the index that `out` is offset by
    const auto pack = bf16 ? pack_matrix_kernel<true> : pack_matrix_kernel<false>;
    for (int l = 0; l < n_layers; ++l) {
        const float *p = plain_f32 + kPlainLayer0 + (size_t)l * pl_layer(dim_ff);
        unsigned char *f = out + (size_t)l * lay.layer_frags() * kFrag;
        launch_pack_matrix(pack, lay.chunk, s, f, p + kPlInW, 3 * kD, kD, kD, 1);
        launch_pack_matrix(pack, lay.chunk, s, f + lay.out_proj() * kFrag, p + kPlOutW, kD, kD, kD, 1);
        launch_pack_matrix(pack, lay.chunk, s, f + lay.w1() * kFrag, p + kPlW1, dim_ff, kD, kD, 1);
        launch_pack_matrix(pack, lay.chunk, s, f + lay.w2() * kFrag, p + pl_w2(dim_ff), kD, dim_ff, dim_ff, 1);
    }
    const float *t = plain_f32 + kPlainLayer0 + (size_t)n_layers * pl_layer(dim_ff);
    launch_pack_matrix(pack, lay.chunk, s, out + lay.fc1() * kFrag, t + kPlFc1W, kFc1, kFlat, kFlat, 1);
    launch_pack_matrix(pack, lay.chunk, s, out + lay.fc2() * kFrag, t + kPlFc2W, kFc2, kFc1, kFc1, 1);
    launch_pack_matrix(pack, lay.chunk, s, out + lay.heads() * kFrag, t + kPlActW, 4, kD, kD, 1, t + kPlCriW, 1);      // actor over critic
    const int count = lay.n_params();
    hipLaunchKernelGGL(tpolicy_pack_params_kernel, dim3(blocks_for((size_t)count, 256)), dim3(256), 0, s, plain_f32, dim_ff, n_layers, count,
                       reinterpret_cast<float *>(out + lay.params()));
    return check_launch("g2048_tpolicy_pack");
}

int g2048_tpolicy_forward(const void *boards, const void *packed, float *probs_out, float *value_out_or_null, size_t n, int dim_ff,
                          int n_layers, uint32_t opts, void *stream)
{
    if (n == 0) return G2048_OK;
    if (!boards || !packed || !probs_out) return fail(G2048_ERR_ARG, "g2048_tpolicy_forward: null pointer");
    if (!aligned(boards, 16) || !aligned(packed, 16) || !aligned(probs_out, 16) || !aligned(value_out_or_null, 4))
        return fail(G2048_ERR_ARG, "g2048_tpolicy_forward: misaligned pointer (boards, packed weights, probs: 16 bytes; value: 4)");
    if (const int rc = check_encoder_net("g2048_tpolicy_forward", (int)opts, "opts (precision)", dim_ff, n_layers)) return rc;
    const size_t blocks = (n + 15) / 16;
    if (blocks > 0x7fffffffu) return fail(G2048_ERR_ARG, "g2048_tpolicy_forward: n too large for one launch");
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_bool(opts == G2048_POLICY_BF16, [&](auto BF16) {
        hipLaunchKernelGGL(tpolicy_forward_kernel<decltype(BF16)::value>, dim3((unsigned)blocks), dim3(64 * kWaves), 0, s,
                           static_cast<const uint8_t *>(boards), static_cast<const unsigned char *>(packed),
                           reinterpret_cast<float4 *>(probs_out), value_out_or_null, n, dim_ff, n_layers);
    });
    return check_launch("g2048_tpolicy_forward");
}

size_t g2048_play_tpolicy_workspace(size_t n_games) { return ticket_workspace_bytes(n_games); }

int g2048_play_tpolicy_games(void *boards_inout, uint32_t *score_inout, const void *packed, int dim_ff, int n_layers, int32_t *moves_out,
                             int32_t *valid_out, int32_t *invalid_out, int32_t *milestone_move_out, double *reward_sum_out_or_null,
                             uint8_t *alive_out, uint8_t *actions_out_or_null, int max_moves, uint64_t seed, uint64_t game_id_base,
                             size_t n_games, uint32_t opts, uint32_t max_blocks, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n_games == 0) return G2048_OK;
    if (const int rc = check_play_args("g2048_play_tpolicy", boards_inout, score_inout, packed, moves_out, valid_out, invalid_out,
                                       milestone_move_out, reward_sum_out_or_null, alive_out, max_moves, n_games, workspace, workspace_bytes))
        return rc;
    const uint32_t precision = opts & 0xfu, mode = (opts >> G2048_PLAY_POLICY_MODE_SHIFT) & 0xfu;
    if ((opts >> (G2048_PLAY_POLICY_MODE_SHIFT + 4)) != 0u || !good_precision((int)precision))
        return fail(G2048_ERR_ARG, "g2048_play_tpolicy_games: unknown opts (precision | mode << 4)");
    if (mode != G2048_PLAY_POLICY_MASKED && mode != G2048_PLAY_POLICY_UNMASKED && mode != G2048_PLAY_POLICY_GREEDY)
        return fail(G2048_ERR_ARG, "g2048_play_tpolicy_games: unknown mode");
    if (const int rc = check_encoder_net("g2048_play_tpolicy_games", (int)precision, "opts (precision | mode << 4)", dim_ff, n_layers)) return rc;
    const bool bf16 = precision == G2048_POLICY_BF16;
    // auto: as many blocks as the chip holds at once (every later one would only find the queue empty)
    const size_t cap = max_blocks ? (size_t)max_blocks : (size_t)device_cus() * with_bool(bf16, [](auto BF16) {
        return resident_per_cu(tpolicy_play_kernel<decltype(BF16)::value>, 64 * kWaves);
    });
    if (cap == 0) return fail(G2048_ERR_HIP, "g2048_play_tpolicy_games: no HIP device (occupancy query failed)");
    const size_t blocks = std::min(std::min((n_games + kSlots - 1) / kSlots, cap), (size_t)0x7fffffffu);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const int rc = reset_play_buffers("g2048_play_tpolicy", workspace, actions_out_or_null, n_games, max_moves, s)) return rc;
    const PlayArgs args{static_cast<unsigned long long *>(workspace), static_cast<uint4 *>(boards_inout), score_inout, n_games, seed,
                        game_id_base, moves_out, valid_out, invalid_out, reinterpret_cast<int4 *>(milestone_move_out), reward_sum_out_or_null,
                        alive_out, actions_out_or_null, max_moves};
    with_bool(bf16, [&](auto BF16) {
        hipLaunchKernelGGL(tpolicy_play_kernel<decltype(BF16)::value>, dim3((unsigned)blocks), dim3(64 * kWaves), 0, s,
                           static_cast<const unsigned char *>(packed), dim_ff, n_layers, mode, args);
    });
    return check_launch("g2048_play_tpolicy_games");
}

}  // extern "C"
