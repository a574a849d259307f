// g2048_policy.hip -- the PPO actor / critic forward pass of the reference (agents/ppo_agent.py:61-136, eval mode) on the
// matrix cores of gfx950 (C-ABI: include/g2048.h, g2048_policy_*).
//
//   policy_pack_kernel     rearranges a network's plain f32 weights (torch's row-major [out][in], BatchNorm already folded
//                          in) into the packed blob the forward kernel streams: every lane's MFMA A operand is one 16-byte
//                          load, and a wavefront reads one contiguous KiB per fragment.
//   policy_forward_kernel  16 -> 256 -> 128 -> 64 -> {4 | 1} for 16 * E boards per wavefront, reading the packed uint8 boards
//                          directly (x = code / 15, PPOAgent.normalize_state). Bias initialises the accumulator, ReLU is
//                          applied on the way out of it, the 4-way softmax runs in f32 in registers. blockIdx.y picks the
//                          network (0 actor, 1 critic), so one launch serves both.
//   policy_play_kernel     complete games of the actor (play.py / train.py): the same forward, then sampling, the env step and
//                          the bookkeeping per game slot, slots refilled from a ticket counter (g2048_play_policy_games).
//
// Layout of the computation. Every layer is computed transposed, Y^T = W . X^T: the MFMA's A operand is a 16-row tile of
// weights, its B operand 16 boards' activations, and the result tile holds output features in its rows (register r of lane l:
// feature 4 * (l >> 4) + r) and boards in its columns (l & 15). That is already the lane -> k map of the next layer's B
// operand, up to a permutation of k, so activations never leave the VGPRs: the packed weights carry the same permutation.
//   f32  (mfma_f32_16x16x4f32, exact f32):  a chunk is 16 input features = 4 MFMAs; MFMA r of input tile t reads, on lane l,
//        feature 16 t + 4 (l >> 4) + r: register r of the previous layer's tile t, as it stands.
//   bf16 (mfma_f32_16x16x32_bf16):          a chunk is 32 input features = 1 MFMA; element j of lane l is feature
//        32 s + 16 (j >> 2) + 4 (l >> 4) + (j & 3): registers 0..3 of tiles 2s and 2s + 1, rounded to bf16 (RNE).
// Layer 1 (K = 16) and layer 2 are fused: each 32-feature slice of h1 is made and consumed at once, so only layer 2's
// accumulators stay live across the loop. No split-K, no atomics: each output is one lane's own accumulation in a fixed order.
// Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <algorithm>

#include "../../include/g2048.h"
#include "g2048_board.h"
#include "g2048_host.h"
#include "g2048_mfma.h"
#include "g2048_play.h"
#include "g2048_policy_forward.h"
#include "g2048_rng.h"

namespace {

using namespace g2048;

// ------------------------------------------------------------------------------------------------ shapes and layouts --
// plain f32 layout (g2048_policy_pack's input): W1 b1 W2 b2 W3 b3 W4 b4, each weight [out][in]
constexpr int kPlainW1 = 0, kPlainB1 = kPlainW1 + kH1 * kIn, kPlainW2 = kPlainB1 + kH1, kPlainB2 = kPlainW2 + kH2 * kH1,
              kPlainW3 = kPlainB2 + kH2, kPlainB3 = kPlainW3 + kH3 * kH2, kPlainW4 = kPlainB3 + kH3;

// ------------------------------------------------------------------------------------------------------------- pack --
// One thread per packed 32-bit word (f32: one weight; bf16: two). Padding (layer 1's missing features in bf16, layer 4's
// rows past n_out) is written as zero, so the blob is fully defined.
template <bool BF16>
__global__ __launch_bounds__(256) void policy_pack_kernel(const float *__restrict__ plain, int n_out, uint32_t *__restrict__ packed)
{
    using P = Packed<BF16>;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t byte = w * 4;
    if (byte >= P::kBytes) return;
    if (byte >= P::kBias) {
        const int i = (int)((byte - P::kBias) / 4);
        float v;
        if (i < kH1) v = plain[kPlainB1 + i];
        else if (i < kH1 + kH2) v = plain[kPlainB2 + i - kH1];
        else if (i < kH1 + kH2 + kH3) v = plain[kPlainB3 + i - kH1 - kH2];
        else {
            const int o = i - kH1 - kH2 - kH3;
            v = o < n_out ? plain[kPlainW4 + n_out * kH3 + o] : 0.0f;
        }
        packed[w] = __float_as_uint(v);
        return;
    }
    int K, N, wofs, rows;
    size_t base;
    if (byte >= P::kL4) { base = P::kL4; K = kH3; N = kOutPad; wofs = kPlainW4; rows = n_out; }
    else if (byte >= P::kL3) { base = P::kL3; K = kH2; N = kH3; wofs = kPlainW3; rows = kH3; }
    else if (byte >= P::kL2) { base = P::kL2; K = kH1; N = kH2; wofs = kPlainW2; rows = kH2; }
    else { base = P::kL1; K = kIn; N = kH1; wofs = kPlainW1; rows = kH1; }
    const size_t rel = byte - base;
    const int frag = (int)(rel / P::kFrag), lane = (int)(rel % P::kFrag) / 16, word = (int)(rel % 16) / 4;
    const int c = frag / (N / 16), o = frag % (N / 16);
    const int row = 16 * o + (lane & 15), h = lane >> 4;
    auto weight = [&](int k) { return (row < rows && k < K) ? plain[wofs + row * K + k] : 0.0f; };
    packed[w] = fragment_word<BF16>(c, h, word, weight);
}

// ---------------------------------------------------------------------------------------------------------- forward --
// The layers (POLICY_LAYERS_, dense, board_operand), the blob's layout (Packed<>) and the tile counts are g2048_policy_forward.h's:
// g2048_ppo_collect.hip expands the same text.
constexpr int kWaves = 4;

template <bool BF16, int E>
__global__ __launch_bounds__(64 * kWaves) void policy_forward_kernel(
    const uint32_t *__restrict__ boards, const unsigned char *__restrict__ actor, const unsigned char *__restrict__ critic,
    float4 *__restrict__ probs, float *__restrict__ value, size_t n)
{
    using P = Packed<BF16>;
    const int lane = threadIdx.x & 63, h = lane >> 4, col = lane & 15;
    const bool is_critic = blockIdx.y != 0;
    const unsigned char *W = is_critic ? critic : actor;
    const float *bias = reinterpret_cast<const float *>(W + P::kBias);
    const size_t env0 = ((size_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * (16 * E);
    if (env0 >= n) return;                       // whole wavefront past the end (wave-uniform)

    // layer-1 B operand: features 4h .. 4h+3 of board env0 + 16e + col (one 32-bit load; rows past n read as empty)
    f4 x[E][2];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const size_t env = env0 + 16 * e + col;
        board_operand(env < n ? boards[env * 4 + h] : 0u, x[e]);
    }

    POLICY_LAYERS_(BF16, E, W, bias, lane, h, x, out);

    // rows 0..3 of the output tile sit in lanes 0..15 (h == 0), one board per lane
    if (h != 0) return;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const size_t env = env0 + 16 * e + col;
        if (env >= n) continue;
        const f4 z = out[e][0];
        if (is_critic) value[env] = z[0];
        else probs[env] = softmax4(z);
    }
}

// --------------------------------------------------------------------------------------------------- complete games --
// The reference's policy games (play.py:44-68, train.py:54-90) played to the end on the device, as g2048_play_games plays
// the beam agent's, with the game-slot core of g2048_play.h. One wavefront is one block and owns S = 16 E game slots, slot s
// on lane s. Per move, for all of its live slots at once: the slot lanes write their boards to LDS, every lane reads the
// dword its layer-1 B operand needs, the wavefront runs the shared forward, lanes 0..15 write the probabilities to LDS, and
// each slot lane reads its own row, picks its action (policy_action) and makes the move (play_move). The slot's Game stays
// in registers: this kernel has them to spare. Slots sit at different move indices, so the RNG keys are derived per lane
// (rng_keys: the seed half is loop-invariant and hoisted). A finished game's slot takes the next game index from the ticket
// counter (claim_games). A wavefront leaves when its slots are idle and the queue is empty.
template <bool BF16, int E>
__global__ __launch_bounds__(64) void policy_play_kernel(const unsigned char *__restrict__ W, uint32_t mode, const PlayArgs par)
{
    constexpr int S = 16 * E;
    __shared__ uint4 s_board[S];
    __shared__ float4 s_prob[S];
    __shared__ uint4 s_dir[G2048_DIR_TABLE_WORDS / 4];
    const int lane = threadIdx.x, h = lane >> 4, col = lane & 15;
    const bool slot_lane = lane < S;
    using P = Packed<BF16>;
    const float *bias = reinterpret_cast<const float *>(W + P::kBias);
    load_dir_table(s_dir, threadIdx.x);

    Game game{};
    bool active = false, drained = false;        // drained: wave-uniform, the queue has no game left
    for (;;) {
        if (!drained && claim_games(par, lane, slot_lane && !active, game.index, drained)) {
            game = start_game(par, game.index);
            active = true;
        }
        if (__ballot(active) == 0ull) break;

        // slot lanes -> LDS (idle slots: the empty board) -> each lane's B-operand dword of every tile
        const Board &cur = game.board;
        if (slot_lane) s_board[lane] = active ? make_uint4(cur.w[0], cur.w[1], cur.w[2], cur.w[3]) : make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        f4 x[E][2];
#pragma unroll
        for (int e = 0; e < E; ++e) board_operand(reinterpret_cast<const uint32_t *>(s_board)[(16 * e + col) * 4 + h], x[e]);
        POLICY_LAYERS_(BF16, E, W, bias, lane, h, x, out);
        if (h == 0) {
#pragma unroll
            for (int e = 0; e < E; ++e) s_prob[16 * e + col] = softmax4(out[e][0]);
        }
        __syncthreads();

        if (slot_lane && active) {
            const uint32_t a = policy_action(s_prob[lane], valid_mask_env(cur), mode, par.seed, game.moves, par.id_base + game.index);
            active = !play_move(game, a, par, s_dir);
        }
    }
}

}  // namespace

extern "C" {

size_t g2048_policy_packed_bytes(int precision, int n_out)
{
    if (n_out != 1 && n_out != 4) return 0;
    if (precision == G2048_POLICY_F32) return Packed<false>::kBytes;
    if (precision == G2048_POLICY_BF16) return Packed<true>::kBytes;
    return 0;
}

int g2048_policy_pack(const float *plain_f32, int n_out, int precision, void *packed_out, void *stream)
{
    if (!plain_f32 || !packed_out) return fail(G2048_ERR_ARG, "g2048_policy_pack: null pointer");
    if (!aligned(plain_f32, 4) || !aligned(packed_out, 16)) return fail(G2048_ERR_ARG, "g2048_policy_pack: misaligned pointer");
    if (n_out != 1 && n_out != 4) return fail(G2048_ERR_ARG, "g2048_policy_pack: n_out must be 4 (actor) or 1 (critic)");
    if (!good_precision(precision)) return fail(G2048_ERR_ARG, "g2048_policy_pack: unknown precision");
    const size_t bytes = g2048_policy_packed_bytes(precision, n_out);
    const dim3 grid((unsigned)((bytes / 4 + 255) / 256));
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_bool(precision == G2048_POLICY_BF16, [&](auto BF16) {
        hipLaunchKernelGGL(policy_pack_kernel<decltype(BF16)::value>, grid, dim3(256), 0, s, plain_f32, n_out, static_cast<uint32_t *>(packed_out));
    });
    return check_launch("g2048_policy_pack");
}

int g2048_policy_forward(const void *boards, const void *actor_packed, const void *critic_packed_or_null, float *probs_out,
                         float *value_out_or_null, size_t n, uint32_t opts, void *stream)
{
    if (n == 0) return G2048_OK;
    if (!boards || !actor_packed || !probs_out) return fail(G2048_ERR_ARG, "g2048_policy_forward: null pointer");
    if (!critic_packed_or_null != !value_out_or_null)
        return fail(G2048_ERR_ARG, "g2048_policy_forward: critic_packed and value_out must both be given or both be NULL");
    if (!aligned(boards, 16) || !aligned(actor_packed, 16) || !aligned(critic_packed_or_null, 16) || !aligned(probs_out, 16) ||
        !aligned(value_out_or_null, 4))
        return fail(G2048_ERR_ARG, "g2048_policy_forward: misaligned pointer (boards, packed weights, probs: 16 bytes; value: 4)");
    if (!good_precision((int)opts)) return fail(G2048_ERR_ARG, "g2048_policy_forward: unknown opts (precision)");
    const bool bf16 = opts == G2048_POLICY_BF16;
    const size_t per_block = (size_t)kWaves * 16 * (bf16 ? kTilesBF16 : kTilesF32);
    const size_t blocks = (n + per_block - 1) / per_block;
    if (blocks > 0x7fffffffu) return fail(G2048_ERR_ARG, "g2048_policy_forward: n too large for one launch");
    const dim3 grid((unsigned)blocks, critic_packed_or_null ? 2u : 1u);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const auto *b = static_cast<const uint32_t *>(boards);
    const auto *a = static_cast<const unsigned char *>(actor_packed);
    const auto *c = static_cast<const unsigned char *>(critic_packed_or_null);
    with_precision(bf16, [&](auto BF16, auto E) {
        hipLaunchKernelGGL((policy_forward_kernel<decltype(BF16)::value, decltype(E)::value>), grid, dim3(64 * kWaves), 0, s, b, a, c,
                           reinterpret_cast<float4 *>(probs_out), value_out_or_null, n);
    });
    return check_launch("g2048_policy_forward");
}

size_t g2048_play_policy_workspace(size_t n_games) { return ticket_workspace_bytes(n_games); }

int g2048_play_policy_games(void *boards_inout, uint32_t *score_inout, const void *actor_packed, int32_t *moves_out,
                            int32_t *valid_out, int32_t *invalid_out, int32_t *milestone_move_out, double *reward_sum_out_or_null,
                            uint8_t *alive_out, uint8_t *actions_out_or_null, int max_moves, uint64_t seed, uint64_t game_id_base,
                            size_t n_games, uint32_t opts, uint32_t max_waves, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n_games == 0) return G2048_OK;
    if (const int rc = check_play_args("g2048_play_policy", boards_inout, score_inout, actor_packed, moves_out, valid_out, invalid_out,
                                       milestone_move_out, reward_sum_out_or_null, alive_out, max_moves, n_games, workspace, workspace_bytes))
        return rc;
    const uint32_t precision = opts & 0xfu, mode = (opts >> G2048_PLAY_POLICY_MODE_SHIFT) & 0xfu;
    if ((opts >> (G2048_PLAY_POLICY_MODE_SHIFT + 4)) != 0u || !good_precision((int)precision))
        return fail(G2048_ERR_ARG, "g2048_play_policy_games: unknown opts (precision | mode << 4)");
    if (mode != G2048_PLAY_POLICY_MASKED && mode != G2048_PLAY_POLICY_UNMASKED && mode != G2048_PLAY_POLICY_GREEDY)
        return fail(G2048_ERR_ARG, "g2048_play_policy_games: unknown mode");
    const bool bf16 = precision == G2048_POLICY_BF16;
    const size_t slots = 16 * (size_t)(bf16 ? kTilesBF16 : kTilesF32);
    // auto: as many wavefronts as the chip holds at once (every later one would only find the queue empty)
    const size_t cap = max_waves ? (size_t)max_waves : (size_t)device_cus() * with_precision(bf16, [](auto BF16, auto E) {
        return resident_per_cu(policy_play_kernel<decltype(BF16)::value, decltype(E)::value>, 64);
    });
    if (cap == 0) return fail(G2048_ERR_HIP, "g2048_play_policy_games: no HIP device (occupancy query failed)");
    const size_t waves = std::min(std::min((n_games + slots - 1) / slots, cap), (size_t)0x7fffffffu);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const PlayArgs args{static_cast<unsigned long long *>(workspace), static_cast<uint4 *>(boards_inout), score_inout, n_games, seed,
                        game_id_base, moves_out, valid_out, invalid_out, reinterpret_cast<int4 *>(milestone_move_out), reward_sum_out_or_null,
                        alive_out, actions_out_or_null, max_moves};
    if (const int rc = reset_play_buffers("g2048_play_policy", workspace, actions_out_or_null, n_games, max_moves, s)) return rc;
    with_precision(bf16, [&](auto BF16, auto E) {
        hipLaunchKernelGGL((policy_play_kernel<decltype(BF16)::value, decltype(E)::value>), dim3((unsigned)waves), dim3(64), 0, s,
                           static_cast<const unsigned char *>(actor_packed), mode, args);
    });
    return check_launch("g2048_play_policy_games");
}

}  // extern "C"
