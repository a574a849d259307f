// g2048_qnet.hip -- the hybrid agent's CNN-transformer Q-network (agents/hybrid.py:700-727, HybridDQN, in eval mode, one board
// per call) on the matrix cores of gfx950, one launch per forward pass (C-ABI: include/g2048.h, g2048_qnet_*, g2048_play_qnet_*).
//
//   pack_matrix_kernel       (g2048_mfma.h) one weight matrix [rows][K] into 1 KiB MFMA fragments (a lane's A operand is one
//                            16-byte load), its columns permuted so that conv2's and the embedding's K run in the order the
//                            forward produces them (conv2: inner 32, stride 4; the embedding: inner 64, stride 16).
//   qnet_pack_params_kernel  conv1 (tap-major), every bias, the LayerNorm weights and their eps into the blob's f32 section.
//   qnet_forward_kernel      Conv2d(1,32,k2,p1)+ReLU -> Conv2d(32,64,k2)+ReLU -> flatten -> Linear(1024,128) -> L x
//                            TransformerEncoderLayer(128, dim_ff, relu, post-norm) at sequence length 1 -> Linear(128,4), and the
//                            exploit action of DQNAgent.select_action (hybrid.py:943-953).
//   qnet_select_kernel       the whole of select_action (:909-953, use_beam_search = False) on given Q-values: epsilon coin,
//                            exploit argmax, exploration biased to RIGHT / DOWN (g2048_qnet_select_actions).
//   qnet_beam_kernel         select_action at use_beam_search = True on given Q-values (g2048_qnet_beam_actions): where the
//                            reference's beam_search plans (max tile >= threshold, at least 8 tiles) the exploit action is the
//                            decision of g2048_lookahead.h -- one ranking of the root's at most 24 children, which is all the
//                            reference's search does (its loop always leaves after the first level) -- and the argmax elsewhere.
//                            search_depth >= 2 consults no network; search_depth 1 reads the candidates' Q-values.
//   qnet_expand_kernel       the candidate boards of that ranking for search_depth 1, 32 slots a board (g2048_qnet_beam_expand).
//   qnet_play_kernel         complete games (evaluate_agent, :1176-1210) in one launch, 32 game slots a wavefront, with the
//                            game-slot core of g2048_play.h (g2048_play_qnet_games; with the planned decision between the exploit
//                            action and the epsilon coin, search_depth >= 2: g2048_play_qnet_beam_games).
//
// What is computed. The reference feeds the encoder x.unsqueeze(1) with batch_first=False, and only ever calls the network with
// one board, so every board is a sequence of ONE token: the softmax over one key is exactly 1.0 and the attention block is
// out_proj(W_v x + b_v); Q, K and the head count cannot influence the result and are skipped. A layer is
// x = norm1(x + out_proj(v(x))), x = norm2(x + linear2(relu(linear1(x)))). Board i's row is model(x[i:i+1]) in eval mode (the
// reference never calls .eval(), so its dropout is live; like the other two policies this is the eval-mode function).
//
// Layout of the computation. Boards are the MFMA N dimension. A wavefront owns kE = 2 column tiles = 32 boards and runs the whole
// network on them by itself, the activation held transposed in registers as 16-feature row tiles: register r of lane l (g = l >> 4,
// c = l & 15) of tile t = x[feature 16 t + 4 g + r][board c]. That register is at once the MFMA's result layout and, as it stands,
// the B operand of the next product (the packed weights carry the k order), so between conv1 and the Q-values nothing is
// exchanged between lanes except LayerNorm's two cross-lane sums. A block is four such wavefronts (128 boards) that share nothing
// but LDS space: no barrier after the boards are loaded.
//   conv1   stays on the VALU in f32 (K = 4, inputs powers of two): the wavefront's boards lie in LDS as zero-padded 6 x 6 grids of
//           tile values; per conv2 position a lane reads the 3 x 3 window that position's four taps see and computes the 32 conv1
//           outputs it owns (its 8 channels x 4 taps) from it.
//   conv2 + Linear(1024,128)  one position (y, x) at a time: conv2 is a 64 x 128 product per position (k = tap * 32 + channel), its
//           64 outputs after ReLU are the K slice (k = channel, feature channel * 16 + position) of the 1024 -> 128 product and are
//           consumed at once. The 1,024 features of a board never exist together.
//   pair()  y = b2 + W2 . act(W1 x + b1), 32 hidden features at a time, a slice made and consumed at once: the feed-forward pair
//           (act = ReLU, hidden = dim_ff) and the attention block (act = identity, W1 = the V rows of in_proj, W2 = out_proj,
//           hidden = 128) are the same code. dim_ff costs no registers beyond one slice.
// Precision. F32: f32 MFMA, exact f32 products and sums. BF16: the weights of conv2 and of every Linear and their inputs rounded
// to bf16 (nearest even), f32 accumulation; conv1, the biases, LayerNorm (biased variance) and the residual adds are f32 in both.
// Every output is one lane's fixed-order accumulation: no split-K, no atomics; a board's result does not depend on n, on its
// place in the batch or on the launch geometry. Weight traffic: every wavefront streams the blob once per 32 boards (5.05 MB f32 /
// 2.54 MB bf16 at dim_ff 2048, from L1 / L2). Measured (DESIGN.md has the arithmetic): f32 runs at 76 % of the MFMA peak and the
// traffic does not bind; bf16 is bound by it (23 % of its peak), and a launch of any size takes at least one wavefront's serial
// pass (0.89 ms f32, 0.35 ms bf16), so small batches are latency-bound. Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include <algorithm>
#include <cmath>

#include "../../include/g2048.h"
#include "g2048_board.h"
#include "g2048_host.h"
#include "g2048_lookahead.h"
#include "g2048_mfma.h"
#include "g2048_play.h"
#include "g2048_qnet_forward.h"
#include "g2048_rng.h"

namespace {

using namespace g2048;

// (the shapes, the layouts, the forward's pieces QNET_GRID_ / QNET_FORWARD_, exploit_action / select_action, the planned
// decision's LDS column and wave_sync: g2048_qnet_forward.h, which the experience collector's library expands as well)

// ------------------------------------------------------------------------------------------------------------- pack --
// (the matrices: pack_matrix_kernel, g2048_mfma.h)
__global__ __launch_bounds__(256) void qnet_pack_params_kernel(const float *__restrict__ plain, int ff, int layers, int count,
                                                                float *__restrict__ out)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= count) return;
    const Layout lay(false, ff, layers);
    int src = -1;
    if (i < 4 * kC1) src = kPlC1W + (i % kC1) * 4 + i / kC1;            // [tap][channel] from [channel][1][2][2]
    else if (i < 5 * kC1) src = kPlC1B + (i - 4 * kC1);
    else if (i < 5 * kC1 + kC2) src = kPlC2B + (i - 5 * kC1);
    else if (i < kPHead) src = kPlEmbB + (i - 5 * kC1 - kC2);
    else if (i < kPHead + layers * lay.layer_params()) {
        const int l = (i - kPHead) / lay.layer_params(), j = (i - kPHead) % lay.layer_params();
        const int base = kPlainLayer0 + l * pl_layer(ff);
        if (j < kD) src = base + kPlInB + 2 * kD + j;                    // the V third of in_proj_bias
        else if (j < 2 * kD) src = base + kPlOutB + (j - kD);
        else if (j < 2 * kD + ff) src = base + pl_b1(ff) + (j - 2 * kD);
        else if (j < 3 * kD + ff) src = base + pl_b2(ff) + (j - 2 * kD - ff);
        else if (j < 7 * kD + ff + 2) src = base + pl_norm(ff) + (j - 3 * kD - ff);
    } else {
        const int j = i - kPHead - layers * lay.layer_params(), base = kPlainLayer0 + layers * pl_layer(ff);
        if (j < 4) src = base + kPlFcB + j;
    }
    out[i] = src >= 0 ? plain[src] : 0.0f;
}

__global__ __launch_bounds__(256) void qnet_select_kernel(const float4 *__restrict__ q, const uint4 *__restrict__ boards,
                                                           uint8_t *__restrict__ actions, uint8_t *__restrict__ explored_out, float epsilon,
                                                           uint32_t k0, uint32_t k1, uint64_t id_base, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 qi = q[i];
    const uint4 bw = boards[i];
    const Board b{{bw.x, bw.y, bw.z, bw.w}};
    const uint32_t mask = valid_mask_env(b);
    bool explored;
    actions[i] = (uint8_t)select_action(exploit_action(qi.x, qi.y, qi.z, qi.w, mask), b, mask, epsilon, Keys{k0, k1}, id_base + i, explored);
    if (explored_out) explored_out[i] = explored ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------ beam_search --
// The whole of select_action at use_beam_search = True (hybrid.py:909-953) on given Q-values, one lane a board: the exploit
// action is beam_search's where it plans and the argmax elsewhere; the coin and the exploration are qnet_select_kernel's.
constexpr int kBeamBlock = 64;
__global__ __launch_bounds__(kBeamBlock) void qnet_beam_kernel(const float4 *__restrict__ q, const uint4 *__restrict__ boards,
                                                              const float *__restrict__ succ_q, uint8_t *__restrict__ actions,
                                                              uint8_t *__restrict__ planned_out, uint8_t *__restrict__ explored_out,
                                                              uint32_t width, uint32_t threshold, double gamma, float epsilon,
                                                              uint32_t k0, uint32_t k1, uint64_t id_base, size_t n)
{
    __shared__ LookaheadLds<kBeamBlock> lds;
    const size_t i = (size_t)blockIdx.x * kBeamBlock + threadIdx.x;
    if (i >= n) return;
    const float4 qi = q[i];
    const uint4 bw = boards[i];
    const Board b{{bw.x, bw.y, bw.z, bw.w}};
    const uint32_t mask = valid_mask_env(b);
    uint32_t a = exploit_action(qi.x, qi.y, qi.z, qi.w, mask);
    const bool planned = lookahead_planned(b, threshold);
    if (planned) {
        LookaheadColumn<kBeamBlock> column{lds, (int)threadIdx.x};
        a = lookahead_action(b, width, gamma, succ_q ? succ_q + i * (kLookaheadSlots * 4u) : nullptr, column);
    }
    bool explored;
    actions[i] = (uint8_t)select_action(a, b, mask, epsilon, Keys{k0, k1}, id_base + i, explored);
    if (planned_out) planned_out[i] = planned ? 1 : 0;
    if (explored_out) explored_out[i] = explored ? 1 : 0;
}

// The candidate boards of every board, one lane a slot (32 a board, slot 8 a + j): pick i of action a from draw 3 a + i of the
// board's id, mapped as simulate_sampled_successor maps it (for a = 0 these are g2048_simulate_move_sampled's successors).
__global__ __launch_bounds__(256) void qnet_expand_kernel(const uint4 *__restrict__ boards, uint4 *__restrict__ succ, uint8_t *__restrict__ count,
                                                           uint32_t k0, uint32_t k1, uint64_t id_base, size_t n)
{
    const size_t gidx = (size_t)blockIdx.x * 256u + threadIdx.x;
    const size_t i = gidx / kLookaheadSlots;
    if (i >= n) return;
    const uint32_t a = ((uint32_t)gidx >> 3) & 3u, j = (uint32_t)gidx & 7u;
    const uint4 bw = boards[i];
    const uint64_t id = id_base + i;
    uint32_t c;
    const Board o = lookahead_slot(Board{{bw.x, bw.y, bw.z, bw.w}}, a, j, rng_draw(k0, k1, id, 3u * a), rng_draw(k0, k1, id, 3u * a + 1u),
                                   rng_draw(k0, k1, id, 3u * a + 2u), c);
    succ[gidx] = make_uint4(o.w[0], o.w[1], o.w[2], o.w[3]);
    if (j == 0u) count[i * 4u + a] = (uint8_t)c;
}

// ---------------------------------------------------------------------------------------------------------- forward --
// Two blocks per compute unit (two wavefronts per SIMD, each covering the other's fragment loads): 236 (f32) / 230 (bf16) VGPRs,
// no scratch.
template <bool BF16>
__global__ __launch_bounds__(64 * kWaves, 2) void qnet_forward_kernel(const uint32_t *__restrict__ boards, const unsigned char *__restrict__ W,
                                                                    float4 *__restrict__ q_out, uint8_t *__restrict__ actions, size_t n,
                                                                    int ff, int layers)
{
    __shared__ float lds[kWaves][kGrid][kWaveBoards];
    const Layout lay(BF16, ff, layers);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const float *P = reinterpret_cast<const float *>(W + lay.params());
    const size_t env0 = (size_t)blockIdx.x * kBlockBoards + (size_t)wave * kWaveBoards;

    // the wavefront's boards as zero-padded grids of tile values; boards past n read as empty
    float (*grid)[kWaveBoards] = lds[wave];
    for (int i = lane; i < kGrid * kWaveBoards; i += 64) (&grid[0][0])[i] = 0.0f;
    __syncthreads();
    QNET_GRID_(env0 + 16 * e + col < n ? boards[(env0 + 16 * e + col) * 4 + g] : 0u)       // lane (g, c): row g of board c
    __syncthreads();

    QNET_FORWARD_(BF16)
    if (g != 0) return;
#pragma unroll
    for (int e = 0; e < kE; ++e) {
        const size_t env = env0 + 16 * e + col;
        if (env >= n) continue;
        q_out[env] = make_float4(q[e][0], q[e][1], q[e][2], q[e][3]);
        if (actions) {
            const uint4 bw = reinterpret_cast<const uint4 *>(boards)[env];
            actions[env] = (uint8_t)exploit_action(q[e][0], q[e][1], q[e][2], q[e][3], valid_mask_env(Board{{bw.x, bw.y, bw.z, bw.w}}));
        }
    }
}

// --------------------------------------------------------------------------------------------------- complete games --
// Complete games of the Q-network (the reference's evaluate_agent, hybrid.py:1176-1210: select_action -> env.step until done),
// as tpolicy_play_kernel (g2048_tpolicy.hip) plays the transformer policy's, with the game-slot core of g2048_play.h. The
// forward's unit is the wavefront: it runs the whole network alone on its 32 boards. So a wavefront owns 32 game slots, slot s =
// column s of its grids = lane s, and shares nothing with the other three of its block but the launch arguments and the
// direction table in LDS: after the prologue there is no block barrier, no wavefront waits on another, nothing spins. Per move
// the wavefront refills its idle slots (refill_slots: one atomicAdd per wavefront), rebuilds its 6 x 6 grids from the slots'
// boards in LDS (an idle slot holds the empty board), runs the shared forward, moves Q of the boards 16..31 from lanes 0..15 to
// lanes 16..31, and each slot lane picks its action (exploit_action / select_action with step index = the slot's own move t, id =
// the game's id) and makes the move (play_slot_move). The forward leaves no registers over, so a slot's state (PlaySlots, 80
// bytes a slot) is parked in LDS between moves and loaded after the forward, and the launch arguments are read from LDS too
// (PlayArgs). The wavefront leaves when all its slots are idle after a refill attempt, which means the queue is empty.
struct QPlayArgs {
    PlayArgs play;
    float epsilon;
    uint32_t n_waves;                                // wavefronts that play; the last block's surplus ones leave at once
};

// With BEAM the exploit action of a board the reference's beam_search plans is that search's decision (g2048_lookahead.h,
// search_depth >= 2: no network behind it) and the kernel takes two more arguments. They ride behind QPlayArgs in a struct of
// their own, and the scratch of the decisions is LDS only this instantiation has, so that without BEAM the kernel is
// instruction for instruction what it was before it had the parameter.
struct QBeamPlayArgs {
    QPlayArgs q;
    uint32_t width, threshold;
};
template <bool BEAM> using QArgs = std::conditional_t<BEAM, QBeamPlayArgs, QPlayArgs>;
__device__ inline const QPlayArgs &qplay(const QPlayArgs &a) { return a; }
__device__ inline const QPlayArgs &qplay(const QBeamPlayArgs &a) { return a.q; }

template <bool BF16, bool BEAM>
__global__ __launch_bounds__(64 * kWaves, 2) void qnet_play_kernel(const unsigned char *__restrict__ weights, int ff, int layers, const QArgs<BEAM> args)
{
    __shared__ QArgs<BEAM> all_args;
    __shared__ LookaheadLds<kWaveBoards> look[BEAM ? kWaves : 1];     // (not referenced without BEAM, and then not allocated)
    const QPlayArgs &par = qplay(all_args);
    __shared__ float lds[kWaves][kGrid][kWaveBoards];
    __shared__ PlaySlots<kWaveBoards> wave_slots[kWaves];
    __shared__ uint4 s_dir[G2048_DIR_TABLE_WORDS / 4];
    const Layout lay(BF16, ff, layers);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), g = lane >> 4, col = lane & 15;
    const bool slot_lane = lane < kWaveBoards;
    PlaySlots<kWaveBoards> &slots = wave_slots[wave];
    float (*grid)[kWaveBoards] = lds[wave];
    load_dir_table(s_dir, threadIdx.x);
    for (int i = lane; i < kGrid * kWaveBoards; i += 64) (&grid[0][0])[i] = 0.0f;
    if (slot_lane) slots.clear(lane);
    if (threadIdx.x == 0) all_args = args;
    __syncthreads();                                 // par and s_dir are there; the only block barrier
    if (blockIdx.x * (unsigned)kWaves + (unsigned)wave >= par.n_waves) return;
    bool drained = false;                            // wavefront-uniform: the queue has no game left

    for (;;) {
        const bool active = refill_slots(slots, par.play, lane, slot_lane, slot_lane && slots.active[lane] != 0u, drained);
        if (__ballot(active) == 0ull) break;         // every slot idle after a refill attempt = the queue is empty
        wave_sync();                                 // the slots' boards are there

        // The blob's address is made opaque once per move as well as once per conv position (QNET_FORWARD_), for the reason
        // tpolicy_play_kernel gives: otherwise every load of the forward that does not depend on the board is hoisted out of the
        // move loop and held in registers across it, which the forward has none to spare for.
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

        if (slot_lane && slots.active[lane] != 0u) {
            Game game = slots.load(lane);
            const uint32_t mask = valid_mask_env(game.board);
            uint32_t a = exploit_action(qs[0], qs[1], qs[2], qs[3], mask);
            if constexpr (BEAM) {
                if (lookahead_planned(game.board, all_args.threshold)) {
                    LookaheadColumn<kWaveBoards> column{look[wave], lane};
                    a = lookahead_action(game.board, all_args.width, 0.0, nullptr, column);
                }
            }
            const float epsilon = par.epsilon;
            if (epsilon > 0.0f) {                    // (epsilon 0 never explores: no draw)
                bool explored;
                a = select_action(a, game.board, mask, epsilon, rng_keys(par.play.seed, DOM_POLICY, (uint64_t)game.moves),
                                  par.play.id_base + game.index, explored);
            }
            play_slot_move(slots, lane, game, a, par.play, s_dir);
        }
        wave_sync();                                 // the next move's refill and grids see this move's slots
    }
}

// g2048_play_qnet_games (BEAM false: the three settings are not read) and g2048_play_qnet_beam_games; `stem` as in g2048_host.h
template <bool BEAM>
int play_qnet(const char *stem, void *boards_inout, uint32_t *score_inout, const void *packed, int dim_ff, int n_layers, int32_t *moves_out,
              int32_t *valid_out, int32_t *invalid_out, int32_t *milestone_move_out, double *reward_sum_out_or_null, uint8_t *alive_out,
              uint8_t *actions_out_or_null, int max_moves, float epsilon, int beam_width, int search_depth, int threshold, uint64_t seed,
              uint64_t game_id_base, size_t n_games, uint32_t opts, uint32_t max_waves, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n_games == 0) return G2048_OK;
    char entry[64];
    snprintf(entry, sizeof entry, "%s_games", stem);
    if (const int rc = check_play_args(stem, boards_inout, score_inout, packed, moves_out, valid_out, invalid_out, milestone_move_out,
                                       reward_sum_out_or_null, alive_out, max_moves, n_games, workspace, workspace_bytes))
        return rc;
    if (const int rc = check_encoder_net(entry, (int)opts, "opts (precision)", dim_ff, n_layers)) return rc;
    if (!good_epsilon(epsilon)) return fail(G2048_ERR_ARG, "%s: epsilon must lie in [0, 1]", entry);
    if (BEAM) {
        if (const int rc = check_beam_settings(entry, beam_width, search_depth, threshold)) return rc;
        if (search_depth == 1)
            return fail(G2048_ERR_ARG, "%s: search_depth 1 asks the network about every candidate and is not played in one launch; use "
                                       "the stepwise form (g2048_qnet_beam_expand, g2048_qnet_forward, g2048_qnet_beam_actions)", entry);
    }
    const bool bf16 = opts == G2048_POLICY_BF16;
    // auto: as many wavefronts as the chip holds at once (every later one would only find the queue empty)
    const size_t cap = max_waves ? (size_t)max_waves : (size_t)device_cus() * kWaves * with_bool(bf16, [](auto BF16) {
        return resident_per_cu(qnet_play_kernel<decltype(BF16)::value, BEAM>, 64 * kWaves);
    });
    if (cap == 0) return fail(G2048_ERR_HIP, "%s: no HIP device (occupancy query failed)", entry);
    const size_t waves = std::min(std::min((n_games + kWaveBoards - 1) / kWaveBoards, cap), (size_t)0x7fffffffu);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const int rc = reset_play_buffers(stem, workspace, actions_out_or_null, n_games, max_moves, s)) return rc;
    const QPlayArgs base{{static_cast<unsigned long long *>(workspace), static_cast<uint4 *>(boards_inout), score_inout, n_games, seed,
                          game_id_base, moves_out, valid_out, invalid_out, reinterpret_cast<int4 *>(milestone_move_out),
                          reward_sum_out_or_null, alive_out, actions_out_or_null, max_moves}, epsilon, (uint32_t)waves};
    QArgs<BEAM> args;
    if constexpr (BEAM) args = QBeamPlayArgs{base, (uint32_t)beam_width, (uint32_t)threshold};
    else args = base;
    with_bool(bf16, [&](auto BF16) {
        hipLaunchKernelGGL((qnet_play_kernel<decltype(BF16)::value, BEAM>), dim3(blocks_for(waves, kWaves)), dim3(64 * kWaves), 0, s,
                           static_cast<const unsigned char *>(packed), dim_ff, n_layers, args);
    });
    return check_launch(entry);
}

}  // namespace

extern "C" {

size_t g2048_qnet_packed_bytes(int precision, int dim_ff, int n_layers)
{
    if (!good_precision(precision) || !good_encoder_shape(dim_ff, n_layers)) return 0;
    return Layout(precision == G2048_POLICY_BF16, dim_ff, n_layers).bytes();
}

int g2048_qnet_pack(const float *plain_f32, int dim_ff, int n_layers, int precision, void *packed_out, void *stream)
{
    if (!plain_f32 || !packed_out) return fail(G2048_ERR_ARG, "g2048_qnet_pack: null pointer");
    if (!aligned(plain_f32, 4) || !aligned(packed_out, 16)) return fail(G2048_ERR_ARG, "g2048_qnet_pack: misaligned pointer");
    if (const int rc = check_encoder_net("g2048_qnet_pack", precision, "precision", dim_ff, n_layers)) return rc;
    const bool bf16 = precision == G2048_POLICY_BF16;
    const Layout lay(bf16, dim_ff, n_layers);
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto *out = static_cast<unsigned char *>(packed_out);
    // one launch per matrix: rows x K into the fragments from the index that `out` is offset by, columns permuted by (inner, stride)
    const auto pack = bf16 ? pack_matrix_kernel<true> : pack_matrix_kernel<false>;
    launch_pack_matrix(pack, lay.chunk, s, out, plain_f32 + kPlC2W, kC2, kK2, kC1, 4);
    launch_pack_matrix(pack, lay.chunk, s, out + lay.emb() * kFrag, plain_f32 + kPlEmbW, kD, kFlat, kC2, 16);
    for (int l = 0; l < n_layers; ++l) {
        const float *p = plain_f32 + kPlainLayer0 + (size_t)l * pl_layer(dim_ff);
        unsigned char *f = out + (lay.layer0() + (size_t)l * lay.layer_frags()) * kFrag;
        launch_pack_matrix(pack, lay.chunk, s, f, p + kPlInW + 2 * kD * kD, kD, kD, kD, 1);     // the V rows 256 .. 383 of in_proj_weight
        launch_pack_matrix(pack, lay.chunk, s, f + lay.out_proj() * kFrag, p + kPlOutW, kD, kD, kD, 1);
        launch_pack_matrix(pack, lay.chunk, s, f + lay.w1() * kFrag, p + kPlW1, dim_ff, kD, kD, 1);
        launch_pack_matrix(pack, lay.chunk, s, f + lay.w2() * kFrag, p + pl_w2(dim_ff), kD, dim_ff, dim_ff, 1);
    }
    const float *t = plain_f32 + kPlainLayer0 + (size_t)n_layers * pl_layer(dim_ff);
    launch_pack_matrix(pack, lay.chunk, s, out + lay.fc() * kFrag, t + kPlFcW, 4, kD, kD, 1);
    const int count = lay.n_params();
    hipLaunchKernelGGL(qnet_pack_params_kernel, dim3(blocks_for((size_t)count, 256)), dim3(256), 0, s, plain_f32, dim_ff, n_layers, count,
                       reinterpret_cast<float *>(out + lay.params()));
    return check_launch("g2048_qnet_pack");
}

int g2048_qnet_forward(const void *boards, const void *packed, float *q_out, uint8_t *actions_out_or_null, size_t n, int dim_ff,
                       int n_layers, uint32_t opts, void *stream)
{
    if (n == 0) return G2048_OK;
    if (!boards || !packed || !q_out) return fail(G2048_ERR_ARG, "g2048_qnet_forward: null pointer");
    if (!aligned(boards, 16) || !aligned(packed, 16) || !aligned(q_out, 16))
        return fail(G2048_ERR_ARG, "g2048_qnet_forward: misaligned pointer (boards, packed weights, q: 16 bytes)");
    if (const int rc = check_encoder_net("g2048_qnet_forward", (int)opts, "opts (precision)", dim_ff, n_layers)) return rc;
    const size_t blocks = (n + kBlockBoards - 1) / kBlockBoards;
    if (blocks > 0x7fffffffu) return fail(G2048_ERR_ARG, "g2048_qnet_forward: n too large for one launch");
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_bool(opts == G2048_POLICY_BF16, [&](auto BF16) {
        hipLaunchKernelGGL(qnet_forward_kernel<decltype(BF16)::value>, dim3((unsigned)blocks), dim3(64 * kWaves), 0, s,
                           static_cast<const uint32_t *>(boards), static_cast<const unsigned char *>(packed),
                           reinterpret_cast<float4 *>(q_out), actions_out_or_null, n, dim_ff, n_layers);
    });
    return check_launch("g2048_qnet_forward");
}

int g2048_qnet_select_actions(const float *q, const void *boards, uint8_t *actions_out, uint8_t *explored_out_or_null, float epsilon,
                              uint64_t seed, uint64_t step_index, uint64_t env_id_base, size_t n, void *stream)
{
    if (n == 0) return G2048_OK;
    if (!q || !boards || !actions_out) return fail(G2048_ERR_ARG, "g2048_qnet_select_actions: null pointer");
    if (!aligned(q, 16) || !aligned(boards, 16)) return fail(G2048_ERR_ARG, "g2048_qnet_select_actions: misaligned pointer (q, boards: 16 bytes)");
    if (!good_epsilon(epsilon)) return fail(G2048_ERR_ARG, "g2048_qnet_select_actions: epsilon must lie in [0, 1]");
    const size_t blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffu) return fail(G2048_ERR_ARG, "g2048_qnet_select_actions: n too large for one launch");
    const Keys k = rng_keys(seed, DOM_POLICY, step_index);
    hipLaunchKernelGGL(qnet_select_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4 *>(q), static_cast<const uint4 *>(boards), actions_out, explored_out_or_null, epsilon,
                       k.k0, k.k1, env_id_base, n);
    return check_launch("g2048_qnet_select_actions");
}

int g2048_qnet_beam_actions(const float *q, const void *boards, const float *succ_q_or_null, uint8_t *actions_out,
                            uint8_t *planned_out_or_null, uint8_t *explored_out_or_null, int beam_width, int search_depth, int threshold,
                            double gamma, float epsilon, uint64_t seed, uint64_t step_index, uint64_t env_id_base, size_t n, void *stream)
{
    if (n == 0) return G2048_OK;
    if (!q || !boards || !actions_out) return fail(G2048_ERR_ARG, "g2048_qnet_beam_actions: null pointer");
    if (!aligned(q, 16) || !aligned(boards, 16) || !aligned(succ_q_or_null, 16))
        return fail(G2048_ERR_ARG, "g2048_qnet_beam_actions: misaligned pointer (q, boards, succ_q: 16 bytes)");
    if (const int rc = check_beam_settings("g2048_qnet_beam_actions", beam_width, search_depth, threshold)) return rc;
    if (!std::isfinite(gamma)) return fail(G2048_ERR_ARG, "g2048_qnet_beam_actions: gamma must be finite");
    if (search_depth == 1 && !succ_q_or_null)
        return fail(G2048_ERR_ARG, "g2048_qnet_beam_actions: search_depth 1 needs succ_q (Q of the boards of g2048_qnet_beam_expand)");
    if (!good_epsilon(epsilon)) return fail(G2048_ERR_ARG, "g2048_qnet_beam_actions: epsilon must lie in [0, 1]");
    const size_t blocks = (n + kBeamBlock - 1) / kBeamBlock;
    if (blocks > 0x7fffffffu) return fail(G2048_ERR_ARG, "g2048_qnet_beam_actions: n too large for one launch");
    const Keys k = rng_keys(seed, DOM_POLICY, step_index);
    hipLaunchKernelGGL(qnet_beam_kernel, dim3((unsigned)blocks), dim3(kBeamBlock), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4 *>(q), static_cast<const uint4 *>(boards), search_depth == 1 ? succ_q_or_null : nullptr,
                       actions_out, planned_out_or_null, explored_out_or_null, (uint32_t)beam_width, (uint32_t)threshold, gamma, epsilon,
                       k.k0, k.k1, env_id_base, n);
    return check_launch("g2048_qnet_beam_actions");
}

int g2048_qnet_beam_expand(const void *boards, void *succ_boards_out, uint8_t *count_out, uint64_t seed, uint64_t step_index,
                           uint64_t state_id_base, size_t n, void *stream)
{
    if (n == 0) return G2048_OK;
    if (!boards || !succ_boards_out || !count_out) return fail(G2048_ERR_ARG, "g2048_qnet_beam_expand: null pointer");
    if (!aligned(boards, 16) || !aligned(succ_boards_out, 16) || !aligned(count_out, 4))
        return fail(G2048_ERR_ARG, "g2048_qnet_beam_expand: misaligned pointer (boards, successors: 16 bytes; counts: 4)");
    const size_t blocks = n / (256 / kLookaheadSlots) + 1;
    if (blocks > 0x7fffffffu) return fail(G2048_ERR_ARG, "g2048_qnet_beam_expand: n too large for one launch");
    const Keys k = rng_keys(seed, DOM_SIMULATE, step_index);
    hipLaunchKernelGGL(qnet_expand_kernel, dim3(blocks_for(n * kLookaheadSlots, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint4 *>(boards), static_cast<uint4 *>(succ_boards_out), count_out, k.k0, k.k1, state_id_base, n);
    return check_launch("g2048_qnet_beam_expand");
}

size_t g2048_play_qnet_workspace(size_t n_games) { return ticket_workspace_bytes(n_games); }
size_t g2048_play_qnet_beam_workspace(size_t n_games) { return ticket_workspace_bytes(n_games); }

int g2048_play_qnet_games(void *boards_inout, uint32_t *score_inout, const void *packed, int dim_ff, int n_layers, int32_t *moves_out,
                          int32_t *valid_out, int32_t *invalid_out, int32_t *milestone_move_out, double *reward_sum_out_or_null,
                          uint8_t *alive_out, uint8_t *actions_out_or_null, int max_moves, float epsilon, uint64_t seed,
                          uint64_t game_id_base, size_t n_games, uint32_t opts, uint32_t max_waves, void *workspace, size_t workspace_bytes,
                          void *stream)
{
    return play_qnet<false>("g2048_play_qnet", boards_inout, score_inout, packed, dim_ff, n_layers, moves_out, valid_out, invalid_out,
                            milestone_move_out, reward_sum_out_or_null, alive_out, actions_out_or_null, max_moves, epsilon, 0, 0, 0, seed,
                            game_id_base, n_games, opts, max_waves, workspace, workspace_bytes, stream);
}

int g2048_play_qnet_beam_games(void *boards_inout, uint32_t *score_inout, const void *packed, int dim_ff, int n_layers, int32_t *moves_out,
                               int32_t *valid_out, int32_t *invalid_out, int32_t *milestone_move_out, double *reward_sum_out_or_null,
                               uint8_t *alive_out, uint8_t *actions_out_or_null, int max_moves, float epsilon, int beam_width,
                               int search_depth, int threshold, uint64_t seed, uint64_t game_id_base, size_t n_games, uint32_t opts,
                               uint32_t max_waves, void *workspace, size_t workspace_bytes, void *stream)
{
    return play_qnet<true>("g2048_play_qnet_beam", boards_inout, score_inout, packed, dim_ff, n_layers, moves_out, valid_out, invalid_out,
                           milestone_move_out, reward_sum_out_or_null, alive_out, actions_out_or_null, max_moves, epsilon, beam_width,
                           search_depth, threshold, seed, game_id_base, n_games, opts, max_waves, workspace, workspace_bytes, stream);
}

}  // extern "C"
