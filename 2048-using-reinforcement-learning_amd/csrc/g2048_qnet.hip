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
#include "g2048_rng.h"

namespace {

using namespace g2048;

// ------------------------------------------------------------------------------------------------ shapes and layouts --
constexpr int kD = 128, kC1 = 32, kC2 = 64, kFlat = 1024, kK2 = 4 * kC1;      // widths; kK2: conv2's K per position

// plain f32 layout (g2048_qnet_pack's input; include/g2048.h): the module's state-dict order
constexpr int kPlC1W = 0, kPlC1B = kPlC1W + kC1 * 4, kPlC2W = kPlC1B + kC1, kPlC2B = kPlC2W + kC2 * kK2, kPlEmbW = kPlC2B + kC2,
              kPlEmbB = kPlEmbW + kD * kFlat, kPlainLayer0 = kPlEmbB + kD;
constexpr int kPlInW = 0, kPlInB = kPlInW + 3 * kD * kD, kPlOutW = kPlInB + 3 * kD, kPlOutB = kPlOutW + kD * kD, kPlW1 = kPlOutB + kD;
__host__ __device__ constexpr int pl_b1(int ff) { return kPlW1 + ff * kD; }
__host__ __device__ constexpr int pl_w2(int ff) { return pl_b1(ff) + ff; }
__host__ __device__ constexpr int pl_b2(int ff) { return pl_w2(ff) + kD * ff; }
__host__ __device__ constexpr int pl_norm(int ff) { return pl_b2(ff) + kD; }             // norm1.w norm1.b norm2.w norm2.b eps1 eps2
__host__ __device__ constexpr int pl_layer(int ff) { return pl_norm(ff) + 4 * kD + 2; }
constexpr int kPlFcW = 0, kPlFcB = kPlFcW + 4 * kD, kPlTail = kPlFcB + 4;

// packed layout: the fragments of conv2 (4 row tiles, K 128), the embedding (8, K 1024); per layer of the V rows of in_proj (8),
// out_proj (8), linear1 (dim_ff / 16), linear2 (8, K dim_ff); fc (1); then the f32 section. A matrix's fragments are ordered
// [row tile o][chunk c]; a chunk is 16 input features (f32) or 32 (bf16). f32 section: conv1 weights [tap][channel] 128, conv1
// bias 32, conv2 bias 64, embedding bias 128 | per layer: V bias 128, out_proj.bias 128, b1 dim_ff, b2 128, norm1.w norm1.b
// norm2.w norm2.b 512, eps1 eps2 0 0 | fc bias 16 (4, then zeros).
constexpr int kPHead = 4 * kC1 + kC1 + kC2 + kD;
struct Layout {
    int ff, layers, chunk;
    __host__ __device__ Layout(bool bf16, int dim_ff, int n_layers) : ff(dim_ff), layers(n_layers), chunk(bf16 ? 32 : 16) {}
    __host__ __device__ int chunks(int k) const { return k / chunk; }
    __host__ __device__ size_t emb() const { return (size_t)(kC2 / 16) * chunks(kK2); }
    __host__ __device__ size_t layer0() const { return emb() + (size_t)(kD / 16) * chunks(kFlat); }
    __host__ __device__ size_t out_proj() const { return (size_t)(kD / 16) * chunks(kD); }   // fragment indices within a layer
    __host__ __device__ size_t w1() const { return 2 * out_proj(); }
    __host__ __device__ size_t w2() const { return w1() + (size_t)(ff / 16) * chunks(kD); }
    __host__ __device__ size_t layer_frags() const { return w2() + (size_t)(kD / 16) * chunks(ff); }
    __host__ __device__ size_t fc() const { return layer0() + (size_t)layers * layer_frags(); }
    __host__ __device__ size_t params() const { return (fc() + chunks(kD)) * kFrag; }     // byte offset of the f32 section
    __host__ __device__ int layer_params() const { return 3 * kD + ff + 4 * kD + 4; }
    __host__ __device__ int n_params() const { return kPHead + layers * layer_params() + 16; }
    __host__ __device__ size_t bytes() const { return params() + (size_t)n_params() * 4; }
    __host__ __device__ size_t plain_floats() const { return (size_t)kPlainLayer0 + (size_t)layers * pl_layer(ff) + kPlTail; }
};

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

// ------------------------------------------------------------------------------------------------- forward's parts --
constexpr int kWaves = 4, kE = 2;                    // wavefronts per block, column tiles per wavefront: 32 boards a wavefront
constexpr int kWaveBoards = 16 * kE, kBlockBoards = kWaves * kWaveBoards;
constexpr int kGrid = 36;                            // a board's zero-padded 6 x 6 grid; LDS holds [wave][grid cell][board]

// acc[e] += (row tile o of the matrix at `mat`, K = 16 T) . x[e]  (x: the T feature tiles of each column tile)
template <bool BF16, int T>
__device__ inline void project(const unsigned char *mat, int o, int lane, const f4 (&x)[kE][T], f4 (&acc)[kE])
{
    constexpr int TPC = BF16 ? 2 : 1, C = T / TPC;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        f4 in[kE][2];
#pragma unroll
        for (int e = 0; e < kE; ++e) {
            in[e][0] = x[e][TPC * c];
            in[e][1] = x[e][TPC * c + TPC - 1];
        }
        chunk_mma<BF16, kE>(mat + ((size_t)(o * C + c) * 64 + lane) * 16, in, acc);
    }
}

// y[e][m] += (row tile m of the matrix at `mat`, c2 chunks a row tile) . (the 32-feature slice s of its K, tiles h[e][0..1])
template <bool BF16>
__device__ inline void consume32(const unsigned char *mat, int c2, int s, int lane, const f4 (&h)[kE][2], f4 (&y)[kE][8])
{
    constexpr int CPS = BF16 ? 1 : 2;                // chunks per 32-feature slice
#pragma unroll
    for (int t = 0; t < CPS; ++t) {
        const int c = CPS * s + t;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            f4 in[kE][2], acc[kE];
#pragma unroll
            for (int e = 0; e < kE; ++e) {
                in[e][0] = h[e][t];
                in[e][1] = h[e][1];
                acc[e] = y[e][m];
            }
            chunk_mma<BF16, kE>(mat + ((size_t)(m * c2 + c) * 64 + lane) * 16, in, acc);
#pragma unroll
            for (int e = 0; e < kE; ++e) y[e][m] = acc[e];
        }
    }
}

// y = b2 + W2 . act(W1 x + b1), the hidden layer 32 features at a time (act: ReLU or the identity)
template <bool BF16, bool RELU>
__device__ inline void pair(const unsigned char *W1, const float *b1, const unsigned char *W2, const float *b2, int hidden, int lane,
                            int g, const f4 (&x)[kE][8], f4 (&y)[kE][8])
{
    const int c2 = hidden / (BF16 ? 32 : 16);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const f4 b = load_f4(b2 + 16 * m + 4 * g);
#pragma unroll
        for (int e = 0; e < kE; ++e) y[e][m] = b;
    }
#pragma unroll 1
    for (int s = 0; s < hidden / 32; ++s) {
        f4 h[kE][2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            f4 acc[kE];
            const f4 b = load_f4(b1 + 32 * s + 16 * t + 4 * g);
#pragma unroll
            for (int e = 0; e < kE; ++e) acc[e] = b;
            project<BF16, 8>(W1, 2 * s + t, lane, x, acc);
#pragma unroll
            for (int e = 0; e < kE; ++e) h[e][t] = RELU ? relu(acc[e]) : acc[e];
        }
        consume32<BF16>(W2, c2, s, lane, h, y);
    }
}

// x = LayerNorm(x + y) over the 128 features of every board column; np = weight[128] bias[128], biased variance
__device__ inline void add_norm(f4 (&x)[kE][8], const f4 (&y)[kE][8], const float *np, float eps, int g)
{
#pragma unroll
    for (int e = 0; e < kE; ++e) {
        float s = 0.0f;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            x[e][t] = x[e][t] + y[e][t];
            s += (x[e][t][0] + x[e][t][1]) + (x[e][t][2] + x[e][t][3]);
        }
        const float mean = lanes_sum(s) / (float)kD;
        float q = 0.0f;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            x[e][t] = x[e][t] - splat(mean);
            const f4 d2 = x[e][t] * x[e][t];
            q += (d2[0] + d2[1]) + (d2[2] + d2[3]);
        }
        const float rstd = 1.0f / sqrtf(lanes_sum(q) / (float)kD + eps);
#pragma unroll
        for (int t = 0; t < 8; ++t) x[e][t] = x[e][t] * splat(rstd) * load_f4(np + 16 * t + 4 * g) + load_f4(np + kD + 16 * t + 4 * g);
    }
}

// ---------------------------------------------------------------------------------------------------- select_action --
// The exploit half of DQNAgent.select_action (hybrid.py:943-953): q[i] = -1e9 where invalid, then np.argmax (ties to the lowest
// index; no valid move: action 0). The forward kernel, the select kernel and the game kernel all decide with this function.
__device__ inline uint32_t exploit_action(float q0, float q1, float q2, float q3, uint32_t mask)
{
    const float q[4] = {q0, q1, q2, q3};
    float best = (mask & 1u) ? q[0] : -1e9f;
    uint32_t a = 0u;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const float v = ((mask >> k) & 1u) ? q[k] : -1e9f;
        if (v > best) { best = v; a = (uint32_t)k; }
    }
    return a;
}

// The whole of select_action at use_beam_search = False for one board: the coin u = (draw 1 >> 8) * 2^-24 < epsilon decides for
// exploration (hybrid.py:912), which samples among the valid moves with the preferences (1, 1, 3, 3) when the max tile is >= 64
// and np.argmax(board) is cell (3,3) -- cell 15's code is >= 6 and strictly above every other cell's -- and (1, 1, 1, 1)
// otherwise (:914-936, random.choices(valid_actions, weights)): sample_action with draw 0. The normalised preferences are exact
// in f32 and sample_action's + 1e-10f does not change them. A dead board samples among all four (:918-919).
__device__ inline uint32_t select_action(uint32_t exploit, const Board &b, uint32_t mask, float epsilon, Keys k, uint64_t id, bool &explored)
{
    const float u = (float)(rng_draw(k.k0, k.k1, id, 1u) >> 8) * 5.9604644775390625e-08f;
    explored = u < epsilon;
    if (!explored) return exploit;
    const uint32_t corner = b.w[3] >> 24;
    uint32_t rest = 0u;
#pragma unroll
    for (int c = 0; c < 15; ++c) {
        const uint32_t v = (b.w[c >> 2] >> (8 * (c & 3))) & 0xffu;
        rest = v > rest ? v : rest;
    }
    const bool biased = corner >= 6u && corner > rest;
    const float lo = biased ? 0.125f : 0.25f, hi = biased ? 0.375f : 0.25f;
    float pa;
    return sample_action(lo, lo, hi, hi, mask, rng_draw(k.k0, k.k1, id, 0u), pa);
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
// One decision's scratch (g2048_lookahead.h) as a column of LDS: lane s of S owns key[.][s] and rank[.][s], nobody else touches
// them, and every index the decision uses is uniform over the lanes that run it, so the accesses are free of bank conflicts.
template <int S>
struct LookaheadLds {
    double key[kLookaheadCandidates][S];
    uint32_t rank[kLookaheadCandidates][S];
};

template <int S>
struct LookaheadColumn {
    LookaheadLds<S> &lds;
    int s;
    __device__ double &key(uint32_t i) { return lds.key[i][s]; }
    __device__ uint32_t &rank(uint32_t i) { return lds.rank[i][s]; }
};

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
// The forward pass in two pieces that qnet_forward_kernel and the game-playing kernel (qnet_play_kernel, below) share. Both
// expand exactly this text, and a wavefront's pass depends on nothing but its own 32 boards and the blob, so the two kernels give
// bit-identical Q-values for the same board. Macros, not functions, for the reason TPOLICY_ENCODER_ of g2048_tpolicy.hip is one:
// expanded in place, the forward kernel's code stays what it was before the pieces were named. They use the kernel's names: W, P,
// lay, ff, layers, grid, lane, g, col.
//   QNET_GRID_     the wavefront's boards into its zero-padded grids of tile values (2 ** code, 0 for empty); ROW = row g of the
//                  board in column 16 e + col (the border cells are zeroed once and never written again);
//   QNET_FORWARD_  conv1 .. Linear(128,4): q[e] on lanes 0..15 (g = 0) = Q of the board in column 16 e + col.
#define QNET_GRID_(ROW) \
_Pragma("unroll") \
    for (int e = 0; e < kE; ++e) { \
        const uint32_t row = (ROW); \
_Pragma("unroll") \
        for (int k = 0; k < 4; ++k) { \
            const uint32_t code = (row >> (8 * k)) & 0xffu; \
            grid[6 * (g + 1) + k + 1][16 * e + col] = code ? __uint_as_float((127u + code) << 23) : 0.0f; \
        } \
    }

#define QNET_FORWARD_(BF16) \
/* conv1 -> conv2 -> Linear(1024,128), one conv2 position at a time */ \
    f4 x[kE][8]; \
_Pragma("unroll") \
    for (int m = 0; m < 8; ++m) { \
        const f4 b = load_f4(P + 5 * kC1 + kC2 + 16 * m + 4 * g); \
_Pragma("unroll") \
        for (int e = 0; e < kE; ++e) x[e][m] = b; \
    } \
    { \
        const int cemb = kFlat / (BF16 ? 32 : 16); \
_Pragma("unroll 1") \
        for (int p = 0; p < 16; ++p) { \
/* The blob's address is made opaque once per position: conv1's weights and conv2's fragments do not depend on the */ \
/* position, and hoisted out of this loop they would be held in registers the loop has none to spare for. */ \
            const unsigned char *Wc2 = W; \
            asm volatile("" : "+s"(Wc2)); \
            const unsigned char *Wemb = Wc2 + lay.emb() * kFrag; \
            const float *c1w = reinterpret_cast<const float *>(Wc2 + lay.params()), *c1b = c1w + 4 * kC1, *c2b = c1w + 5 * kC1; \
            const int py = p >> 2, px = p & 3; \
            float win[kE][3][3];  /* the padded grid's cells (py .. py + 2, px .. px + 2) */ \
_Pragma("unroll") \
            for (int e = 0; e < kE; ++e) \
_Pragma("unroll") \
                for (int i = 0; i < 3; ++i) \
_Pragma("unroll") \
                    for (int j = 0; j < 3; ++j) win[e][i][j] = grid[6 * (py + i) + px + j][16 * e + col]; \
            f4 c2[kE][4]; \
_Pragma("unroll") \
            for (int o = 0; o < 4; ++o) { \
                const f4 b = load_f4(c2b + 16 * o + 4 * g); \
_Pragma("unroll") \
                for (int e = 0; e < kE; ++e) c2[e][o] = b; \
            } \
_Pragma("unroll") \
            for (int tap = 0; tap < 4; ++tap) {  /* conv2's tap (dy, dx): conv1's output at (py + dy, px + dx), 32 channels */ \
                const int dy = tap >> 1, dx = tap & 1; \
                f4 c1[kE][2]; \
_Pragma("unroll") \
                for (int h = 0; h < 2; ++h) {  /* channels 16 h + 4 g + r */ \
                    const int ch = 16 * h + 4 * g; \
                    const f4 w0 = load_f4(c1w + ch), w1 = load_f4(c1w + kC1 + ch), w2 = load_f4(c1w + 2 * kC1 + ch), \
                             w3 = load_f4(c1w + 3 * kC1 + ch), b = load_f4(c1b + ch); \
_Pragma("unroll") \
                    for (int e = 0; e < kE; ++e) \
                        c1[e][h] = relu((((b + w0 * splat(win[e][dy][dx])) + w1 * splat(win[e][dy][dx + 1])) + \
                                         w2 * splat(win[e][dy + 1][dx])) + w3 * splat(win[e][dy + 1][dx + 1])); \
                } \
/* k = tap * 32 + channel: the 32-feature slice `tap` of conv2's K */ \
_Pragma("unroll") \
                for (int t = 0; t < (BF16 ? 1 : 2); ++t) { \
                    const int c = (BF16 ? 1 : 2) * tap + t; \
_Pragma("unroll") \
                    for (int o = 0; o < 4; ++o) { \
                        f4 in[kE][2], acc[kE]; \
_Pragma("unroll") \
                        for (int e = 0; e < kE; ++e) { \
                            in[e][0] = c1[e][t]; \
                            in[e][1] = c1[e][1]; \
                            acc[e] = c2[e][o]; \
                        } \
                        chunk_mma<BF16, kE>(Wc2 + ((size_t)(o * (kK2 / (BF16 ? 32 : 16)) + c) * 64 + lane) * 16, in, acc); \
_Pragma("unroll") \
                        for (int e = 0; e < kE; ++e) c2[e][o] = acc[e]; \
                    } \
                } \
            } \
/* the embedding's K slice k = p * 64 + channel (plain feature channel * 16 + p), two 32-feature slices */ \
_Pragma("unroll") \
            for (int s = 0; s < 2; ++s) { \
                f4 h[kE][2]; \
_Pragma("unroll") \
                for (int e = 0; e < kE; ++e) { \
                    h[e][0] = relu(c2[e][2 * s]); \
                    h[e][1] = relu(c2[e][2 * s + 1]); \
                } \
                consume32<BF16>(Wemb, cemb, 2 * p + s, lane, h, x); \
            } \
        } \
    } \
 \
/* the encoder layers at sequence length 1 */ \
_Pragma("unroll 1") \
    for (int l = 0; l < layers; ++l) { \
        const unsigned char *Wl = W + (lay.layer0() + (size_t)l * lay.layer_frags()) * kFrag; \
        const float *Pl = P + kPHead + l * lay.layer_params(); \
        const float *bv = Pl, *bo = Pl + kD, *b1 = Pl + 2 * kD, *b2 = b1 + ff, *norms = b2 + kD; \
        f4 y[kE][8]; \
        pair<BF16, false>(Wl, bv, Wl + lay.out_proj() * kFrag, bo, kD, lane, g, x, y); \
        add_norm(x, y, norms, norms[4 * kD], g); \
        pair<BF16, true>(Wl + lay.w1() * kFrag, b1, Wl + lay.w2() * kFrag, b2, ff, lane, g, x, y); \
        add_norm(x, y, norms + 2 * kD, norms[4 * kD + 1], g); \
    } \
 \
/* Linear(128,4): rows 0..3 of one row tile, on lanes 0..15 (g = 0); the exploit action from the board's own valid moves */ \
    const float *Pt = P + kPHead + layers * lay.layer_params(); \
    f4 q[kE]; \
    { \
        const f4 b = load_f4(Pt + 4 * g); \
_Pragma("unroll") \
        for (int e = 0; e < kE; ++e) q[e] = b; \
    } \
    project<BF16, 8>(W + lay.fc() * kFrag, 0, lane, x, q);

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

// LDS accesses of one wavefront complete in program order; this only keeps the compiler from moving them across the point
// where lanes read what other lanes of the wavefront wrote.
__device__ inline void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

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

bool good_epsilon(float e) { return e >= 0.0f && e <= 1.0f; }      // false for NaN

// the settings of the reference's beam_search: G2048_OK, or the error as `entry`'s
int check_beam_settings(const char *entry, int beam_width, int search_depth, int threshold)
{
    if (beam_width < 1 || beam_width > 64) return fail(G2048_ERR_ARG, "%s: beam_width must lie in 1 .. 64", entry);
    if (search_depth < 1) return fail(G2048_ERR_ARG, "%s: search_depth must be at least 1", entry);
    if (threshold < 1) return fail(G2048_ERR_ARG, "%s: threshold (a tile value) must be at least 1", entry);
    return G2048_OK;
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
