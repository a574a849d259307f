// g2048_qnet_batch_fwd.h -- the forward kernels of the hybrid agent's Q-network on a BATCH of boards (one sequence of n tokens), and below
// them the host side of its four batch passes (one call description, one check, one forward launch sequence: qb_forward<kDrop>), shared
// by g2048_qnet_batch.hip (the forward alone) and g2048_qnet_grad.hip (the forward that keeps its activations, then the gradient
// pass); g2048_ppo_grad.hip takes qb_linear_kernel from here for the PPO networks' fc2 and fc3, and g2048_qnet_train.hip (the training
// library) instantiates the attention, proj_norm and linear kernels a second time with a QDrop (g2048_qnet_drop.h) as their trailing
// argument: the reference's live dropout. The instantiations without one keep the parameter lists and the statements they had as
// plain kernels. Device and host code, included by those four files and nothing else; every kernel is per translation unit. What the phases are and
// why the weights are read from the plain buffer: the head of g2048_qnet_batch.hip. The outputs the gradient pass needs on top
// (conv1's output, the attention rows' maximum and sum, the sums before the LayerNorms) are optional pointers that the forward
// alone passes as null; they change no arithmetic.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/g2048.h"
#include "g2048_host.h"
#include "g2048_mfma.h"
#include "g2048_qnet_drop.h"

namespace {

using namespace g2048;

constexpr int kD = 128, kC1 = 32, kC2 = 64, kFlat = 1024, kHeads = 8, kHead = 16, kQkv = 3 * kD;

// plain f32 layout (include/g2048.h, g2048_qnet_pack), in floats
constexpr int kPlC1W = 0, kPlC1B = kPlC1W + kC1 * 4, kPlC2W = kPlC1B + kC1, kPlC2B = kPlC2W + kC2 * 4 * kC1, kPlEmbW = kPlC2B + kC2,
              kPlEmbB = kPlEmbW + kD * kFlat, kPlLayer0 = kPlEmbB + kD;
constexpr int kPlInW = 0, kPlInB = kPlInW + kQkv * kD, kPlOutW = kPlInB + kQkv, kPlOutB = kPlOutW + kD * kD, kPlW1 = kPlOutB + kD;
constexpr size_t pl_b1(size_t ff) { return kPlW1 + ff * kD; }
constexpr size_t pl_w2(size_t ff) { return pl_b1(ff) + ff; }
constexpr size_t pl_b2(size_t ff) { return pl_w2(ff) + kD * ff; }
constexpr size_t pl_norm(size_t ff) { return pl_b2(ff) + kD; }          // norm1.w norm1.b norm2.w norm2.b eps1 eps2
constexpr size_t pl_layer(size_t ff) { return pl_norm(ff) + 4 * kD + 2; }

// ------------------------------------------------------------------------------------------------------------- conv --
// One block a board. conv1 (32 x 5 x 5 from the zero-padded 6 x 6 grid of tile values) into LDS, then thread t computes conv2's
// channel t >> 2 at the four positions of row t & 3: 128 taps each, channel-major, fused multiply-adds into four partial sums a
// position (input channel & 3), in one fixed order. c1_out (optional, [board][32][25]): conv1's ReLU'd output, kept for the
// gradient pass.
__global__ __launch_bounds__(256) void qb_conv_kernel(const uint8_t *__restrict__ boards, const float *__restrict__ P, float *__restrict__ feat,
                                                      float *__restrict__ c1_out)
{
    __shared__ float pad[36];
    __shared__ float c1[kC1][25];
    const int t = threadIdx.x;
    const size_t board = blockIdx.x;
    if (t < 36) pad[t] = 0.0f;
    __syncthreads();
    if (t < 16) {
        const uint32_t code = boards[board * 16 + t];
        pad[6 * ((t >> 2) + 1) + (t & 3) + 1] = code ? __uint_as_float((127u + code) << 23) : 0.0f;
    }
    __syncthreads();
    for (int i = t; i < kC1 * 25; i += 256) {
        const int ch = i / 25, pos = i % 25, y = pos / 5, x = pos % 5;
        const float *w = P + kPlC1W + 4 * ch;
        float v = P[kPlC1B + ch];
        v = fmaf(w[0], pad[6 * y + x], v);
        v = fmaf(w[1], pad[6 * y + x + 1], v);
        v = fmaf(w[2], pad[6 * y + 6 + x], v);
        v = fmaf(w[3], pad[6 * y + 7 + x], v);
        c1[ch][pos] = fmaxf(v, 0.0f);
        if (c1_out) c1_out[board * (kC1 * 25) + i] = fmaxf(v, 0.0f);
    }
    __syncthreads();
    const int oc = t >> 2, py = t & 3;
    const float bias = P[kPlC2B + oc];
    float acc[4][4];                                 // [position][channel & 3]: four partial sums a position, combined pairwise
#pragma unroll
    for (int px = 0; px < 4; ++px)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[px][s] = s == 0 ? bias : 0.0f;
    const float *w2 = P + kPlC2W + (size_t)oc * (4 * kC1);
    for (int ic0 = 0; ic0 < kC1; ic0 += 4) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int ic = ic0 + s;
            const f4 w = load_w(w2 + 4 * ic);
            float a[5], b[5];
#pragma unroll
            for (int x = 0; x < 5; ++x) {
                a[x] = c1[ic][5 * py + x];
                b[x] = c1[ic][5 * py + 5 + x];
            }
#pragma unroll
            for (int px = 0; px < 4; ++px) {
                float v = acc[px][s];
                v = fmaf(w[0], a[px], v);
                v = fmaf(w[1], a[px + 1], v);
                v = fmaf(w[2], b[px], v);
                v = fmaf(w[3], b[px + 1], v);
                acc[px][s] = v;
            }
        }
    }
    float sum[4];
#pragma unroll
    for (int px = 0; px < 4; ++px) sum[px] = (acc[px][0] + acc[px][1]) + (acc[px][2] + acc[px][3]);
    *reinterpret_cast<f4 *>(feat + board * kFlat + oc * 16 + py * 4) = relu(f4{sum[0], sum[1], sum[2], sum[3]});
}

// ----------------------------------------------------------------------------------------------------------- linear --
// the whole K of one tile through chunks_product (g2048_mfma.h): groups of eight chunks, then pairs
__device__ inline f4 tile_product(const float *__restrict__ wrow, const float *__restrict__ xrow, bool live, int K, f4 bias)
{
    f4 acc[8] = {bias, splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f)};
    int k = 0;
    for (; k + 128 <= K; k += 128) chunks_product<8>(wrow + k, xrow + k, live, acc);
    for (; k < K; k += 32) chunks_product<2>(wrow + k, xrow + k, live, acc);
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}

// Y [n][M] = act(X [n][K] W^T + b): four wavefronts a block = four feature tiles of one board tile; grid (M / 64 up, board tiles).
// KEEP_NAN: the ReLU passes a NaN on, as torch.relu does (the PPO update, whose NaN loss is its caller's signal). With a QDrop
// (the Q-network's training forward, site 2: the ReLU'd hidden layer) Y is multiplied by the site's m, element board M + feature.
template <bool RELU, bool KEEP_NAN = false, class... MaybeDrop>
__global__ __launch_bounds__(256) void qb_linear_kernel(const float *__restrict__ X, int K, const float *__restrict__ W,
                                                         const float *__restrict__ bias, float *__restrict__ Y, int M, int n, MaybeDrop... drop)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const int o = (int)blockIdx.x * 4 + wave;
    if (16 * o >= M) return;
    const int board = (int)blockIdx.y * 16 + col;
    const bool live = board < n;
    f4 acc = load_w(bias + 16 * o + 4 * g);
    acc = tile_product(W + (size_t)(16 * o + col) * K + 4 * g, X + (size_t)board * K + 4 * g, live, K, acc);
    if (RELU) acc = KEEP_NAN ? relu_nan(acc) : relu(acc);
    if constexpr (sizeof...(MaybeDrop) != 0) {
        const uint32_t e = (uint32_t)board * (uint32_t)M + (uint32_t)(16 * o + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] *= qdrop_mult(drop..., e + r);
    }
    if (live) *reinterpret_cast<f4 *>(Y + (size_t)board * M + 16 * o + 4 * g) = acc;
}

// -------------------------------------------------------------------------------------------------------- attention --
// One wavefront a (query tile, head). Scores of a key tile: S[key][query] = K . Q over the head's 16 features (four MFMAs), so
// lane (query col, g) holds the scores of keys 4 g .. 4 g + 3 of the tile for its query: the maximum and the sum over a tile's
// keys are the toolkit's cross-lane reductions, and the probabilities are, as they stand, the B operand of P.V (A = V^T, lane
// (feature col, g) reading V[key 4 g + r][col]). The next tile's K and V are loaded before this tile's arithmetic. max_out, sum_out
// (optional, [query][head]): the row's final maximum and sum, from which the gradient pass recomputes the probabilities. With a
// QDrop (the training forward, site 0) the probabilities are multiplied by the site's m before P.V, element (head n + query) n + key;
// the row's maximum and sum are of the unmasked scores.
template <class... MaybeDrop>
__global__ __launch_bounds__(64) void qb_attention_kernel(const float *__restrict__ qkv, float *__restrict__ att, int n,
                                                          float *__restrict__ max_out, float *__restrict__ sum_out, MaybeDrop... drop)
{
    const int lane = threadIdx.x, g = lane >> 4, col = lane & 15, head = blockIdx.y;
    const int query = (int)blockIdx.x * 16 + col;
    const float *base = qkv + head * kHead;
    const f4 q = query < n ? load_f4(base + (size_t)query * kQkv + 4 * g) : splat(0.0f);
    const int tiles = (n + 15) / 16;
    const float ninf = -__builtin_inff();
    float m = ninf, l = 0.0f;
    f4 acc = splat(0.0f);

    f4 k_next = col < n ? load_f4(base + (size_t)col * kQkv + kD + 4 * g) : splat(0.0f);
    f4 v_next;
#pragma unroll
    for (int r = 0; r < 4; ++r) v_next[r] = 4 * g + r < n ? base[(size_t)(4 * g + r) * kQkv + 2 * kD + col] : 0.0f;

    for (int t = 0; t < tiles; ++t) {
        const f4 k = k_next, v = v_next;
        if (t + 1 < tiles) {
            const int key = 16 * (t + 1) + col;
            k_next = key < n ? load_f4(base + (size_t)key * kQkv + kD + 4 * g) : splat(0.0f);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kv = 16 * (t + 1) + 4 * g + r;
                v_next[r] = kv < n ? base[(size_t)kv * kQkv + 2 * kD + col] : 0.0f;
            }
        }
        f4 s = splat(0.0f);
#pragma unroll
        for (int r = 0; r < 4; ++r) s = __builtin_amdgcn_mfma_f32_16x16x4f32(k[r], q[r], s, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] = 16 * t + 4 * g + r < n ? s[r] * 0.25f : ninf;
        const float mn = fmaxf(m, lanes_max(fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]))));   // finite: key 0 of tile 0 is a board
        const float scale = expf(m - mn);
        f4 p;
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = expf(s[r] - mn);
        l = l * scale + lanes_sum((p[0] + p[1]) + (p[2] + p[3]));
        acc = acc * splat(scale);
        if constexpr (sizeof...(MaybeDrop) != 0) {
            const uint32_t e = ((uint32_t)head * (uint32_t)n + (uint32_t)query) * (uint32_t)n + (uint32_t)(16 * t + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) p[r] *= qdrop_mult(drop..., e + r);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v[r], p[r], acc, 0, 0, 0);
        m = mn;
    }
    if (query < n) *reinterpret_cast<f4 *>(att + (size_t)query * kD + head * kHead + 4 * g) = acc / splat(l);
    if (max_out && g == 0 && query < n) {
        max_out[(size_t)query * kHeads + head] = m;
        sum_out[(size_t)query * kHeads + head] = l;
    }
}

// -------------------------------------------------------------------------------------------------------- proj_norm --
// x = LayerNorm(x + H W^T + b) for one tile of 16 boards; norm: weight[128] bias[128]; eps: one float on the device. With fc
// (fc.weight [4][128], fc.bias [4]) Q = fc(x) goes to q_out. The residual rows are read from x, the normalised rows go to x_out
// (which may be x: a row is read and written by its own block only; null: not stored) and the sum before the norm to pre_out
// (optional; the gradient pass keeps it). With a QDrop (the training forward, sites 1 and 3: dropout1 / dropout2) H W^T + b is
// multiplied by the site's m before the residual add, element board 128 + feature.
constexpr int kTileStride = kD + 4;
__device__ inline float half_sum(float v)            // over the 32 lanes of the wavefront's half, the same on all of them
{
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) v += __shfl_xor(v, d);
    return v;
}

template <class... MaybeDrop>
__global__ __launch_bounds__(512) void qb_proj_norm_kernel(const float *__restrict__ H, int K, const float *__restrict__ W,
                                                           const float *__restrict__ bias, const float *__restrict__ norm,
                                                           const float *__restrict__ eps, const float *x, float *x_out, float *__restrict__ pre_out,
                                                           const float *__restrict__ fc, float4 *__restrict__ q_out, int n, MaybeDrop... drop)
{
    __shared__ __attribute__((aligned(16))) float tile[16][kTileStride];
    const int lane = threadIdx.x & 63, o = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    {
        const int board = (int)blockIdx.x * 16 + col;
        const bool live = board < n;
        f4 acc = load_w(bias + 16 * o + 4 * g);
        acc = tile_product(W + (size_t)(16 * o + col) * K + 4 * g, H + (size_t)board * K + 4 * g, live, K, acc);
        if constexpr (sizeof...(MaybeDrop) != 0) {
            const uint32_t e = (uint32_t)board * (uint32_t)kD + (uint32_t)(16 * o + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] *= qdrop_mult(drop..., e + r);
        }
        const f4 res = live ? load_f4(x + (size_t)board * kD + 16 * o + 4 * g) : splat(0.0f);
        *reinterpret_cast<f4 *>(&tile[col][16 * o + 4 * g]) = res + acc;
        if (pre_out && live) *reinterpret_cast<f4 *>(pre_out + (size_t)board * kD + 16 * o + 4 * g) = res + acc;
    }
    __syncthreads();
    const int row = 2 * o + (lane >> 5), j = lane & 31, board = (int)blockIdx.x * 16 + row;
    f4 v = *reinterpret_cast<const f4 *>(&tile[row][4 * j]);
    const float mean = half_sum((v[0] + v[1]) + (v[2] + v[3])) / (float)kD;
    v = v - splat(mean);
    const f4 d2 = v * v;
    const float rstd = 1.0f / sqrtf(half_sum((d2[0] + d2[1]) + (d2[2] + d2[3])) / (float)kD + eps[0]);
    v = v * splat(rstd) * load_w(norm + 4 * j) + load_w(norm + kD + 4 * j);
    if (x_out && board < n) *reinterpret_cast<f4 *>(x_out + (size_t)board * kD + 4 * j) = v;
    if (!fc) return;
    float out[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const f4 w = load_w(fc + a * kD + 4 * j);
        out[a] = half_sum(fmaf(w[3], v[3], fmaf(w[2], v[2], fmaf(w[1], v[1], w[0] * v[0]))));
    }
    if (j == 0 && board < n) q_out[board] = make_float4(out[0] + fc[4 * kD], out[1] + fc[4 * kD + 1], out[2] + fc[4 * kD + 2], out[3] + fc[4 * kD + 3]);
}

// ------------------------------------------------------------------------------------------------------------- host --
// One call of any of the Q-network's four batch passes (g2048_qnet_forward_batch, g2048_qnet_loss_grad and their _dropout forms).
// backward false: the forward alone; actions, targets, weights, grad, td and loss are then not looked at. p4, seed, call_index: the
// training-mode passes' (kDrop true), else unused.
struct QbCall {
    const void *boards;
    const float *plain;
    const int64_t *actions;
    const float *targets, *weights;
    size_t n;
    int dim_ff, n_layers;
    float *grad, *td, *loss, *q;
    void *workspace, *stream;
    bool backward;
    const double *p4;
    uint64_t seed, call_index;
};

// the argument checks of the four passes, all before any device call
template <bool kDrop>
int qb_check(const char *entry, const QbCall &c)
{
    if (!c.boards || !c.plain || !c.q || !c.workspace ||
        (c.backward && (!c.actions || !c.targets || !c.weights || !c.grad || !c.td || !c.loss)))
        return fail(G2048_ERR_ARG, "%s: null pointer", entry);
    if (!aligned(c.boards, 16) || !aligned(c.plain, 16) || !aligned(c.grad, 16) || !aligned(c.q, 16) || !aligned(c.workspace, 16) ||
        !aligned(c.actions, 8) || !aligned(c.targets, 4) || !aligned(c.weights, 4) || !aligned(c.td, 4) || !aligned(c.loss, 4))
        return c.backward ? fail(G2048_ERR_ARG, "%s: misaligned pointer (boards, plain weights, grad, q, workspace: 16 bytes; actions: 8; "
                                                "the rest: 4)", entry)
                          : fail(G2048_ERR_ARG, "%s: misaligned pointer (boards, plain weights, q, workspace: 16 bytes)", entry);
    if (c.n > G2048_QNET_BATCH_MAX)
        return fail(G2048_ERR_ARG, "%s: n must not exceed G2048_QNET_BATCH_MAX = %d (the boards are one sequence; a larger batch is not "
                                   "truncated)", entry, G2048_QNET_BATCH_MAX);
    if (!good_encoder_shape(c.dim_ff, c.n_layers))
        return fail(G2048_ERR_ARG, "%s: dim_ff must be a multiple of 32 (32 .. 65536) and n_layers 1 .. 64", entry);
    if constexpr (kDrop)
        if (const int rc = check_p(entry, c.p4)) return rc;
    return G2048_OK;
}

// the forward-only passes' workspace, in floats: x [np][128], qkv [np][384], att [np][128], h [np][max(1024, dim_ff)] (feat, then
// the hidden layer); every layer works in place
struct FwdWorkspace {
    size_t np, hw;
    FwdWorkspace(size_t n, int ff) : np((n + 15) / 16 * 16), hw((size_t)(ff > kFlat ? ff : kFlat)) {}
    size_t x() const { return 0; }
    size_t qkv() const { return np * kD; }
    size_t att() const { return qkv() + np * kQkv; }
    size_t h() const { return att() + np * kD; }
    size_t floats() const { return h() + np * hw; }
};

// one encoder layer's arrays: from x0 into x_next (null: not stored, as on the last layer of a forward-only pass); att and h are the
// DROPPED ones in a training pass. pre1, pre2, amax, asum: what the gradient pass keeps on top, null in a forward-only pass.
struct LayerBuffers {
    float *x0, *qkv, *att, *x1, *pre1, *h, *x_next, *pre2, *amax, *asum;
};

// layer l's five launches; fc_or_null: fc on the last layer, which then writes q_out
template <bool kDrop>
void qb_forward_layer(hipStream_t s, const float *L, int ff, const DropSites &st, const LayerBuffers &b, const float *fc_or_null, float *q_out,
                      int ni, unsigned tiles)
{
    const float *norms = L + pl_norm(ff), *none = nullptr;
    hipLaunchKernelGGL((qb_linear_kernel<false>), dim3((unsigned)(kQkv + 63) / 64, tiles), dim3(256), 0, s, static_cast<const float *>(b.x0), kD,
                       L + kPlInW, L + kPlInB, b.qkv, kQkv, ni);
    launch_site<kDrop>(st.at(0), [](auto... d) { return qb_attention_kernel<decltype(d)...>; }, dim3(tiles, kHeads), dim3(64), s,
                       static_cast<const float *>(b.qkv), b.att, ni, b.amax, b.asum);
    launch_site<kDrop>(st.at(1), [](auto... d) { return qb_proj_norm_kernel<decltype(d)...>; }, dim3(tiles), dim3(512), s,
                       static_cast<const float *>(b.att), kD, L + kPlOutW, L + kPlOutB, norms, norms + 4 * kD, static_cast<const float *>(b.x0),
                       b.x1, b.pre1, none, static_cast<float4 *>(nullptr), ni);
    launch_site<kDrop>(st.at(2), [](auto... d) { return qb_linear_kernel<true, false, decltype(d)...>; }, dim3((unsigned)(ff + 63) / 64, tiles),
                       dim3(256), s, static_cast<const float *>(b.x1), kD, L + kPlW1, L + pl_b1(ff), b.h, ff, ni);
    launch_site<kDrop>(st.at(3), [](auto... d) { return qb_proj_norm_kernel<decltype(d)...>; }, dim3(tiles), dim3(512), s,
                       static_cast<const float *>(b.h), ff, L + pl_w2(ff), L + pl_b2(ff), norms + 2 * kD, norms + 4 * kD + 1,
                       static_cast<const float *>(b.x1), b.x_next, b.pre2, fc_or_null, reinterpret_cast<float4 *>(q_out), ni);
}

// The forward of all four passes, 2 + 5 n_layers launches: conv into feat (and c1 where it is kept), the embedding into layer 0's
// x0, the layers, Q from the last. buffers(l, last): layer l's LayerBuffers. kDrop true: site s of a layer is live where p4[s] > 0
// and then launches the QDrop instantiation; with all four 0 the sequence and the bits are the eval-mode pass's.
template <bool kDrop, class Buffers>
void qb_forward(const QbCall &c, unsigned tiles, float *feat, float *c1, Buffers buffers)
{
    hipStream_t s = static_cast<hipStream_t>(c.stream);
    const float *P = c.plain;
    const int ni = (int)c.n, ff = c.dim_ff;
    hipLaunchKernelGGL(qb_conv_kernel, dim3((unsigned)c.n), dim3(256), 0, s, static_cast<const uint8_t *>(c.boards), P, feat, c1);
    hipLaunchKernelGGL((qb_linear_kernel<false>), dim3((unsigned)(kD + 63) / 64, tiles), dim3(256), 0, s, static_cast<const float *>(feat), kFlat,
                       P + kPlEmbW, P + kPlEmbB, buffers(0, c.n_layers == 1).x0, kD, ni);
    for (int l = 0; l < c.n_layers; ++l) {
        const bool last = l == c.n_layers - 1;
        qb_forward_layer<kDrop>(s, P + kPlLayer0 + (size_t)l * pl_layer(ff), ff,
                                DropSites(kDomQnetDropout, c.seed, c.call_index, l, kDrop ? c.p4 : nullptr), buffers(l, last),
                                last ? P + kPlLayer0 + (size_t)c.n_layers * pl_layer(ff) : nullptr, c.q, ni, tiles);
    }
}

// a forward-only pass: g2048_qnet_forward_batch (kDrop false) or g2048_qnet_forward_batch_dropout
template <bool kDrop>
int qb_forward_pass(const char *entry, const QbCall &c)
{
    if (c.n == 0) return G2048_OK;
    if (const int rc = qb_check<kDrop>(entry, c)) return rc;
    const FwdWorkspace ws(c.n, c.dim_ff);
    float *base = static_cast<float *>(c.workspace), *x = base + ws.x(), *qkv = base + ws.qkv(), *att = base + ws.att(), *h = base + ws.h();
    float *nowhere = nullptr;
    qb_forward<kDrop>(c, (unsigned)(ws.np / 16), h, nowhere, [&](int, bool last) {
        return LayerBuffers{x, qkv, att, x, nowhere, h, last ? nowhere : x, nowhere, nowhere, nowhere};
    });
    return check_launch(entry);
}

}  // namespace
