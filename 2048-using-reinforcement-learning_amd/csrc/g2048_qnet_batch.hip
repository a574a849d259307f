// g2048_qnet_batch.hip -- the hybrid agent's Q-network (agents/hybrid.py:700-727, HybridDQN, eval mode) on a BATCH of boards as the
// reference's train_step calls it (:1038-1046): the encoder layer is not batch_first and is fed x.unsqueeze(1), so the n boards
// are ONE sequence of n tokens that attend to each other (8 heads of 16, scores q.k / 4, softmax over all n keys). This is a
// different function from g2048_qnet_forward's (every board its own sequence of one token); they agree at n = 1. With it, the
// no-gradient block of train_step: the online network's argmax, the target network's Q at it and the Double-DQN target
// (g2048_dqn_targets). C-ABI: include/g2048.h, g2048_qnet_forward_batch / g2048_qnet_batch_workspace / g2048_dqn_targets.
//
// Shape of the work. n is small (the reference's batch is 256), so the pass is a short sequence of launches, one phase each,
// every phase's grid spread over board tiles x feature tiles (or query tiles x heads); between phases the activations lie
// row-major [board][feature] in the caller's workspace. 2 + 5 n_layers launches:
//   conv      conv1 + ReLU + conv2 + ReLU on the VALU, one block a board -> feat [n][1024] (feature = channel * 16 + position)
//   linear    Y = act(X W^T + b) on the f32 matrix cores, one wavefront a 16-board x 16-feature tile: the embedding (K 1024),
//             in_proj whole (Q, K, V: 384 outputs), linear1 + ReLU
//   attention one wavefront a (16-query tile, head): the key tiles streamed with an online softmax (running maximum subtracted,
//             keys past n masked out of the maximum and the sum, their V rows read as zero); scores and P.V on the matrix cores
//   proj_norm x = LayerNorm(x + H W^T + b), a block of eight wavefronts a 16-board tile, one wavefront a 16-feature tile of the
//             product, the 16 x 128 tile through LDS, then one wavefront two boards' statistics: out_proj + norm1 (K 128) and
//             linear2 + norm2 (K dim_ff); the last one computes fc on the normalised rows and writes Q instead of x
// Weights are read from the PLAIN f32 buffer (g2048_qnet_pack's input, state-dict order) as they lie: with boards as the MFMA N
// dimension a lane's A operand over 16 input features is the 16 bytes W[row][16 c + 4 g ..], one load from the row-major matrix.
// There is no second blob, and DeviceQNetwork.refresh() refreshes this path by refreshing `plain`. A layer's parameters start at
// an odd multiple of 8 bytes (two eps floats per layer), hence the 4-byte-aligned vector type of the weight loads.
// f32 only: the first layer's logits reach 1e9 on tile values up to 131,072 and its softmax is nearly one-hot; bf16 logits would
// pick keys at random. Every output element is one wavefront's fixed-order accumulation: no split-K, no atomics, so a call is
// bit-repeatable; rows past n are neither read nor written. No cooperative launch, no block waits on another: phase boundaries
// are launch boundaries. Compile with -ffp-contract=off (g2048_dqn_targets follows torch's operation order).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/g2048.h"
#include "g2048_host.h"
#include "g2048_mfma.h"

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

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));      // a weight row's 16 bytes: 4-byte aligned at worst
__device__ inline f4 load_w(const float *p) { const f4u v = *reinterpret_cast<const f4u *>(p); return f4{v[0], v[1], v[2], v[3]}; }

// workspace, in floats: x [np][128], qkv [np][384], att [np][128], h [np][max(1024, dim_ff)] (feat, then the hidden layer)
struct Workspace {
    size_t np, hw;
    Workspace(size_t n, int ff) : np((n + 15) / 16 * 16), hw((size_t)(ff > kFlat ? ff : kFlat)) {}
    size_t x() const { return 0; }
    size_t qkv() const { return np * kD; }
    size_t att() const { return qkv() + np * kQkv; }
    size_t h() const { return att() + np * kD; }
    size_t floats() const { return h() + np * hw; }
};

// ------------------------------------------------------------------------------------------------------------- conv --
// One block a board. conv1 (32 x 5 x 5 from the zero-padded 6 x 6 grid of tile values) into LDS, then thread t computes conv2's
// channel t >> 2 at the four positions of row t & 3: 128 taps each, channel-major, fused multiply-adds into four partial sums a
// position (input channel & 3), in one fixed order.
__global__ __launch_bounds__(256) void qb_conv_kernel(const uint8_t *__restrict__ boards, const float *__restrict__ P, float *__restrict__ feat)
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
// acc (features 16 o + 4 g + r of board `col` of the tile) += W[16 o ..][K] . X[board][K]; W row-major as it lies in `plain`.
// Lane (col, g): the A operand is W[16 o + col][16 c + 4 g ..], the B operand X[board][16 c + 4 g ..], four MFMAs a chunk.
// N chunks at once, every load issued before the first MFMA (K is a multiple of 32: the chunks come in pairs). Chunk c of a
// group of eight accumulates into acc[c]: eight independent partial sums, so that consecutive MFMAs do not wait on each other and
// the rounding error of a long K grows like a blocked sum's, not like one serial chain's. The order is fixed all the same.
template <int N>
__device__ inline void chunks_product(const float *__restrict__ wrow, const float *__restrict__ xrow, bool live, f4 (&acc)[8])
{
    f4 w[N], x[N];
#pragma unroll
    for (int c = 0; c < N; ++c) {
        w[c] = load_w(wrow + 16 * c);
        x[c] = live ? load_f4(xrow + 16 * c) : splat(0.0f);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[c][r], x[c][r], acc[c], 0, 0, 0);
}

__device__ inline f4 tile_product(const float *__restrict__ wrow, const float *__restrict__ xrow, bool live, int K, f4 bias)
{
    f4 acc[8] = {bias, splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f)};
    int k = 0;
    for (; k + 128 <= K; k += 128) chunks_product<8>(wrow + k, xrow + k, live, acc);
    for (; k < K; k += 32) chunks_product<2>(wrow + k, xrow + k, live, acc);
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
}

// Y [n][M] = act(X [n][K] W^T + b): four wavefronts a block = four feature tiles of one board tile; grid (M / 64 up, board tiles)
template <bool RELU>
__global__ __launch_bounds__(256) void qb_linear_kernel(const float *__restrict__ X, int K, const float *__restrict__ W,
                                                         const float *__restrict__ bias, float *__restrict__ Y, int M, int n)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const int o = (int)blockIdx.x * 4 + wave;
    if (16 * o >= M) return;
    const int board = (int)blockIdx.y * 16 + col;
    const bool live = board < n;
    f4 acc = load_w(bias + 16 * o + 4 * g);
    acc = tile_product(W + (size_t)(16 * o + col) * K + 4 * g, X + (size_t)board * K + 4 * g, live, K, acc);
    if (RELU) acc = relu(acc);
    if (live) *reinterpret_cast<f4 *>(Y + (size_t)board * M + 16 * o + 4 * g) = acc;
}

// -------------------------------------------------------------------------------------------------------- attention --
// One wavefront a (query tile, head). Scores of a key tile: S[key][query] = K . Q over the head's 16 features (four MFMAs), so
// lane (query col, g) holds the scores of keys 4 g .. 4 g + 3 of the tile for its query: the maximum and the sum over a tile's
// keys are the toolkit's cross-lane reductions, and the probabilities are, as they stand, the B operand of P.V (A = V^T, lane
// (feature col, g) reading V[key 4 g + r][col]). The next tile's K and V are loaded before this tile's arithmetic.
__global__ __launch_bounds__(64) void qb_attention_kernel(const float *__restrict__ qkv, float *__restrict__ att, int n)
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
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(v[r], p[r], acc, 0, 0, 0);
        m = mn;
    }
    if (query < n) *reinterpret_cast<f4 *>(att + (size_t)query * kD + head * kHead + 4 * g) = acc / splat(l);
}

// -------------------------------------------------------------------------------------------------------- proj_norm --
// x = LayerNorm(x + H W^T + b) for one tile of 16 boards; norm: weight[128] bias[128]; eps: one float on the device. With fc
// (fc.weight [4][128], fc.bias [4]) the normalised rows are not stored: Q = fc(x) is, to q_out.
constexpr int kTileStride = kD + 4;
__device__ inline float half_sum(float v)            // over the 32 lanes of the wavefront's half, the same on all of them
{
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(512) void qb_proj_norm_kernel(const float *__restrict__ H, int K, const float *__restrict__ W,
                                                           const float *__restrict__ bias, const float *__restrict__ norm,
                                                           const float *__restrict__ eps, float *x, const float *__restrict__ fc,
                                                           float4 *__restrict__ q_out, int n)
{
    __shared__ __attribute__((aligned(16))) float tile[16][kTileStride];
    const int lane = threadIdx.x & 63, o = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    {
        const int board = (int)blockIdx.x * 16 + col;
        const bool live = board < n;
        f4 acc = load_w(bias + 16 * o + 4 * g);
        acc = tile_product(W + (size_t)(16 * o + col) * K + 4 * g, H + (size_t)board * K + 4 * g, live, K, acc);
        const f4 res = live ? load_f4(x + (size_t)board * kD + 16 * o + 4 * g) : splat(0.0f);
        *reinterpret_cast<f4 *>(&tile[col][16 * o + 4 * g]) = res + acc;
    }
    __syncthreads();
    const int row = 2 * o + (lane >> 5), j = lane & 31, board = (int)blockIdx.x * 16 + row;
    f4 v = *reinterpret_cast<const f4 *>(&tile[row][4 * j]);
    const float mean = half_sum((v[0] + v[1]) + (v[2] + v[3])) / (float)kD;
    v = v - splat(mean);
    const f4 d2 = v * v;
    const float rstd = 1.0f / sqrtf(half_sum((d2[0] + d2[1]) + (d2[2] + d2[3])) / (float)kD + eps[0]);
    v = v * splat(rstd) * load_w(norm + 4 * j) + load_w(norm + kD + 4 * j);
    if (!fc) {
        if (board < n) *reinterpret_cast<f4 *>(x + (size_t)board * kD + 4 * j) = v;
        return;
    }
    float out[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const f4 w = load_w(fc + a * kD + 4 * j);
        out[a] = half_sum(fmaf(w[3], v[3], fmaf(w[2], v[2], fmaf(w[1], v[1], w[0] * v[0]))));
    }
    if (j == 0 && board < n) q_out[board] = make_float4(out[0] + fc[4 * kD], out[1] + fc[4 * kD + 1], out[2] + fc[4 * kD + 2], out[3] + fc[4 * kD + 3]);
}

// ------------------------------------------------------------------------------------------------------ dqn targets --
// hybrid.py:1042-1046 on given Q: next_action = argmax of the online Q (unmasked, first maximum), next_q = the target Q at it,
// target = shaped + (1 - done) * gamma * next_q in torch's order of operations, every step rounded to f32, no contraction.
__global__ __launch_bounds__(256) void dqn_targets_kernel(const float4 *__restrict__ q_online, const float4 *__restrict__ q_target,
                                                           const float *__restrict__ shaped, const float *__restrict__ dones, float gamma,
                                                           long long *__restrict__ next_actions, float *__restrict__ targets, int n)
{
#pragma clang fp contract(off)
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    const float4 qo = q_online[i], qt = q_target[i];
    const float o[4] = {qo.x, qo.y, qo.z, qo.w}, tq[4] = {qt.x, qt.y, qt.z, qt.w};
    int a = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (o[k] > o[a]) a = k;
    float t = (1.0f - dones[i]) * gamma;
    t = t * tq[a];
    next_actions[i] = a;
    targets[i] = shaped[i] + t;
}

}  // namespace

extern "C" {

size_t g2048_qnet_batch_workspace(size_t n, int dim_ff)
{
    if (n == 0 || n > G2048_QNET_BATCH_MAX || !good_encoder_shape(dim_ff, 1)) return 0;
    return Workspace(n, dim_ff).floats() * sizeof(float);
}

int g2048_qnet_forward_batch(const void *boards, const float *plain_f32, float *q_out, size_t n, int dim_ff, int n_layers,
                             void *workspace, void *stream)
{
    if (n == 0) return G2048_OK;
    if (!boards || !plain_f32 || !q_out || !workspace) return fail(G2048_ERR_ARG, "g2048_qnet_forward_batch: null pointer");
    if (!aligned(boards, 16) || !aligned(plain_f32, 16) || !aligned(q_out, 16) || !aligned(workspace, 16))
        return fail(G2048_ERR_ARG, "g2048_qnet_forward_batch: misaligned pointer (boards, plain weights, q, workspace: 16 bytes)");
    if (n > G2048_QNET_BATCH_MAX)
        return fail(G2048_ERR_ARG, "g2048_qnet_forward_batch: n must not exceed G2048_QNET_BATCH_MAX = %d (the boards are one sequence; "
                                   "a larger batch is not truncated)", G2048_QNET_BATCH_MAX);
    if (!good_encoder_shape(dim_ff, n_layers))
        return fail(G2048_ERR_ARG, "g2048_qnet_forward_batch: dim_ff must be a multiple of 32 (32 .. 65536) and n_layers 1 .. 64");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Workspace ws(n, dim_ff);
    float *base = static_cast<float *>(workspace), *x = base + ws.x(), *qkv = base + ws.qkv(), *att = base + ws.att(), *h = base + ws.h();
    const float *P = plain_f32;
    const int ni = (int)n, ff = dim_ff;
    const unsigned tiles = (unsigned)(ws.np / 16);
    const auto linear = [&](auto RELU, const float *X, int K, const float *W, const float *b, float *Y, int M) {
        hipLaunchKernelGGL(qb_linear_kernel<decltype(RELU)::value>, dim3((unsigned)(M + 63) / 64, tiles), dim3(256), 0, s, X, K, W, b, Y, M, ni);
    };
    hipLaunchKernelGGL(qb_conv_kernel, dim3((unsigned)n), dim3(256), 0, s, static_cast<const uint8_t *>(boards), P, h);
    linear(std::false_type{}, h, kFlat, P + kPlEmbW, P + kPlEmbB, x, kD);
    for (int l = 0; l < n_layers; ++l) {
        const float *L = P + kPlLayer0 + (size_t)l * pl_layer(ff), *norms = L + pl_norm(ff);
        const bool last = l == n_layers - 1;
        linear(std::false_type{}, x, kD, L + kPlInW, L + kPlInB, qkv, kQkv);
        hipLaunchKernelGGL(qb_attention_kernel, dim3(tiles, kHeads), dim3(64), 0, s, qkv, att, ni);
        hipLaunchKernelGGL(qb_proj_norm_kernel, dim3(tiles), dim3(512), 0, s, att, kD, L + kPlOutW, L + kPlOutB, norms, norms + 4 * kD, x,
                           static_cast<const float *>(nullptr), static_cast<float4 *>(nullptr), ni);
        linear(std::true_type{}, x, kD, L + kPlW1, L + pl_b1(ff), h, ff);
        hipLaunchKernelGGL(qb_proj_norm_kernel, dim3(tiles), dim3(512), 0, s, h, ff, L + pl_w2(ff), L + pl_b2(ff), norms + 2 * kD,
                           norms + 4 * kD + 1, x, last ? P + kPlLayer0 + (size_t)n_layers * pl_layer(ff) : static_cast<const float *>(nullptr),
                           reinterpret_cast<float4 *>(q_out), ni);
    }
    return check_launch("g2048_qnet_forward_batch");
}

int g2048_dqn_targets(const float *q_online_next, const float *q_target_next, const float *shaped, const float *dones, float gamma,
                      int64_t *next_actions_out, float *targets_out, size_t n, void *stream)
{
    if (n == 0) return G2048_OK;
    if (!q_online_next || !q_target_next || !shaped || !dones || !next_actions_out || !targets_out)
        return fail(G2048_ERR_ARG, "g2048_dqn_targets: null pointer");
    if (!aligned(q_online_next, 16) || !aligned(q_target_next, 16) || !aligned(shaped, 4) || !aligned(dones, 4) ||
        !aligned(next_actions_out, 8) || !aligned(targets_out, 4))
        return fail(G2048_ERR_ARG, "g2048_dqn_targets: misaligned pointer (the two Q: 16 bytes; actions: 8; the rest: 4)");
    if (!std::isfinite(gamma)) return fail(G2048_ERR_ARG, "g2048_dqn_targets: gamma must be finite");
    if (n > 0x7fffffffu) return fail(G2048_ERR_ARG, "g2048_dqn_targets: n too large for one launch");
    hipLaunchKernelGGL(dqn_targets_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4 *>(q_online_next), reinterpret_cast<const float4 *>(q_target_next), shaped, dones, gamma,
                       reinterpret_cast<long long *>(next_actions_out), targets_out, (int)n);
    return check_launch("g2048_dqn_targets");
}

}  // extern "C"
