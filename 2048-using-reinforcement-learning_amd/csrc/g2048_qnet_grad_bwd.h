// g2048_qnet_grad_bwd.h -- the backward kernels of the hybrid agent's Q-network, the workspace they share with the forward that
// keeps its activations, and the one launch sequence of the loss and gradient pass (qg_pass<kDrop>; its forward is qb_forward of
// g2048_qnet_batch_fwd.h): shared by g2048_qnet_grad.hip (g2048_qnet_loss_grad, eval mode) and g2048_qnet_train.hip (the same pass with
// the reference's live dropout, libg2048_train_hip.so). Device code, included by those two files and nothing else; every kernel is
// per translation unit. What the phases are and the rules they keep: the head of g2048_qnet_grad.hip. The two attention kernels
// take a QDrop (g2048_qnet_drop.h) as a trailing argument in the training pass: each hashes the tile it recomputes; the instantiation
// without one is the eval-mode kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "g2048_grad_products.h"
#include "g2048_host.h"
#include "g2048_mfma.h"
#include "g2048_qnet_batch_fwd.h"
#include "g2048_qnet_drop.h"

namespace {

constexpr int kC1Out = kC1 * 25;                     // conv1's output a board: 32 channels of 5 x 5

// workspace, in floats, every array [np] rows (np = n rounded up to a tile of 16; rows past n are never touched)
struct GradWorkspace {
    size_t np, ff, hw, layers;
    GradWorkspace(size_t n, int dim_ff, int n_layers)
        : np((n + 15) / 16 * 16), ff((size_t)dim_ff), hw((size_t)(dim_ff > kFlat ? dim_ff : kFlat)), layers((size_t)n_layers) {}
    // kept by the forward
    size_t feat() const { return 0; }
    size_t c1() const { return feat() + np * kFlat; }
    size_t x(size_t l) const { return c1() + np * kC1Out + l * np * kD; }             // l = 0 .. layers: layer l's input
    size_t layer(size_t l) const { return x(layers + 1) + l * np * (kQkv + 4 * kD + 2 * kHeads + ff); }
    size_t qkv(size_t l) const { return layer(l); }
    size_t att(size_t l) const { return qkv(l) + np * kQkv; }
    size_t pre1(size_t l) const { return att(l) + np * kD; }
    size_t x1(size_t l) const { return pre1(l) + np * kD; }
    size_t pre2(size_t l) const { return x1(l) + np * kD; }
    size_t amax(size_t l) const { return pre2(l) + np * kD; }
    size_t asum(size_t l) const { return amax(l) + np * kHeads; }
    size_t h(size_t l) const { return asum(l) + np * kHeads; }
    // the backward's own
    size_t ga() const { return layer(layers); }
    size_t gb() const { return ga() + np * kD; }
    size_t ds() const { return gb() + np * kD; }
    size_t datt() const { return ds() + np * kD; }
    size_t dqkv() const { return datt() + np * kD; }
    size_t dh() const { return dqkv() + np * kQkv; }                                   // [np][max(1024, dim_ff)]: dh, then dfeat
    size_t dz1() const { return dh() + np * hw; }
    size_t dd() const { return dz1() + np * kC1Out; }
    size_t dq() const { return dd() + np * kHeads; }
    size_t term() const { return dq() + np * 4; }
    size_t part() const { return term() + np; }                                        // [np / 16][256]
    size_t floats() const { return part() + np / 16 * 2 * kD; }
};

// ------------------------------------------------------------------------------------------------------------- head --
// One block a board, thread k feature k: d = q[a] - target, td, the derivative dq = w / n . clamp(d, -1, 1) at action a (a row of
// four, the other three zero), the loss term w . td, and the gradient into the last norm's output, dq . fc.weight[a][k].
__global__ __launch_bounds__(128) void qg_head_kernel(const float4 *__restrict__ q, const long long *__restrict__ actions,
                                                       const float *__restrict__ targets, const float *__restrict__ weights,
                                                       const float *__restrict__ fc, float *__restrict__ td_out, float4 *__restrict__ dq_out,
                                                       float *__restrict__ term, float *__restrict__ gx, int n)
{
    const size_t i = blockIdx.x;
    const int a = (int)(actions[i] & 3), k = threadIdx.x;
    const float4 qi = q[i];
    const float qa = a == 0 ? qi.x : a == 1 ? qi.y : a == 2 ? qi.z : qi.w;
    const float d = qa - targets[i], w = weights[i];
    const float dq = w / (float)n * fminf(fmaxf(d, -1.0f), 1.0f);
    gx[i * kD + k] = dq * fc[a * kD + k];
    if (k == 0) {
        const float td = fabsf(d) < 1.0f ? 0.5f * d * d : fabsf(d) - 0.5f;
        td_out[i] = td;
        term[i] = w * td;
        dq_out[i] = make_float4(a == 0 ? dq : 0.0f, a == 1 ? dq : 0.0f, a == 2 ? dq : 0.0f, a == 3 ? dq : 0.0f);
    }
}

// out[0] = sum(term[0 .. n-1]) / n: thread t adds the terms t, t + 256, .. in order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void qg_sum_kernel(const float *__restrict__ term, float *__restrict__ out, int n)
{
    __shared__ float red[256];
    const int t = threadIdx.x;
    float v = 0.0f;
    for (int i = t; i < n; i += 256) v += term[i];
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) out[0] = red[0] / (float)n;
}

// --------------------------------------------------------------------------------------------------- LayerNorm backward --
// A block of 512 a tile of 16 boards, a half wavefront a row (as the forward's statistics): with xhat = (s - mean) rstd and
// gy = g . gamma, ds = rstd (gy - mean(gy) - xhat mean(gy . xhat)). part[tile][0..127] = the tile's sum of g . xhat,
// part[tile][128..255] of g, its 16 rows added pairwise (rows past n are zero).
__global__ __launch_bounds__(512) void qg_ln_kernel(const float *__restrict__ G, const float *__restrict__ S, const float *__restrict__ norm,
                                                     const float *__restrict__ eps, float *__restrict__ dS, float *__restrict__ part, int n)
{
    __shared__ __attribute__((aligned(16))) float pg[2][16][kD];
    const int lane = threadIdx.x & 63, o = threadIdx.x >> 6;
    const int row = 2 * o + (lane >> 5), j = lane & 31, board = (int)blockIdx.x * 16 + row;
    const bool live = board < n;
    const f4 s = live ? load_f4(S + (size_t)board * kD + 4 * j) : splat(0.0f);
    const f4 g = live ? load_f4(G + (size_t)board * kD + 4 * j) : splat(0.0f);
    const float mean = half_sum(sum4(s)) / (float)kD;
    const f4 v = s - splat(mean);
    const float rstd = 1.0f / sqrtf(half_sum(sum4(v * v)) / (float)kD + eps[0]);
    const f4 xhat = v * splat(rstd), gy = g * load_w(norm + 4 * j);
    const float c1 = half_sum(sum4(gy)) / (float)kD, c2 = half_sum(sum4(gy * xhat)) / (float)kD;
    if (live) *reinterpret_cast<f4 *>(dS + (size_t)board * kD + 4 * j) = (gy - splat(c1) - xhat * splat(c2)) * splat(rstd);
    *reinterpret_cast<f4 *>(&pg[0][row][4 * j]) = g * xhat;
    *reinterpret_cast<f4 *>(&pg[1][row][4 * j]) = g;
    __syncthreads();
    if (threadIdx.x < 2 * kD) {
        const int which = threadIdx.x >> 7, k = threadIdx.x & (kD - 1);
        float r[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) r[i] = pg[which][i][k];
        part[(size_t)blockIdx.x * (2 * kD) + threadIdx.x] =
            (((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))) + (((r[8] + r[9]) + (r[10] + r[11])) + ((r[12] + r[13]) + (r[14] + r[15])));
    }
}

// out[t] = the tiles' part[tile][t] added in order, four partial sums (tile & 3) combined pairwise; `zero` (optional): two floats
// set to 0, the layer's LayerNorm-eps slots of the plain layout, which have no gradient
__global__ __launch_bounds__(256) void qg_tiles_kernel(const float *__restrict__ part, int tiles, float *__restrict__ out, float *__restrict__ zero)
{
    const int t = threadIdx.x;
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int i = 0;
    for (; i + 4 <= tiles; i += 4)
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] += part[(size_t)(i + u) * (2 * kD) + t];
#pragma unroll
    for (int u = 0; u < 3; ++u)
        if (i + u < tiles) a[u] += part[(size_t)(i + u) * (2 * kD) + t];
    out[t] = (a[0] + a[1]) + (a[2] + a[3]);
    if (zero && t < 2) zero[t] = 0.0f;
}

// ----------------------------------------------------------------------------------------------- attention backward --
// The probabilities are not kept: P_ij = exp(q_i . k_j / 4 - max_i) / sum_i from qkv and the forward's row maximum and sum.
// Scores and dP = V . dO^T of a tile are D[key][query] here (lane (query col, g) holds keys 4 g + r, as in the forward), so
// dS is, as it stands, the B operand of dQ^T = K^T . dS (A = K^T, lane (feature col, g) reading K[key 4 g + r][col]). Four key
// tiles go to four accumulators, combined pairwise. Also writes D_i = sum dO_i . O_i to dd [query][head] for the other kernel.
// With a QDrop (site 0; att is then the DROPPED attention output O = (P o M) V, M = the multipliers): dP_ij = M_ij (dO_i . V_j),
// the multiplier regenerated for element (head n + query) n + key; D_i = sum_j P_ij dP_ij = dO_i . O_i still.
template <class... MaybeDrop>
__global__ __launch_bounds__(64) void qg_att_dq_kernel(const float *__restrict__ qkv, const float *__restrict__ att, const float *__restrict__ datt,
                                                        const float *__restrict__ amax, const float *__restrict__ asum,
                                                        float *__restrict__ dqkv, float *__restrict__ dd, int n, MaybeDrop... drop)
{
    const int lane = threadIdx.x, g = lane >> 4, col = lane & 15, head = blockIdx.y;
    const int query = (int)blockIdx.x * 16 + col;
    const bool qlive = query < n;
    const float *base = qkv + head * kHead;
    const size_t orow = (size_t)query * kD + head * kHead + 4 * g;
    const f4 q = qlive ? load_f4(base + (size_t)query * kQkv + 4 * g) : splat(0.0f);
    const f4 dO = qlive ? load_f4(datt + orow) : splat(0.0f);
    const f4 O = qlive ? load_f4(att + orow) : splat(0.0f);
    const float D = lanes_sum(sum4(dO * O));
    const float m = qlive ? amax[(size_t)query * kHeads + head] : 0.0f, l = qlive ? asum[(size_t)query * kHeads + head] : 1.0f;
    if (g == 0 && qlive) dd[(size_t)query * kHeads + head] = D;
    const int tiles = (n + 15) / 16;
    f4 acc[4] = {splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f)};
    for (int t0 = 0; t0 < tiles; t0 += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + u;
            if (t < tiles) {
                const int key = 16 * t + col;
                const f4 k = key < n ? load_f4(base + (size_t)key * kQkv + kD + 4 * g) : splat(0.0f);
                const f4 v = key < n ? load_f4(base + (size_t)key * kQkv + 2 * kD + 4 * g) : splat(0.0f);
                f4 kt;
#pragma unroll
                for (int r = 0; r < 4; ++r) kt[r] = 16 * t + 4 * g + r < n ? base[(size_t)(16 * t + 4 * g + r) * kQkv + kD + col] : 0.0f;
                f4 s = splat(0.0f), dp = splat(0.0f);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s = __builtin_amdgcn_mfma_f32_16x16x4f32(k[r], q[r], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_16x16x4f32(v[r], dO[r], dp, 0, 0, 0);
                }
                if constexpr (sizeof...(MaybeDrop) != 0) {
                    const uint32_t e = ((uint32_t)head * (uint32_t)n + (uint32_t)query) * (uint32_t)n + (uint32_t)(16 * t + 4 * g);
#pragma unroll
                    for (int r = 0; r < 4; ++r) dp[r] *= qdrop_mult(drop..., e + r);
                }
                f4 ds;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = 16 * t + 4 * g + r < n ? expf(s[r] * 0.25f - m) / l : 0.0f;
                    ds[r] = p * (dp[r] - D);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kt[r], ds[r], acc[u], 0, 0, 0);
            }
        }
    }
    if (qlive) *reinterpret_cast<f4 *>(dqkv + (size_t)query * kQkv + head * kHead + 4 * g) = ((acc[0] + acc[1]) + (acc[2] + acc[3])) * splat(0.25f);
}

// One wavefront a (key tile, head), the query tiles streamed: scores and dP are D[query][key] here (A = Q resp. dO of the query
// tile, B = K resp. V of this key tile), so lane (key col, g) holds queries 4 g + r and P and dS are the B operands of
// dV^T = dO^T . P and dK^T = Q^T . dS (A: lane (feature col, g) reading dO resp. Q of query 4 g + r at feature col).
// With a QDrop (site 0): dP_ij = M_ij (dO_i . V_j) and dV_j = sum_i P_ij M_ij dO_i, the multipliers of this tile regenerated.
template <class... MaybeDrop>
__global__ __launch_bounds__(64) void qg_att_dkv_kernel(const float *__restrict__ qkv, const float *__restrict__ datt, const float *__restrict__ amax,
                                                         const float *__restrict__ asum, const float *__restrict__ dd, float *__restrict__ dqkv, int n,
                                                         MaybeDrop... drop)
{
    const int lane = threadIdx.x, g = lane >> 4, col = lane & 15, head = blockIdx.y;
    const int key = (int)blockIdx.x * 16 + col;
    const bool klive = key < n;
    const float *base = qkv + head * kHead, *dbase = datt + head * kHead;
    const f4 k = klive ? load_f4(base + (size_t)key * kQkv + kD + 4 * g) : splat(0.0f);
    const f4 v = klive ? load_f4(base + (size_t)key * kQkv + 2 * kD + 4 * g) : splat(0.0f);
    const int tiles = (n + 15) / 16;
    f4 acc_v[4] = {splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f)}, acc_k[4] = {splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f)};
    for (int t0 = 0; t0 < tiles; t0 += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + u;
            if (t < tiles) {
                const int qa = 16 * t + col;
                const f4 q = qa < n ? load_f4(base + (size_t)qa * kQkv + 4 * g) : splat(0.0f);
                const f4 dO = qa < n ? load_f4(dbase + (size_t)qa * kD + 4 * g) : splat(0.0f);
                f4 qt, dot, m, l, D;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int qr = 16 * t + 4 * g + r;
                    const bool live = qr < n;
                    qt[r] = live ? base[(size_t)qr * kQkv + col] : 0.0f;
                    dot[r] = live ? dbase[(size_t)qr * kD + col] : 0.0f;
                    m[r] = live ? amax[(size_t)qr * kHeads + head] : 0.0f;
                    l[r] = live ? asum[(size_t)qr * kHeads + head] : 1.0f;
                    D[r] = live ? dd[(size_t)qr * kHeads + head] : 0.0f;
                }
                f4 s = splat(0.0f), dp = splat(0.0f);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s = __builtin_amdgcn_mfma_f32_16x16x4f32(q[r], k[r], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_16x16x4f32(dO[r], v[r], dp, 0, 0, 0);
                }
                f4 p, ds;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    p[r] = klive && 16 * t + 4 * g + r < n ? expf(s[r] * 0.25f - m[r]) / l[r] : 0.0f;
                    if constexpr (sizeof...(MaybeDrop) != 0) {
                        const uint32_t e = ((uint32_t)head * (uint32_t)n + (uint32_t)(16 * t + 4 * g + r)) * (uint32_t)n + (uint32_t)key;
                        const float mult = qdrop_mult(drop..., e);
                        dp[r] *= mult;
                        ds[r] = p[r] * (dp[r] - D[r]);
                        p[r] *= mult;                                       // from here on P o M, dV's operand
                    } else {
                        ds[r] = p[r] * (dp[r] - D[r]);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    acc_v[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(dot[r], p[r], acc_v[u], 0, 0, 0);
                    acc_k[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(qt[r], ds[r], acc_k[u], 0, 0, 0);
                }
            }
        }
    }
    if (!klive) return;
    float *out = dqkv + (size_t)key * kQkv + head * kHead + 4 * g;
    *reinterpret_cast<f4 *>(out + kD) = ((acc_k[0] + acc_k[1]) + (acc_k[2] + acc_k[3])) * splat(0.25f);
    *reinterpret_cast<f4 *>(out + 2 * kD) = (acc_v[0] + acc_v[1]) + (acc_v[2] + acc_v[3]);
}

// ---------------------------------------------------------------------------------------------------- conv backward --
// dz2 [n][64][16] is the gradient at conv2's output with its ReLU mask applied (the embedding's dx launch). conv2.weight's
// gradient: a block an output channel, thread (group, input channel, tap): group = board & 3, the four groups' sums combined pairwise.
// dW2[oc][ic][dy][dx] = sum over boards and positions of dz2[oc][py][px] c1[ic][py + dy][px + dx]; db2[oc] = sum of dz2[oc].
__global__ __launch_bounds__(512) void qg_conv_dw2_kernel(const float *__restrict__ dz2, const float *__restrict__ c1, float *__restrict__ dW,
                                                           float *__restrict__ db, int n)
{
    __shared__ float red[4][4 * kC1], bred[4];
    const int t = threadIdx.x, j = t & 127, grp = t >> 7, oc = blockIdx.x;
    const int ic = j >> 2, dy = (j >> 1) & 1, dx = j & 1;
    float acc = 0.0f, bacc = 0.0f;
    for (int board = grp; board < n; board += 4) {
        const float *z = dz2 + (size_t)board * kFlat + oc * 16, *c = c1 + (size_t)board * kC1Out + ic * 25 + 5 * dy + dx;
#pragma unroll
        for (int py = 0; py < 4; ++py) {
            const f4 zr = load_f4(z + 4 * py);
#pragma unroll
            for (int px = 0; px < 4; ++px) acc = fmaf(zr[px], c[5 * py + px], acc);
            bacc += sum4(zr);
        }
    }
    red[grp][j] = acc;
    if (j == 0) bred[grp] = bacc;
    __syncthreads();
    if (t < 4 * kC1) dW[(size_t)oc * (4 * kC1) + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    if (t == 0) db[oc] = (bred[0] + bred[1]) + (bred[2] + bred[3]);
}

// The transposed convolution into conv1's output, a block a board: dz1[ic][y][x] = sum over oc, dy, dx of conv2.weight[oc][ic][dy][dx]
// dz2[oc][y - dy][x - dx] where that position exists, zero where conv1's ReLU was; four partial sums (oc & 3) combined pairwise.
__global__ __launch_bounds__(256) void qg_conv_dz1_kernel(const float *__restrict__ dz2, const float *__restrict__ c1, const float *__restrict__ P,
                                                           float *__restrict__ dz1)
{
    __shared__ float z[kFlat];
    const size_t board = blockIdx.x;
    for (int i = threadIdx.x; i < kFlat; i += 256) z[i] = dz2[board * kFlat + i];
    __syncthreads();
    for (int i = threadIdx.x; i < kC1Out; i += 256) {
        const int ic = i / 25, pos = i % 25, y = pos / 5, x = pos % 5;
        float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int oc0 = 0; oc0 < kC2; oc0 += 4)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int oc = oc0 + s;
                const f4 w = load_w(P + kPlC2W + (size_t)oc * (4 * kC1) + 4 * ic);
#pragma unroll
                for (int tap = 0; tap < 4; ++tap) {
                    const int py = y - (tap >> 1), px = x - (tap & 1);
                    if (py >= 0 && py < 4 && px >= 0 && px < 4) a[s] = fmaf(w[tap], z[oc * 16 + 4 * py + px], a[s]);
                }
            }
        const float v = (a[0] + a[1]) + (a[2] + a[3]);
        dz1[board * kC1Out + i] = c1[board * kC1Out + i] > 0.0f ? v : 0.0f;
    }
}

// conv1.weight's gradient, a block a channel: thread t adds its boards t, t + 256, .. in order (dW1[ch][dy][dx] = sum of dz1[ch][y][x]
// times the zero-padded tile value at (y + dy, x + dx), db1[ch] = sum of dz1[ch]), then a fixed tree over the 256 threads.
__global__ __launch_bounds__(256) void qg_conv_dw1_kernel(const float *__restrict__ dz1, const uint8_t *__restrict__ boards, float *__restrict__ dW,
                                                           float *__restrict__ db, int n)
{
    __shared__ float red[5][256];
    const int t = threadIdx.x, ch = blockIdx.x;
    float a[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int board = t; board < n; board += 256) {
        float pad[36];
#pragma unroll
        for (int i = 0; i < 36; ++i) pad[i] = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t code = boards[(size_t)board * 16 + i];
            pad[6 * ((i >> 2) + 1) + (i & 3) + 1] = code ? __uint_as_float((127u + code) << 23) : 0.0f;
        }
        const float *z = dz1 + (size_t)board * kC1Out + ch * 25;
#pragma unroll
        for (int y = 0; y < 5; ++y)
#pragma unroll
            for (int x = 0; x < 5; ++x) {
                const float zv = z[5 * y + x];
                a[0] = fmaf(zv, pad[6 * y + x], a[0]);
                a[1] = fmaf(zv, pad[6 * y + x + 1], a[1]);
                a[2] = fmaf(zv, pad[6 * y + 6 + x], a[2]);
                a[3] = fmaf(zv, pad[6 * y + 7 + x], a[3]);
                a[4] += zv;
            }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) red[k][t] = a[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s)
#pragma unroll
            for (int k = 0; k < 5; ++k) red[k][t] += red[k][t + s];
        __syncthreads();
    }
    if (t < 4) dW[ch * 4 + t] = red[t][0];
    if (t == 4) db[ch] = red[4][0];
}

// ------------------------------------------------------------------------------------------------------------- host --
// the training pass's workspace: GradWorkspace, then dsm [np][128], the LayerNorm backward's ds x a site's multipliers
struct TrainWorkspace : GradWorkspace {
    using GradWorkspace::GradWorkspace;
    size_t dsm() const { return GradWorkspace::floats(); }
    size_t floats() const { return dsm() + np * kD; }
};

// A loss and gradient pass: g2048_qnet_loss_grad (kDrop false, GradWorkspace) or g2048_qnet_loss_grad_dropout (TrainWorkspace). The
// forward is qb_forward with every layer's activations kept, so q has the bits of the forward-only pass; then the loss and the
// backward, one phase a launch (the head of g2048_qnet_grad.hip). kDrop true: where the masks go is in the head of
// g2048_qnet_train.hip; a site with p4[s] == 0 launches the instantiation without a QDrop.
template <bool kDrop>
int qg_pass(const char *entry, const QbCall &c)
{
    if (c.n == 0) return G2048_OK;
    if (const int rc = qb_check<kDrop>(entry, c)) return rc;
    hipStream_t s = static_cast<hipStream_t>(c.stream);
    const size_t n = c.n, nl = (size_t)c.n_layers;
    const std::conditional_t<kDrop, TrainWorkspace, GradWorkspace> ws(n, c.dim_ff, c.n_layers);
    float *base = static_cast<float *>(c.workspace);
    const float *P = c.plain;
    float *G = c.grad;
    const int ni = (int)n, ff = c.dim_ff;
    const unsigned tiles = (unsigned)(ws.np / 16);
    const float *none = nullptr;
    float *nowhere = nullptr;
    const float *fc = P + kPlLayer0 + nl * pl_layer(ff);

    // ---- the forward, its activations kept
    float *feat = base + ws.feat(), *c1 = base + ws.c1();
    qb_forward<kDrop>(c, tiles, feat, c1, [&](size_t l, bool) {
        return LayerBuffers{base + ws.x(l), base + ws.qkv(l), base + ws.att(l), base + ws.x1(l), base + ws.pre1(l), base + ws.h(l),
                            base + ws.x(l + 1), base + ws.pre2(l), base + ws.amax(l), base + ws.asum(l)};
    });

    // ---- the loss and the backward
    const auto dx = [&](const float *dY, int M, const float *W, int K, const float *res, const float *mask, float *dX) {
        hipLaunchKernelGGL(qg_dx_kernel<>, dim3((unsigned)(K + 63) / 64, tiles), dim3(256), 0, s, dY, M, W, K, res, mask, dX, ni);
    };
    const auto dw = [&](const float *dY, int ldy, int M, const float *X, int K, float *dW, float *db) {
        hipLaunchKernelGGL(qg_dw_kernel, dim3((unsigned)(K + 63) / 64, (unsigned)(M + 15) / 16), dim3(256), 0, s, dY, ldy, M, X, K, dW, db, ni);
    };
    float *part = base + ws.part();
    const auto ln = [&](const float *g, const float *pre, const float *norm, const float *eps, float *ds, float *dnorm, float *zero) {
        hipLaunchKernelGGL(qg_ln_kernel, dim3(tiles), dim3(512), 0, s, g, pre, norm, eps, ds, part, ni);
        hipLaunchKernelGGL(qg_tiles_kernel, dim3(1), dim3(256), 0, s, static_cast<const float *>(part), (int)tiles, dnorm, zero);
    };
    float *ga = base + ws.ga(), *gb = base + ws.gb(), *ds = base + ws.ds(), *datt = base + ws.datt(), *dqkv = base + ws.dqkv(),
          *dh = base + ws.dh(), *dz1 = base + ws.dz1(), *dd = base + ws.dd(), *dq = base + ws.dq(), *term = base + ws.term();
    // ds x the multipliers of site 1 or 3: what enters the dropped projection's dW and dX (ds itself where the site is off)
    const auto scaled = [&](const QDrop *d) -> const float * {
        if constexpr (kDrop) {
            if (d) {
                float *dsm = base + ws.dsm();
                hipLaunchKernelGGL(qt_scale_kernel<QDrop>, dim3(blocks_for(n * kD, 256)), dim3(256), 0, s, static_cast<const float *>(ds), dsm, *d,
                                   (uint32_t)(n * kD));
                return dsm;
            }
        }
        return ds;
    };
    hipLaunchKernelGGL(qg_head_kernel, dim3((unsigned)n), dim3(128), 0, s, reinterpret_cast<const float4 *>(c.q),
                       reinterpret_cast<const long long *>(c.actions), c.targets, c.weights, fc, c.td, reinterpret_cast<float4 *>(dq), term, ga, ni);
    hipLaunchKernelGGL(qg_sum_kernel, dim3(1), dim3(256), 0, s, static_cast<const float *>(term), c.loss, ni);
    {
        float *Gfc = G + kPlLayer0 + nl * pl_layer(ff);
        dw(dq, 4, 4, base + ws.x(nl), kD, Gfc, Gfc + 4 * kD);
    }
    for (size_t l = nl; l-- > 0;) {
        const size_t lo = kPlLayer0 + l * pl_layer(ff);
        const float *L = P + lo, *norms = L + pl_norm(ff);
        float *GL = G + lo, *gnorms = GL + pl_norm(ff);
        const float *x0 = base + ws.x(l), *qkv = base + ws.qkv(l), *att = base + ws.att(l), *x1 = base + ws.x1(l), *h = base + ws.h(l);
        const float *amax = base + ws.amax(l), *asum = base + ws.asum(l);
        const DropSites st(kDomQnetDropout, c.seed, c.call_index, (int)l, kDrop ? c.p4 : nullptr);
        ln(ga, base + ws.pre2(l), norms + 2 * kD, norms + 4 * kD + 1, ds, gnorms + 2 * kD, gnorms + 4 * kD);
        const float *d3 = scaled(st.at(3));
        dw(d3, kD, kD, h, ff, GL + pl_w2(ff), GL + pl_b2(ff));
        launch_site<kDrop>(st.at(2), [](auto... d) { return qg_dx_kernel<decltype(d)...>; }, dim3((unsigned)(ff + 63) / 64, tiles), dim3(256), s, d3,
                           kD, L + pl_w2(ff), ff, none, h, dh, ni);
        dw(dh, ff, ff, x1, kD, GL + kPlW1, GL + pl_b1(ff));
        dx(dh, ff, L + kPlW1, kD, ds, none, gb);
        ln(gb, base + ws.pre1(l), norms, norms + 4 * kD, ds, gnorms, nowhere);
        const float *d1 = scaled(st.at(1));
        dw(d1, kD, kD, att, kD, GL + kPlOutW, GL + kPlOutB);
        dx(d1, kD, L + kPlOutW, kD, none, none, datt);
        launch_site<kDrop>(st.at(0), [](auto... d) { return qg_att_dq_kernel<decltype(d)...>; }, dim3(tiles, kHeads), dim3(64), s, qkv, att,
                           static_cast<const float *>(datt), amax, asum, dqkv, dd, ni);
        launch_site<kDrop>(st.at(0), [](auto... d) { return qg_att_dkv_kernel<decltype(d)...>; }, dim3(tiles, kHeads), dim3(64), s, qkv,
                           static_cast<const float *>(datt), amax, asum, static_cast<const float *>(dd), dqkv, ni);
        dw(dqkv, kQkv, kQkv, x0, kD, GL + kPlInW, GL + kPlInB);
        dx(dqkv, kQkv, L + kPlInW, kD, ds, none, ga);
    }
    dw(ga, kD, kD, feat, kFlat, G + kPlEmbW, G + kPlEmbB);
    dx(ga, kD, P + kPlEmbW, kFlat, none, feat, dh);
    hipLaunchKernelGGL(qg_conv_dw2_kernel, dim3(kC2), dim3(512), 0, s, static_cast<const float *>(dh), static_cast<const float *>(c1),
                       G + kPlC2W, G + kPlC2B, ni);
    hipLaunchKernelGGL(qg_conv_dz1_kernel, dim3((unsigned)n), dim3(256), 0, s, static_cast<const float *>(dh), static_cast<const float *>(c1), P, dz1);
    hipLaunchKernelGGL(qg_conv_dw1_kernel, dim3(kC1), dim3(256), 0, s, static_cast<const float *>(dz1), static_cast<const uint8_t *>(c.boards),
                       G + kPlC1W, G + kPlC1B, ni);
    return check_launch(entry);
}

}  // namespace
