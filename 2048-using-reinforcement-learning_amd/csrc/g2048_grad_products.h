// g2048_grad_products.h -- the two general products of a gradient pass on the f32 matrix cores, shared by g2048_qnet_grad.hip
// (the Q-network's backward) and g2048_ppo_grad.hip (the PPO actor's and critic's): the data gradient dX = dY . W and the
// weight gradient dW = dY^T . X with db = sum dY, for row-major f32 operands as they lie in a plain parameter buffer and a
// workspace. Device code, included by those two files, g2048_qnet_train.hip (through g2048_qnet_grad_bwd.h) and g2048_tpolicy_grad.hip
// (the transformer policy's backward over n boards) and nothing else; every
// kernel is per translation unit. The rules are
// g2048_qnet_grad.hip's: every output element is one wavefront's fixed-order accumulation, nothing past row n is read or written.
#pragma once
#include <hip/hip_runtime.h>

#include "g2048_mfma.h"
#include "g2048_qnet_drop.h"

namespace {

using namespace g2048;

__device__ inline float sum4(f4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }
__device__ inline f4 sum8(const f4 (&a)[8]) { return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])); }

// --------------------------------------------------------------------------------------------------------------- dx --
// dX [n][K] = dY [n][M] . W [M][K] (+ RES, or where MASK <= 0 zero): the tile is D[feature 16 o + 4 g + r][board col]. Lane (col, g):
// the A operand is the column slice W[16 c + 4 g + r][16 o + col] of chunk c (M in chunks of 16), the B operand dY[board][16 c +
// 4 g ..], one 16-byte load. As in the forward's product, eight chunks at a time into eight accumulators, combined pairwise.
template <int N>
__device__ inline void dx_chunks(const float *__restrict__ wcol, size_t K, const float *__restrict__ yrow, bool live, f4 (&acc)[8])
{
    f4 w[N], y[N];
#pragma unroll
    for (int c = 0; c < N; ++c) {
#pragma unroll
        for (int r = 0; r < 4; ++r) w[c][r] = wcol[(size_t)(16 * c + r) * K];
        y[c] = live ? load_f4(yrow + 16 * c) : splat(0.0f);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[c][r], y[c][r], acc[c], 0, 0, 0);
}

// four wavefronts a block = four feature tiles of one board tile; grid (K / 64 up, board tiles). M is a multiple of 32. With a
// QDrop (the Q-network's training pass, site 2) dX is the gradient at a dropped layer's input: after the ReLU mask it is multiplied
// by the site's regenerated m, element board K + feature.
template <class... MaybeDrop>
__global__ __launch_bounds__(256) void qg_dx_kernel(const float *__restrict__ dY, int M, const float *__restrict__ W, int K,
                                                     const float *__restrict__ res, const float *__restrict__ mask, float *__restrict__ dX, int n,
                                                     MaybeDrop... drop)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const int o = (int)blockIdx.x * 4 + wave;
    if (16 * o >= K) return;
    const int board = (int)blockIdx.y * 16 + col;
    const bool live = board < n;
    const float *wcol = W + (size_t)(4 * g) * K + 16 * o + col, *yrow = dY + (size_t)board * M + 4 * g;
    f4 acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = splat(0.0f);
    int m = 0;
    for (; m + 128 <= M; m += 128) dx_chunks<8>(wcol + (size_t)m * K, (size_t)K, yrow + m, live, acc);
    for (; m < M; m += 32) dx_chunks<2>(wcol + (size_t)m * K, (size_t)K, yrow + m, live, acc);
    if (!live) return;
    f4 v = sum8(acc);
    const size_t at = (size_t)board * K + 16 * o + 4 * g;
    if (res) v = load_f4(res + at) + v;                                     // the residual's two paths, in this order
    if (mask) {
        const f4 a = load_f4(mask + at);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = a[r] > 0.0f ? v[r] : 0.0f;
    }
    if constexpr (sizeof...(MaybeDrop) != 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] *= qdrop_mult(drop..., (uint32_t)at + (uint32_t)r);
    }
    *reinterpret_cast<f4 *>(dX + at) = v;
}

// --------------------------------------------------------------------------------------------------------------- dw --
// dW [M][K] = sum over the boards of dY[board][M] . X[board][K]; db [M] = sum over the boards of dY. The tile is D[row 16 mo + 4 g + r]
// [column 16 ko + col]; the contraction runs over the boards in tiles of 16 (board 16 t + 4 g + r on MFMA r of lane group g): the A
// operand is dY[board][16 mo + col] (row stride ldy; rows past M and boards past n read as zero), the B operand X[board][16 ko + col].
// Eight board tiles at a time into eight accumulators, combined pairwise. The wavefronts of column tile 0 also add their A operands
// up into db. Four wavefronts a block = four column tiles; grid (K / 64 up, M / 16 up).
__global__ __launch_bounds__(256) void qg_dw_kernel(const float *__restrict__ dY, int ldy, int M, const float *__restrict__ X, int K,
                                                     float *__restrict__ dW, float *__restrict__ db, int n)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const int ko = (int)blockIdx.x * 4 + wave, mo = blockIdx.y;
    if (16 * ko >= K) return;
    const int mrow = 16 * mo + col;
    const bool mlive = mrow < M;
    const float *ycol = dY + mrow, *xcol = X + 16 * ko + col;
    const int tiles = (n + 15) / 16;
    f4 acc[8];
    float bs[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        acc[c] = splat(0.0f);
        bs[c] = 0.0f;
    }
    for (int t0 = 0; t0 < tiles; t0 += 8) {
        f4 a[8], b[8];
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int board = 16 * (t0 + c) + 4 * g + r;
                a[c][r] = board < n && mlive ? ycol[(size_t)board * ldy] : 0.0f;
                b[c][r] = board < n ? xcol[(size_t)board * K] : 0.0f;
            }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][r], b[c][r], acc[c], 0, 0, 0);
#pragma unroll
        for (int c = 0; c < 8; ++c) bs[c] += sum4(a[c]);
    }
    const f4 v = sum8(acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * mo + 4 * g + r;
        if (row < M) dW[(size_t)row * K + 16 * ko + col] = v[r];
    }
    if (ko == 0) {
        const float s = lanes_sum(((bs[0] + bs[1]) + (bs[2] + bs[3])) + ((bs[4] + bs[5]) + (bs[6] + bs[7])));
        if (g == 0 && mlive) db[mrow] = s;
    }
}

}  // namespace
