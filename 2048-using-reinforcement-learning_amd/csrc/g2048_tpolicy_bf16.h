// g2048_tpolicy_bf16.h -- the three bf16 products of the transformer policy's gradient pass in its bf16 feed-forward mode
// (include/g2048_tbf16.h; tg_pass<kDrop, true> of g2048_tpolicy_grad_pass.h, which includes this header) and the launch that packs
// the bf16 copies of a layer's two feed-forward weights. Operands are rounded to bf16 (round to nearest even: the float -> __bf16
// cast, gfx950's v_cvt_pk_bf16_f32) where they are read, the products run on v_mfma_f32_16x16x32_bf16 and accumulate in f32 in a
// fixed order; biases, residuals, masks and dropout multipliers are applied in f32 after the product. Kernels are templates, so
// only a library that launches one holds it; the f32 libraries name none. Device code, per translation unit.
//
// The 16x16x32 operand: lane (col = lane & 15, g = lane >> 4) holds elements k = 8 g .. 8 g + 7 of row `col` of A and of column
// `col` of B, 16 contiguous bytes of a row-major bf16 array whose rows run along the contraction; D[4 g + r][col] is register r.
#pragma once
#include <hip/hip_runtime.h>

#include "g2048_mfma.h"
#include "g2048_qnet_drop.h"

namespace {

using namespace g2048;

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

__device__ inline bf16x8 tb_zero8() { return __builtin_bit_cast(bf16x8, u4{0u, 0u, 0u, 0u}); }

// eight consecutive elements of a row as one operand: f32 rounded here, bf16 as stored
__device__ inline bf16x8 tb_load8(const float *p, bool live)
{
    return live ? to_bf16x8(load_f4(p), load_f4(p + 4)) : tb_zero8();
}
__device__ inline bf16x8 tb_load8(const __bf16 *p, bool live) { return live ? *reinterpret_cast<const bf16x8 *>(p) : tb_zero8(); }

__device__ inline void tb_store4(float *p, f4 v) { *reinterpret_cast<f4 *>(p) = v; }
__device__ inline void tb_store4(__bf16 *p, f4 v) { *reinterpret_cast<bf16x4 *>(p) = bf16x4{(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]}; }

// ------------------------------------------------------------------------------------------------------------- pack --
// The bf16 copies of up to two row-major f32 matrices (blockIdx.y picks one): plain[r][c] = rnd(W[r][c]) and trans[c][r] the same
// value, either left out where its pointer is null. A thread an element. The pass packs a layer's W1 [dim_ff][64] and W2
// [64][dim_ff] in one launch a layer and call: the plain copies are the forward's operands, the transposed ones the data gradients'.
template <int = 0>                                   // a template, as every kernel here: only a library that launches it holds it
__global__ __launch_bounds__(256) void tb_pack_kernel(const float *__restrict__ Wa, int ra, int ca, __bf16 *__restrict__ pa, __bf16 *__restrict__ ta,
                                                       const float *__restrict__ Wb, int rb, int cb, __bf16 *__restrict__ pb, __bf16 *__restrict__ tb)
{
    const bool second = blockIdx.y != 0;
    const float *W = second ? Wb : Wa;
    const int R = second ? rb : ra, Cn = second ? cb : ca;
    __bf16 *plain = second ? pb : pa, *trans = second ? tb : ta;
    const size_t e = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= (size_t)R * (size_t)Cn) return;
    const __bf16 v = (__bf16)W[e];
    if (plain) plain[e] = v;
    if (trans) trans[(e % (size_t)Cn) * (size_t)R + e / (size_t)Cn] = v;
}

// ----------------------------------------------------------------------------------------------------------- linear --
// Y [n][M] = epilogue(rnd(X) [n][K] . W^T), W [M][K] bf16 row-major (a packed copy), X f32 or bf16, Y f32 or bf16; K a multiple of 32,
// M of 16. tg_linear_kernel's geometry: the tile is D[feature 16 o + 4 g + r][row col], four wavefronts a block = four feature
// tiles of one row tile, grid (M / 64 up, row tiles). Chunk c of K (32 wide, one MFMA) accumulates into acc[c & 3], combined
// pairwise: the order is fixed. The epilogue, with v the sum, bias its start (null: none) and element = row M + feature:
//   DX false (the forward's)  sites 1 and 3 (no ReLU) v x m + res; site 2 relu(v) x m: tg_linear_kernel's
//   DX true  (dX = dY . W through the transposed copy)  res + v, zero where mask <= 0 (the stored bf16 hidden layer), x m:
//            qg_dx_kernel's
template <bool DX, bool RELU, class TX, class TY, class... MaybeDrop>
__global__ __launch_bounds__(256) void tb_linear_kernel(const TX *__restrict__ X, int K, const __bf16 *__restrict__ W, const float *__restrict__ bias,
                                                         const float *__restrict__ res, const __bf16 *__restrict__ mask, TY *__restrict__ Y, int M,
                                                         int n, MaybeDrop... drop)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const int o = (int)blockIdx.x * 4 + wave;
    if (16 * o >= M) return;
    const int row = (int)blockIdx.y * 16 + col;
    const bool live = row < n;
    const __bf16 *wrow = W + (size_t)(16 * o + col) * K + 8 * g;
    const TX *xrow = X + (size_t)(live ? row : 0) * K + 8 * g;
    f4 acc[4] = {bias ? load_w(bias + 16 * o + 4 * g) : splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f)};
    const int chunks = K / 32;
    int c = 0;
    for (; c + 4 <= chunks; c += 4) {
        bf16x8 w[4], x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            w[u] = tb_load8(wrow + 32 * (c + u), true);
            x[u] = tb_load8(xrow + 32 * (c + u), live);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[u], x[u], acc[u], 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 3; ++u)
        if (c + u < chunks)
            acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tb_load8(wrow + 32 * (c + u), true), tb_load8(xrow + 32 * (c + u), live), acc[u], 0, 0, 0);
    if (!live) return;
    f4 v = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    const size_t at = (size_t)row * M + 16 * o + 4 * g;
    if constexpr (DX) {
        if (res) v = load_f4(res + at) + v;
        if (mask) {
            const bf16x4 a = *reinterpret_cast<const bf16x4 *>(mask + at);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (float)a[r] > 0.0f ? v[r] : 0.0f;
        }
        if constexpr (sizeof...(MaybeDrop) != 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] *= qdrop_mult(drop..., (uint32_t)at + (uint32_t)r);
        }
    } else {
        if constexpr (sizeof...(MaybeDrop) != 0 && !RELU) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] *= qdrop_mult(drop..., (uint32_t)at + (uint32_t)r);
        }
        if (res) v = load_f4(res + at) + v;
        if (RELU) v = relu_nan(v);
        if constexpr (sizeof...(MaybeDrop) != 0 && RELU) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] *= qdrop_mult(drop..., (uint32_t)at + (uint32_t)r);
        }
    }
    tb_store4(Y + at, v);
}

// ------------------------------------------------------------------------------------------------ split weight gradient --
// part[chunk][M][K] = the chunk's rnd(dY)^T . rnd(X), bpart[chunk][M] = the chunk's sum of dY as stored (f32 values unrounded), over the
// rows [chunk_rows c, min(n, chunk_rows (c + 1))): tg_dw_split_kernel's split and outputs. dY [n][M] and X [n][K], each f32 or bf16;
// M and K multiples of 16. The contraction runs over the rows, so both operands are wanted across rows: a block stages 32 rows of
// 64 columns of each through LDS -- a thread reads eight consecutive columns of one row (16 or 32 bytes) and writes them, rounded,
// into the transposed image t[column][row] -- and a lane's operand is then 16 contiguous bytes, t[column][8 g ..]. An image row is
// 32 rows = 64 bytes, pitched to 80: the sixteen rows a ds_read_b128 group takes start at dword 20 col, which are sixteen different
// multiples of 4 modulo 64, so the read is conflict-free; the 2-byte writes of one instruction go to eight image rows x 8 rows each
// and are 2-way at worst. A block is 64 rows of dW (four tiles a wavefront, which share its B operand) x 64 columns (a tile a
// wavefront); grid (K / 64 up, M / 64 up, chunks). Every accumulator is one chain over the chunk's row steps in order. The blocks of
// column tile 0 also add up dY: thread (row slot, eight columns) in row order, the 32 slots pairwise.
constexpr int kTbStep = 32, kTbPitch = 40;

template <class T>
__device__ inline void tb_stage(const T *__restrict__ src, int width, int c0, int r0, int row1, __bf16 (*image)[kTbPitch], float (&sums)[8])
{
    const int r = threadIdx.x >> 3, c8 = (int)(threadIdx.x & 7) * 8;
    const int row = r0 + r, column = c0 + c8;
    float v[8];
    if (row < row1 && column < width) {
        const T *p = src + (size_t)row * width + column;
        if constexpr (sizeof(T) == 4) {
            const f4 lo = load_f4(p), hi = load_f4(p + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = lo[j], v[4 + j] = hi[j];
        } else {
            const bf16x8 b = *reinterpret_cast<const bf16x8 *>(p);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (float)b[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        image[c8 + j][r] = (__bf16)v[j];
        sums[j] += v[j];
    }
}

template <class TA, class TB>
__global__ __launch_bounds__(256) void tb_dw_split_kernel(const TA *__restrict__ dY, int M, const TB *__restrict__ X, int K, float *__restrict__ part,
                                                           float *__restrict__ bpart, int n, int chunk_rows)
{
    __shared__ __attribute__((aligned(16))) __bf16 At[64][kTbPitch];
    __shared__ __attribute__((aligned(16))) __bf16 Bt[64][kTbPitch];
    __shared__ float red[kTbStep][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const int k0 = (int)blockIdx.x * 64, m0 = (int)blockIdx.y * 64, chunk = blockIdx.z;
    const int row0 = chunk * chunk_rows, row1 = min(n, row0 + chunk_rows);
    f4 acc[4] = {splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f)};
    float bs[8], unused[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bs[j] = unused[j] = 0.0f;
    for (int r0 = row0; r0 < row1; r0 += kTbStep) {
        __syncthreads();                                                   // the last step's operands are read
        tb_stage(dY, M, m0, r0, row1, At, bs);
        tb_stage(X, K, k0, r0, row1, Bt, unused);
        __syncthreads();
        const bf16x8 b = *reinterpret_cast<const bf16x8 *>(&Bt[16 * wave + col][8 * g]);
#pragma unroll
        for (int t = 0; t < 4; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8 *>(&At[16 * t + col][8 * g]), b, acc[t], 0, 0, 0);
    }
    float *out = part + (size_t)chunk * M * K;
    const int column = k0 + 16 * wave + col;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m0 + 16 * t + 4 * g + r;
            if (row < M && column < K) out[(size_t)row * K + column] = acc[t][r];
        }
    if (blockIdx.x == 0) {
        const int slot = threadIdx.x >> 3, c8 = (int)(threadIdx.x & 7) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) red[slot][c8 + j] = bs[j];
        __syncthreads();
        if (threadIdx.x < 64 && m0 + (int)threadIdx.x < M) {
            float s[kTbStep];
#pragma unroll
            for (int i = 0; i < kTbStep; ++i) s[i] = red[i][threadIdx.x];
#pragma unroll
            for (int w = kTbStep / 2; w > 0; w >>= 1)
#pragma unroll
                for (int i = 0; i < w; ++i) s[i] = s[2 * i] + s[2 * i + 1];
            bpart[(size_t)chunk * M + m0 + threadIdx.x] = s[0];
        }
    }
}

}  // namespace
