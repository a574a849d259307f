// g2048_tpolicy.hip -- the reference's transformer policy (models/transformer.py:4-40, eval mode) on the matrix cores of
// gfx950, one launch per forward pass (C-ABI: include/g2048.h, g2048_tpolicy_*).
//
//   tpolicy_pack_matrix_kernel  one weight matrix [rows][K] (plus, for the two heads, a second one stacked under it) into 1 KiB
//                               MFMA fragments: a lane's A operand is one 16-byte load.
//   tpolicy_pack_params_kernel  the embedding, every bias, the LayerNorm weights and their eps into the blob's f32 section.
//   tpolicy_forward_kernel      Linear(1,64) -> L x TransformerEncoderLayer(64, 4 heads, dim_ff, relu, post-norm) -> flatten ->
//                               Linear(1024,128)+ReLU -> Linear(128,64)+ReLU -> {Linear(64,4)+softmax | Linear(64,1)}.
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

#include "../../include/g2048.h"
#include "g2048_host.h"

namespace {

using namespace g2048;

typedef float f4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------------------------------------ shapes and layouts --
constexpr int kD = 64, kHeads = 4, kTok = 16, kFc1 = 128, kFc2 = 64, kFlat = kTok * kD;
constexpr int kFrag = 64 * 16;                       // bytes of one fragment

// plain f32 layout (g2048_tpolicy_pack's input; include/g2048.h)
constexpr int kPlainEmb = 0, kPlainLayer0 = 2 * kD;
constexpr int kPlInW = 0, kPlInB = kPlInW + 3 * kD * kD, kPlOutW = kPlInB + 3 * kD, kPlOutB = kPlOutW + kD * kD, kPlW1 = kPlOutB + kD;
__host__ __device__ constexpr int pl_b1(int ff) { return kPlW1 + ff * kD; }
__host__ __device__ constexpr int pl_w2(int ff) { return pl_b1(ff) + ff; }
__host__ __device__ constexpr int pl_b2(int ff) { return pl_w2(ff) + kD * ff; }
__host__ __device__ constexpr int pl_norm(int ff) { return pl_b2(ff) + kD; }             // norm1.w norm1.b norm2.w norm2.b eps1 eps2
__host__ __device__ constexpr int pl_layer(int ff) { return pl_norm(ff) + 4 * kD + 2; }
constexpr int kPlFc1W = 0, kPlFc1B = kPlFc1W + kFc1 * kFlat, kPlFc2W = kPlFc1B + kFc1, kPlFc2B = kPlFc2W + kFc2 * kFc1,
              kPlActW = kPlFc2B + kFc2, kPlActB = kPlActW + 4 * kD, kPlCriW = kPlActB + 4, kPlCriB = kPlCriW + kD, kPlTail = kPlCriB + 1;

// packed layout: per layer the fragments of in_proj (12 row tiles), out_proj (4), linear1 (dim_ff / 16), linear2 (4); then fc1
// (8), fc2 (4), the head tile (1); then the f32 section. A matrix's fragments are ordered [row tile o][chunk c]; a chunk is 16
// input features (f32) or 32 (bf16). f32 section: emb.w emb.b | per layer: in_proj_bias 192, out_proj.bias 64, b1 dim_ff,
// b2 64, norm1.w norm1.b norm2.w norm2.b 256, eps1 eps2 0 0 | fc1.b 128, fc2.b 64, head bias 16 (actor 4, critic 1, zeros).
struct Layout {
    int ff, layers, chunk;
    __host__ __device__ Layout(bool bf16, int dim_ff, int n_layers) : ff(dim_ff), layers(n_layers), chunk(bf16 ? 32 : 16) {}
    __host__ __device__ int chunks(int k) const { return k / chunk; }
    __host__ __device__ size_t out_proj() const { return (size_t)12 * chunks(kD); }      // fragment indices within a layer
    __host__ __device__ size_t w1() const { return out_proj() + (size_t)4 * chunks(kD); }
    __host__ __device__ size_t w2() const { return w1() + (size_t)(ff / 16) * chunks(kD); }
    __host__ __device__ size_t layer_frags() const { return w2() + (size_t)4 * chunks(ff); }
    __host__ __device__ size_t fc1() const { return (size_t)layers * layer_frags(); }
    __host__ __device__ size_t fc2() const { return fc1() + (size_t)(kFc1 / 16) * chunks(kFlat); }
    __host__ __device__ size_t heads() const { return fc2() + (size_t)(kFc2 / 16) * chunks(kFc1); }
    __host__ __device__ size_t params() const { return (heads() + chunks(kD)) * kFrag; }  // byte offset of the f32 section
    __host__ __device__ int layer_params() const { return 3 * kD + kD + ff + kD + 4 * kD + 4; }
    __host__ __device__ int n_params() const { return 2 * kD + layers * layer_params() + kFc1 + kFc2 + 16; }
    __host__ __device__ size_t bytes() const { return params() + (size_t)n_params() * 4; }
    __host__ __device__ size_t plain_floats() const { return (size_t)kPlainLayer0 + (size_t)layers * pl_layer(ff) + kPlTail; }
};

__device__ __host__ inline uint32_t bf16_rne(float v)
{
    const uint32_t u = __float_as_uint(v);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;        // finite inputs: round to nearest even by integer add
}

// ------------------------------------------------------------------------------------------------------------- pack --
// One thread per packed 32-bit word (f32: one weight; bf16: two) of a matrix of rows_a + rows_b rows (a over b, rows past
// them zero) and K columns: word w of lane l of fragment (o, c) = W[16 o + (l & 15)][k], k as the header says.
template <bool BF16>
__global__ __launch_bounds__(256) void tpolicy_pack_matrix_kernel(const float *__restrict__ a, int rows_a, const float *__restrict__ b,
                                                                   int rows_b, int K, unsigned words, uint32_t *__restrict__ packed)
{
    const unsigned w = blockIdx.x * 256u + threadIdx.x;
    if (w >= words) return;
    constexpr int kChunk = BF16 ? 32 : 16;
    const int chunks = K / kChunk;
    const int frag = (int)(w / 256u), lane = (int)(w % 256u) / 4, word = (int)(w % 4u);
    const int o = frag / chunks, c = frag % chunks;
    const int row = 16 * o + (lane & 15), g = lane >> 4;
    auto weight = [&](int k) {
        if (row < rows_a) return a[(size_t)row * K + k];
        if (row < rows_a + rows_b) return b[(size_t)(row - rows_a) * K + k];
        return 0.0f;
    };
    if (BF16) {
        uint32_t pair[2];
        for (int q = 0; q < 2; ++q) {
            const int j = 2 * word + q;
            pair[q] = bf16_rne(weight(32 * c + 16 * (j >> 2) + 4 * g + (j & 3)));
        }
        packed[w] = pair[0] | (pair[1] << 16);
    } else {
        packed[w] = __float_as_uint(weight(16 * c + 4 * g + word));
    }
}

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
constexpr int kWaves = 4, kE = 4;                    // wavefronts per block, boards per wavefront: 16 boards per block
constexpr int kTokStride = kD + 4;                   // LDS strides in floats: + 4 spreads the 16-byte accesses over the banks
constexpr int kBoardStride = kTok * kTokStride + 4;
constexpr int kH1Stride = kFc1 + 4, kH2Stride = kFc2 + 4;
constexpr int kLdsFloats = 16 * kBoardStride;
static_assert(16 * kH1Stride + 16 * kH2Stride <= kLdsFloats, "the fc1 / fc2 outputs reuse the encoder-output buffer");

__device__ inline f4 relu(f4 v)
{
    return f4{fmaxf(v[0], 0.0f), fmaxf(v[1], 0.0f), fmaxf(v[2], 0.0f), fmaxf(v[3], 0.0f)};
}

__device__ inline bf16x8 to_bf16x8(f4 lo, f4 hi)
{
    // the float -> __bf16 cast is gfx950's v_cvt_pk_bf16_f32 (round to nearest even, two values per instruction)
    return bf16x8{(__bf16)lo[0], (__bf16)lo[1], (__bf16)lo[2], (__bf16)lo[3], (__bf16)hi[0], (__bf16)hi[1], (__bf16)hi[2], (__bf16)hi[3]};
}

__device__ inline f4 load_f4(const void *p) { return *reinterpret_cast<const f4 *>(p); }
__device__ inline f4 splat(float v) { return f4{v, v, v, v}; }

// acc[e] += W(fragment) . act[e] over one chunk (f32: act[e][0] is the chunk's tile, 4 MFMAs; bf16: act[e][0..1], one MFMA).
// TRANSPOSED: acc[e] += act[e]^T . W^T instead, the activation as the A operand and the same fragment as the B operand.
template <bool BF16, int E, bool TRANSPOSED = false>
__device__ inline void chunk_mma(const unsigned char *frag, const f4 (&act)[E][2], f4 (&acc)[E])
{
    const f4 a = load_f4(frag);
    if constexpr (BF16) {
        const bf16x8 w = __builtin_bit_cast(bf16x8, a);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const bf16x8 x = to_bf16x8(act[e][0], act[e][1]);
            acc[e] = TRANSPOSED ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, w, acc[e], 0, 0, 0)
                                : __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, x, acc[e], 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int e = 0; e < E; ++e)
                acc[e] = TRANSPOSED ? __builtin_amdgcn_mfma_f32_16x16x4f32(act[e][0][r], a[r], acc[e], 0, 0, 0)
                                    : __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], act[e][0][r], acc[e], 0, 0, 0);
    }
}

// acc[e] += (row tile o of the matrix at `mat`, K = 64) . x[e]  (x: the four feature tiles of each board)
template <bool BF16, bool TRANSPOSED = false>
__device__ inline void project64(const unsigned char *mat, int o, int lane, const f4 (&x)[kE][4], f4 (&acc)[kE])
{
    constexpr int TPC = BF16 ? 2 : 1, C = 4 / TPC;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        f4 in[kE][2];
#pragma unroll
        for (int e = 0; e < kE; ++e) {
            in[e][0] = x[e][TPC * c];
            in[e][1] = x[e][TPC * c + TPC - 1];
        }
        chunk_mma<BF16, kE, TRANSPOSED>(mat + ((size_t)(o * C + c) * 64 + lane) * 16, in, acc);
    }
}

__device__ inline float lanes_sum(float v)           // over the four lanes c, c + 16, c + 32, c + 48, the same on all four
{
    v += __shfl_xor(v, 16);
    return v + __shfl_xor(v, 32);
}

__device__ inline float lanes_max(float v)
{
    v = fmaxf(v, __shfl_xor(v, 16));
    return fmaxf(v, __shfl_xor(v, 32));
}

// x = LayerNorm(x + y) over the 64 features of every (board, token) column; np = weight[64] bias[64], biased variance
__device__ inline void add_norm(f4 (&x)[kE][4], const f4 (&y)[kE][4], const float *np, float eps, int g)
{
    f4 w[4], b[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        w[t] = load_f4(np + 16 * t + 4 * g);
        b[t] = load_f4(np + kD + 16 * t + 4 * g);
    }
#pragma unroll
    for (int e = 0; e < kE; ++e) {
        float s = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            x[e][t] = x[e][t] + y[e][t];
            s += (x[e][t][0] + x[e][t][1]) + (x[e][t][2] + x[e][t][3]);
        }
        const float mean = lanes_sum(s) / (float)kD;
        float q = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            x[e][t] = x[e][t] - splat(mean);
            const f4 d2 = x[e][t] * x[e][t];
            q += (d2[0] + d2[1]) + (d2[2] + d2[3]);
        }
        const float rstd = 1.0f / sqrtf(lanes_sum(q) / (float)kD + eps);
#pragma unroll
        for (int t = 0; t < 4; ++t) x[e][t] = x[e][t] * splat(rstd) * w[t] + b[t];
    }
}

// nn.Softmax(dim=-1) of one board's four logits: exp(z - max) / sum, in f32
__device__ __forceinline__ float4 softmax4(f4 z)
{
    const float m = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
    const float e0 = expf(z[0] - m), e1 = expf(z[1] - m), e2 = expf(z[2] - m), e3 = expf(z[3] - m);
    const float sum = ((e0 + e1) + e2) + e3;
    return make_float4(e0 / sum, e1 / sum, e2 / sum, e3 / sum);
}

// out += (row tile o of the matrix at `mat`, K = 16 * KT) . act, the activation of the 16 boards read from LDS rows of
// `stride` floats ([board][k]); k runs over KT tiles of 16, tile t at offset tile_ofs(t) within a row
template <bool BF16, int KT, class Ofs>
__device__ inline void dense_lds(const unsigned char *mat, int o, int lane, const float *act, int stride, Ofs tile_ofs, f4 &out)
{
    constexpr int TPC = BF16 ? 2 : 1, C = KT / TPC;
    const float *row = act + (lane & 15) * stride + 4 * (lane >> 4);
    f4 acc[1] = {out};
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
        f4 in[1][2];
        in[0][0] = load_f4(row + tile_ofs(TPC * c));
        in[0][1] = load_f4(row + tile_ofs(TPC * c + TPC - 1));
        chunk_mma<BF16, 1>(mat + ((size_t)(o * C + c) * 64 + lane) * 16, in, acc);
    }
    out = acc[0];
}

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

    // embedding: x[f][token] = w[f] * (code / 15) + b[f]; boards past n read as empty
    f4 x[kE][4];
    {
        f4 ew[4], eb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            ew[t] = load_f4(P + 16 * t + 4 * g);
            eb[t] = load_f4(P + kD + 16 * t + 4 * g);
        }
#pragma unroll
        for (int e = 0; e < kE; ++e) {
            const size_t env = env0 + (size_t)(kE * wave + e);
            const float v = (float)(env < n ? boards[env * 16 + col] : (uint8_t)0) / 15.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t) x[e][t] = ew[t] * splat(v) + eb[t];
        }
    }

#pragma unroll 1
    for (int l = 0; l < layers; ++l) {
        const unsigned char *Wl = W + (size_t)l * lay.layer_frags() * kFrag;
        const float *Pl = P + 2 * kD + l * lay.layer_params();
        const float *in_b = Pl, *out_b = Pl + 3 * kD, *b1 = Pl + 4 * kD, *b2 = b1 + ff, *norms = b2 + kD;

        // self-attention, head by head; attn[e][h] = row tile h of the concatenated heads
        f4 attn[kE][4];
#pragma unroll
        for (int h = 0; h < kHeads; ++h) {
            f4 q[kE], k[kE], vt[kE];
            const f4 qb = load_f4(in_b + 16 * h + 4 * g), kb = load_f4(in_b + kD + 16 * h + 4 * g);
            const f4 vb = splat(in_b[2 * kD + 16 * h + col]);
#pragma unroll
            for (int e = 0; e < kE; ++e) { q[e] = qb; k[e] = kb; vt[e] = vb; }
            project64<BF16>(Wl, h, lane, x, q);
            project64<BF16>(Wl, 4 + h, lane, x, k);
            project64<BF16, true>(Wl, 8 + h, lane, x, vt);
#pragma unroll
            for (int e = 0; e < kE; ++e) {
                f4 s = splat(0.0f);
#pragma unroll
                for (int r = 0; r < 4; ++r) s = __builtin_amdgcn_mfma_f32_16x16x4f32(k[e][r], q[e][r], s, 0, 0, 0);
                s = s * splat(0.25f);                                           // 1 / sqrt(head_dim)
                const float m = lanes_max(fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3])));
                f4 p{expf(s[0] - m), expf(s[1] - m), expf(s[2] - m), expf(s[3] - m)};
                const float sum = lanes_sum((p[0] + p[1]) + (p[2] + p[3]));
                p = p / splat(sum);
                f4 o = splat(0.0f);
#pragma unroll
                for (int r = 0; r < 4; ++r) o = __builtin_amdgcn_mfma_f32_16x16x4f32(vt[e][r], p[r], o, 0, 0, 0);
                attn[e][h] = o;
            }
        }

        // x = norm1(x + out_proj(attn))
        {
            f4 y[kE][4];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                f4 acc[kE];
                const f4 b = load_f4(out_b + 16 * o + 4 * g);
#pragma unroll
                for (int e = 0; e < kE; ++e) acc[e] = b;
                project64<BF16>(Wl + lay.out_proj() * kFrag, o, lane, attn, acc);
#pragma unroll
                for (int e = 0; e < kE; ++e) y[e][o] = acc[e];
            }
            add_norm(x, y, norms, norms[4 * kD], g);
        }

        // x = norm2(x + W2 relu(W1 x + b1) + b2), 32 features of the hidden layer at a time
        {
            const unsigned char *W1 = Wl + lay.w1() * kFrag, *W2 = Wl + lay.w2() * kFrag;
            constexpr int CPS = BF16 ? 1 : 2;                                   // W2 chunks per 32-feature slice
            const int c2 = ff / (32 / CPS);                                     // W2 chunks per row tile
            f4 y[kE][4];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const f4 b = load_f4(b2 + 16 * o + 4 * g);
#pragma unroll
                for (int e = 0; e < kE; ++e) y[e][o] = b;
            }
#pragma unroll 1
            for (int s = 0; s < ff / 32; ++s) {
                f4 h1[kE][2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    f4 acc[kE];
                    const f4 b = load_f4(b1 + 32 * s + 16 * t + 4 * g);
#pragma unroll
                    for (int e = 0; e < kE; ++e) acc[e] = b;
                    project64<BF16>(W1, 2 * s + t, lane, x, acc);
#pragma unroll
                    for (int e = 0; e < kE; ++e) h1[e][t] = relu(acc[e]);
                }
#pragma unroll
                for (int t = 0; t < CPS; ++t) {
                    const int c = CPS * s + t;
#pragma unroll
                    for (int o = 0; o < 4; ++o) {
                        f4 in[kE][2], acc[kE];
#pragma unroll
                        for (int e = 0; e < kE; ++e) {
                            in[e][0] = h1[e][t];
                            in[e][1] = h1[e][1];
                            acc[e] = y[e][o];
                        }
                        chunk_mma<BF16, kE>(W2 + ((size_t)(o * c2 + c) * 64 + lane) * 16, in, acc);
#pragma unroll
                        for (int e = 0; e < kE; ++e) y[e][o] = acc[e];
                    }
                }
            }
            add_norm(x, y, norms + 2 * kD, norms[4 * kD + 1], g);
        }
    }

    // flatten: lds[board][token][feature] (the block's 16 boards)
#pragma unroll
    for (int e = 0; e < kE; ++e)
#pragma unroll
        for (int t = 0; t < 4; ++t)
            *reinterpret_cast<f4 *>(lds + (kE * wave + e) * kBoardStride + col * kTokStride + 16 * t + 4 * g) = x[e][t];
    __syncthreads();

    // fc1: row tiles 2 wave, 2 wave + 1 for the 16 boards; flat k = 64 token + feature, tile t of 16 = token t / 4
    const float *Pt = P + 2 * kD + layers * lay.layer_params();
    f4 h1[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int o = 2 * wave + q;
        h1[q] = load_f4(Pt + 16 * o + 4 * g);
        dense_lds<BF16, kFlat / 16>(W + lay.fc1() * kFrag, o, lane, lds, kBoardStride,
                                    [](int t) { return (t >> 2) * kTokStride + 16 * (t & 3); }, h1[q]);
    }
    __syncthreads();                                                            // every wavefront is done with the encoder outputs
    float *a1 = lds, *a2 = lds + 16 * kH1Stride;
#pragma unroll
    for (int q = 0; q < 2; ++q) *reinterpret_cast<f4 *>(a1 + col * kH1Stride + 16 * (2 * wave + q) + 4 * g) = relu(h1[q]);
    __syncthreads();

    // fc2: row tile `wave`
    f4 h2 = load_f4(Pt + kFc1 + 16 * wave + 4 * g);
    dense_lds<BF16, kFc1 / 16>(W + lay.fc2() * kFrag, wave, lane, a1, kH1Stride, [](int t) { return 16 * t; }, h2);
    *reinterpret_cast<f4 *>(a2 + col * kH2Stride + 16 * wave + 4 * g) = relu(h2);
    __syncthreads();
    if (wave != 0) return;

    // heads: rows 0..3 the actor's logits (lanes 0..15), row 4 the critic's value (register 0 of lanes 16..31)
    f4 z = load_f4(Pt + kFc1 + kFc2 + 4 * g);
    dense_lds<BF16, kFc2 / 16>(W + lay.heads() * kFrag, 0, lane, a2, kH2Stride, [](int t) { return 16 * t; }, z);
    const size_t env = env0 + col;
    if (env >= n) return;
    if (g == 0) probs[env] = softmax4(z);
    else if (g == 1 && value) value[env] = z[0];
}

bool good_shape(int dim_ff, int n_layers) { return dim_ff >= 32 && dim_ff % 32 == 0 && dim_ff <= 65536 && n_layers >= 1 && n_layers <= 64; }
bool good_precision(int p) { return p == G2048_POLICY_F32 || p == G2048_POLICY_BF16; }

}  // namespace

extern "C" {

size_t g2048_tpolicy_packed_bytes(int precision, int dim_ff, int n_layers)
{
    if (!good_precision(precision) || !good_shape(dim_ff, n_layers)) return 0;
    return Layout(precision == G2048_POLICY_BF16, dim_ff, n_layers).bytes();
}

int g2048_tpolicy_pack(const float *plain_f32, int dim_ff, int n_layers, int precision, void *packed_out, void *stream)
{
    if (!plain_f32 || !packed_out) return fail(G2048_ERR_ARG, "g2048_tpolicy_pack: null pointer");
    if (!aligned(plain_f32, 4) || !aligned(packed_out, 16)) return fail(G2048_ERR_ARG, "g2048_tpolicy_pack: misaligned pointer");
    if (!good_precision(precision)) return fail(G2048_ERR_ARG, "g2048_tpolicy_pack: unknown precision");
    if (!good_shape(dim_ff, n_layers))
        return fail(G2048_ERR_ARG, "g2048_tpolicy_pack: dim_ff must be a multiple of 32 (32 .. 65536) and n_layers 1 .. 64");
    const bool bf16 = precision == G2048_POLICY_BF16;
    const Layout lay(bf16, dim_ff, n_layers);
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto *out = static_cast<unsigned char *>(packed_out);
    // one launch per matrix: `rows` (a over b) x K into the fragments from index `frag`
    auto matrix = [&](const float *a, int rows_a, const float *b, int rows_b, int K, size_t frag) {
        const unsigned words = (unsigned)(((rows_a + rows_b + 15) / 16) * lay.chunks(K)) * 256u;
        with_bool(bf16, [&](auto BF16) {
            hipLaunchKernelGGL(tpolicy_pack_matrix_kernel<decltype(BF16)::value>, dim3(words / 256u), dim3(256), 0, s, a, rows_a, b, rows_b, K,
                               words, reinterpret_cast<uint32_t *>(out + frag * kFrag));
        });
    };
    for (int l = 0; l < n_layers; ++l) {
        const float *p = plain_f32 + kPlainLayer0 + (size_t)l * pl_layer(dim_ff);
        const size_t f = (size_t)l * lay.layer_frags();
        matrix(p + kPlInW, 3 * kD, nullptr, 0, kD, f);
        matrix(p + kPlOutW, kD, nullptr, 0, kD, f + lay.out_proj());
        matrix(p + kPlW1, dim_ff, nullptr, 0, kD, f + lay.w1());
        matrix(p + pl_w2(dim_ff), kD, nullptr, 0, dim_ff, f + lay.w2());
    }
    const float *t = plain_f32 + kPlainLayer0 + (size_t)n_layers * pl_layer(dim_ff);
    matrix(t + kPlFc1W, kFc1, nullptr, 0, kFlat, lay.fc1());
    matrix(t + kPlFc2W, kFc2, nullptr, 0, kFc1, lay.fc2());
    matrix(t + kPlActW, 4, t + kPlCriW, 1, kD, lay.heads());
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
    if (opts != G2048_POLICY_F32 && opts != G2048_POLICY_BF16) return fail(G2048_ERR_ARG, "g2048_tpolicy_forward: unknown opts (precision)");
    if (!good_shape(dim_ff, n_layers))
        return fail(G2048_ERR_ARG, "g2048_tpolicy_forward: dim_ff must be a multiple of 32 (32 .. 65536) and n_layers 1 .. 64");
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

}  // extern "C"
