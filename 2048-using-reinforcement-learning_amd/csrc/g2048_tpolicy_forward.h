// g2048_tpolicy_forward.h -- the parts of the transformer policy's forward pass (g2048_tpolicy.hip has the description) that more
// than one kernel file expands: the packed blob's layout, the block geometry and its LDS strides, the encoder's helpers and the
// forward in three macros. Included by g2048_tpolicy.hip (the forward kernel, the game-playing kernel) and by
// g2048_tpolicy_collect.hip (the transformer policy's experience collector, a library of its own); both expand exactly this
// text, so a board's probabilities and value are the same bits in every one of them. Compile with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "g2048_mfma.h"
#include "g2048_tpolicy_layout.h"

namespace {

using namespace g2048;

// ------------------------------------------------------------------------------------------------ shapes and layouts --
// the shapes (kD, kHeads, kTok, kFc1, kFc2, kFlat) and the plain f32 layout (kPl*, pl_*): g2048_tpolicy_layout.h

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

// ---------------------------------------------------------------------------------------------------------- forward --
constexpr int kWaves = 4, kE = 4;                    // wavefronts per block, boards per wavefront: 16 boards per block
constexpr int kTokStride = kD + 4;                   // LDS strides in floats: + 4 spreads the 16-byte accesses over the banks
constexpr int kBoardStride = kTok * kTokStride + 4;
constexpr int kH1Stride = kFc1 + 4, kH2Stride = kFc2 + 4;
constexpr int kLdsFloats = 16 * kBoardStride;
static_assert(16 * kH1Stride + 16 * kH2Stride <= kLdsFloats, "the fc1 / fc2 outputs reuse the encoder-output buffer");

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

// The forward pass in three pieces that tpolicy_forward_kernel and the game-playing kernel (tpolicy_play_kernel, below) share.
// Both expand exactly this text, and a board's outputs do not depend on the column, the tile or the block it sits in, so the
// two kernels give bit-identical probabilities for the same board and blob. Macros, not functions, for the reason
// POLICY_LAYERS_ of g2048_policy.hip is one: expanded in place, the forward kernel's code object is byte for byte what it was
// before the pieces were named (profiles/r09_tpolicy_device_code_diff.txt). They use the kernel's names: W, P, lay, ff, layers,
// lds, lane, wave, g, col.
//   TPOLICY_ENCODER_  embedding and the encoder layers in registers, then the wavefront's four boards to lds[board][token][feature];
//   TPOLICY_DENSE_    barrier, fc1, fc2 through LDS, barrier (every wavefront must reach it);
//   TPOLICY_HEADS_    the head tile z (wavefront 0 only): lanes 0..15 hold the logits of board `col`, lanes 16..31 the value.
#define TPOLICY_ENCODER_(BF16, CODE) \
    /* embedding: x[f][token] = w[f] * (code / 15) + b[f]; CODE = the code of cell `col` of the wavefront's board e */ \
    f4 x[kE][4]; \
    { \
        f4 ew[4], eb[4]; \
_Pragma("unroll") \
        for (int t = 0; t < 4; ++t) { \
            ew[t] = load_f4(P + 16 * t + 4 * g); \
            eb[t] = load_f4(P + kD + 16 * t + 4 * g); \
        } \
_Pragma("unroll") \
        for (int e = 0; e < kE; ++e) { \
            const float v = (float)(CODE) / 15.0f; \
_Pragma("unroll") \
            for (int t = 0; t < 4; ++t) x[e][t] = ew[t] * splat(v) + eb[t]; \
        } \
    } \
 \
_Pragma("unroll 1") \
    for (int l = 0; l < layers; ++l) { \
        const unsigned char *Wl = W + (size_t)l * lay.layer_frags() * kFrag; \
        const float *Pl = P + 2 * kD + l * lay.layer_params(); \
        const float *in_b = Pl, *out_b = Pl + 3 * kD, *b1 = Pl + 4 * kD, *b2 = b1 + ff, *norms = b2 + kD; \
 \
        /* self-attention, head by head; attn[e][h] = row tile h of the concatenated heads */ \
        f4 attn[kE][4]; \
_Pragma("unroll") \
        for (int h = 0; h < kHeads; ++h) { \
            f4 q[kE], k[kE], vt[kE]; \
            const f4 qb = load_f4(in_b + 16 * h + 4 * g), kb = load_f4(in_b + kD + 16 * h + 4 * g); \
            const f4 vb = splat(in_b[2 * kD + 16 * h + col]); \
_Pragma("unroll") \
            for (int e = 0; e < kE; ++e) { q[e] = qb; k[e] = kb; vt[e] = vb; } \
            project64<BF16>(Wl, h, lane, x, q); \
            project64<BF16>(Wl, 4 + h, lane, x, k); \
            project64<BF16, true>(Wl, 8 + h, lane, x, vt); \
_Pragma("unroll") \
            for (int e = 0; e < kE; ++e) { \
                f4 s = splat(0.0f); \
_Pragma("unroll") \
                for (int r = 0; r < 4; ++r) s = __builtin_amdgcn_mfma_f32_16x16x4f32(k[e][r], q[e][r], s, 0, 0, 0); \
                s = s * splat(0.25f);  /* 1 / sqrt(head_dim) */ \
                const float m = lanes_max(fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]))); \
                f4 p{expf(s[0] - m), expf(s[1] - m), expf(s[2] - m), expf(s[3] - m)}; \
                const float sum = lanes_sum((p[0] + p[1]) + (p[2] + p[3])); \
                p = p / splat(sum); \
                f4 o = splat(0.0f); \
_Pragma("unroll") \
                for (int r = 0; r < 4; ++r) o = __builtin_amdgcn_mfma_f32_16x16x4f32(vt[e][r], p[r], o, 0, 0, 0); \
                attn[e][h] = o; \
            } \
        } \
 \
        /* x = norm1(x + out_proj(attn)) */ \
        { \
            f4 y[kE][4]; \
_Pragma("unroll") \
            for (int o = 0; o < 4; ++o) { \
                f4 acc[kE]; \
                const f4 b = load_f4(out_b + 16 * o + 4 * g); \
_Pragma("unroll") \
                for (int e = 0; e < kE; ++e) acc[e] = b; \
                project64<BF16>(Wl + lay.out_proj() * kFrag, o, lane, attn, acc); \
_Pragma("unroll") \
                for (int e = 0; e < kE; ++e) y[e][o] = acc[e]; \
            } \
            add_norm(x, y, norms, norms[4 * kD], g); \
        } \
 \
        /* x = norm2(x + W2 relu(W1 x + b1) + b2), 32 features of the hidden layer at a time */ \
        { \
            const unsigned char *W1 = Wl + lay.w1() * kFrag, *W2 = Wl + lay.w2() * kFrag; \
            constexpr int CPS = BF16 ? 1 : 2;  /* W2 chunks per 32-feature slice */ \
            const int c2 = ff / (32 / CPS);  /* W2 chunks per row tile */ \
            f4 y[kE][4]; \
_Pragma("unroll") \
            for (int o = 0; o < 4; ++o) { \
                const f4 b = load_f4(b2 + 16 * o + 4 * g); \
_Pragma("unroll") \
                for (int e = 0; e < kE; ++e) y[e][o] = b; \
            } \
_Pragma("unroll 1") \
            for (int s = 0; s < ff / 32; ++s) { \
                f4 h1[kE][2]; \
_Pragma("unroll") \
                for (int t = 0; t < 2; ++t) { \
                    f4 acc[kE]; \
                    const f4 b = load_f4(b1 + 32 * s + 16 * t + 4 * g); \
_Pragma("unroll") \
                    for (int e = 0; e < kE; ++e) acc[e] = b; \
                    project64<BF16>(W1, 2 * s + t, lane, x, acc); \
_Pragma("unroll") \
                    for (int e = 0; e < kE; ++e) h1[e][t] = relu(acc[e]); \
                } \
_Pragma("unroll") \
                for (int t = 0; t < CPS; ++t) { \
                    const int c = CPS * s + t; \
_Pragma("unroll") \
                    for (int o = 0; o < 4; ++o) { \
                        f4 in[kE][2], acc[kE]; \
_Pragma("unroll") \
                        for (int e = 0; e < kE; ++e) { \
                            in[e][0] = h1[e][t]; \
                            in[e][1] = h1[e][1]; \
                            acc[e] = y[e][o]; \
                        } \
                        chunk_mma<BF16, kE>(W2 + ((size_t)(o * c2 + c) * 64 + lane) * 16, in, acc); \
_Pragma("unroll") \
                        for (int e = 0; e < kE; ++e) y[e][o] = acc[e]; \
                    } \
                } \
            } \
            add_norm(x, y, norms + 2 * kD, norms[4 * kD + 1], g); \
        } \
    } \
 \
    /* flatten: lds[board][token][feature] (the block's 16 boards) */ \
_Pragma("unroll") \
    for (int e = 0; e < kE; ++e) \
_Pragma("unroll") \
        for (int t = 0; t < 4; ++t) \
            *reinterpret_cast<f4 *>(lds + (kE * wave + e) * kBoardStride + col * kTokStride + 16 * t + 4 * g) = x[e][t];

#define TPOLICY_DENSE_(BF16) \
    __syncthreads(); \
 \
    /* fc1: row tiles 2 wave, 2 wave + 1 for the 16 boards; flat k = 64 token + feature, tile t of 16 = token t / 4 */ \
    const float *Pt = P + 2 * kD + layers * lay.layer_params(); \
    f4 h1[2]; \
_Pragma("unroll") \
    for (int q = 0; q < 2; ++q) { \
        const int o = 2 * wave + q; \
        h1[q] = load_f4(Pt + 16 * o + 4 * g); \
        dense_lds<BF16, kFlat / 16>(W + lay.fc1() * kFrag, o, lane, lds, kBoardStride, \
                                    [](int t) { return (t >> 2) * kTokStride + 16 * (t & 3); }, h1[q]); \
    } \
    __syncthreads();  /* every wavefront is done with the encoder outputs */ \
    float *a1 = lds, *a2 = lds + 16 * kH1Stride; \
_Pragma("unroll") \
    for (int q = 0; q < 2; ++q) *reinterpret_cast<f4 *>(a1 + col * kH1Stride + 16 * (2 * wave + q) + 4 * g) = relu(h1[q]); \
    __syncthreads(); \
 \
    /* fc2: row tile `wave` */ \
    f4 h2 = load_f4(Pt + kFc1 + 16 * wave + 4 * g); \
    dense_lds<BF16, kFc1 / 16>(W + lay.fc2() * kFrag, wave, lane, a1, kH1Stride, [](int t) { return 16 * t; }, h2); \
    *reinterpret_cast<f4 *>(a2 + col * kH2Stride + 16 * wave + 4 * g) = relu(h2); \
    __syncthreads();

#define TPOLICY_HEADS_(BF16) \
    /* heads: rows 0..3 the actor's logits (lanes 0..15), row 4 the critic's value (register 0 of lanes 16..31) */ \
    f4 z = load_f4(Pt + kFc1 + kFc2 + 4 * g); \
    dense_lds<BF16, kFc2 / 16>(W + lay.heads() * kFrag, 0, lane, a2, kH2Stride, [](int t) { return 16 * t; }, z);

}  // namespace
