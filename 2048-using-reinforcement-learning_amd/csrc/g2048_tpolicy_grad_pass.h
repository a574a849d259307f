// g2048_tpolicy_grad_pass.h -- the transformer policy's loss and gradient pass: its workspace, its kernels and the one launch
// sequence, shared by g2048_tpolicy_grad.hip (libg2048_tlearn_hip.so, eval mode) and g2048_tpolicy_train.hip
// (libg2048_ttrain_hip.so, the training-mode pass with the encoder's live dropout) and included by nothing else; every kernel is
// per translation unit. What the pass computes, what it keeps and its rules are in g2048_tpolicy_grad.hip's head comment.
//
// The kernels a dropout site touches are templates on a trailing pack (`MaybeDrop...`, empty or one QDrop of g2048_qnet_drop.h),
// `if constexpr (sizeof...(MaybeDrop) != 0)` round the dropout lines: the learner library instantiates them without the pack, the
// training library also with a QDrop. tg_pass<kDrop> is the launch sequence; with kDrop false it names no QDrop instantiation, so
// the learner library's code object holds none. A site with p == 0 is not hashed: its launch is the instantiation without a QDrop.
// Where the masks go (site s of layer L, element e; the rule and the sites: include/g2048_ttrain.h):
//   forward   s = 0  tg_attention_kernel: p x m is the B operand of V^T . P, the maximum and the sum are of the unmasked scores, and
//                    the UNMASKED probabilities are kept
//             s = 1  tg_linear_kernel<false> (out_proj): (X W^T + b) x m + res      s = 3  the same on linear2
//             s = 2  tg_linear_kernel<true> (linear1): relu(..) x m; the backward's recomputation of the hidden layer passes the
//                    same QDrop and is bit for bit the forward's
//   backward  s = 3, 1  the gradient ds leaving the LayerNorm backward goes to the residual path as it is and x m (qt_scale_kernel,
//                    one elementwise launch into the one extra array dsm [16 n][64]) into the dW / dX products of linear2 / out_proj
//             s = 2  qg_dx_kernel<QDrop> through linear2: x m next to the ReLU mask; linear2's dW reads the dropped hidden layer
//             s = 0  tg_attention_bwd_kernel, with M the multipliers and P the kept unmasked probabilities:
//                    dV = (P o M)^T dO, dP = M o (dO V^T), D = rowsum(dP o P), dS = P o (dP - D). Both orientations of P and dP
//                    are hashed with the element index of the orientation they are in, eight draws a lane. No mask is stored.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "../../include/g2048_tlearn.h"
#include "g2048_grad_products.h"
#include "g2048_host.h"
#include "g2048_mfma.h"
#include "g2048_ppo_head.h"
#include "g2048_qnet_drop.h"
#include "g2048_tpolicy_bf16.h"
#include "g2048_tpolicy_layout.h"

namespace {

using namespace g2048;

constexpr int kQkv = 3 * kD, kHead = kD / kHeads;
constexpr int kRowChunk = 512;                       // rows of one partial weight-gradient tile
constexpr int kColRows = 64;                         // rows of one partial column sum (LayerNorm parameters, embedding)
static_assert(kHead == 16 && kTok == 16, "the attention kernels are three 16 x 16 x 16 products");

inline size_t row_chunks(size_t rows) { return (rows + kRowChunk - 1) / kRowChunk; }
inline size_t col_chunks(size_t rows) { return (rows + kColRows - 1) / kColRows; }

// workspace, in floats; T = 16 n tokens. Every array's size is a multiple of four floats, so every array is 16-byte aligned.
// half (the bf16 feed-forward mode, g2048_tbf16.h): h and dh hold bf16, two elements a float, and wb follows the training array.
struct Workspace {
    size_t n, T, ff, layers;
    bool half;
    Workspace(size_t n_, int dim_ff, int n_layers, bool half_ = false)
        : n(n_), T(16 * n_), ff((size_t)dim_ff), layers((size_t)n_layers), half(half_) {}
    size_t hidden() const { return half ? T * ff / 2 : T * ff; }                      // floats of h, and of dh
    // kept by the forward
    size_t x(size_t l) const { return l * T * kD; }                                   // l = 0 .. layers: layer l's input
    size_t layer(size_t l) const { return x(layers + 1) + l * T * (kQkv + 5 * kD + 4); }
    size_t qkv(size_t l) const { return layer(l); }
    size_t prob(size_t l) const { return qkv(l) + T * kQkv; }                         // [board][head][query][key]
    size_t att(size_t l) const { return prob(l) + T * kD; }
    size_t pre1(size_t l) const { return att(l) + T * kD; }
    size_t x1(size_t l) const { return pre1(l) + T * kD; }
    size_t pre2(size_t l) const { return x1(l) + T * kD; }
    size_t stat(size_t l) const { return pre2(l) + T * kD; }                          // [2][T][2]: norm1's, norm2's (mean, rstd)
    size_t h() const { return layer(layers); }                                        // [T][dim_ff], one for all layers
    size_t a1() const { return h() + hidden(); }
    size_t a2() const { return a1() + n * kFc1; }
    // the backward's own
    size_t dz() const { return a2() + n * kFc2; }                                     // [n][8]: logits 0..3, value 4
    size_t terms() const { return dz() + n * 8; }                                     // [3][4 n / 4 up]: actor, value, entropy
    size_t tstride() const { return (n + 3) / 4 * 4; }
    size_t d2() const { return terms() + 3 * tstride(); }
    size_t d1() const { return d2() + n * kFc2; }
    size_t ga() const { return d1() + n * kFc1; }
    size_t gb() const { return ga() + T * kD; }
    size_t ds() const { return gb() + T * kD; }
    size_t datt() const { return ds() + T * kD; }
    size_t dqkv() const { return datt() + T * kD; }
    size_t dh() const { return dqkv() + T * kQkv; }
    size_t wpart() const { return dh() + hidden(); }                                    // [row chunks][the largest M K]
    size_t wmax() const { return (size_t)kD * (ff > (size_t)kQkv ? ff : (size_t)kQkv); }
    size_t bpart() const { return wpart() + row_chunks(T) * wmax(); }                 // [row chunks][the largest M]
    size_t bmax() const { return ff > (size_t)kQkv ? ff : (size_t)kQkv; }
    size_t cpart() const { return bpart() + row_chunks(T) * bmax(); }                 // [col chunks][128]
    size_t floats() const { return cpart() + col_chunks(T) * 2 * kD; }
    // the training-mode pass's one array more: ds x the multipliers of site 1 or 3
    size_t dsm() const { return floats(); }
    size_t train_floats() const { return dsm() + T * kD; }
    // the bf16 mode's: per layer the packed bf16 weights W1 [ff][64], its transpose [64][ff], W2 [64][ff], its transpose [ff][64]
    size_t wb() const { return train_floats(); }
    size_t bf16_floats() const { return wb() + layers * 4 * (size_t)kD * ff / 2; }
};

__device__ inline float sum16(float v)               // over the 16 lanes that share lane >> 4, the same on all of them
{
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) v += __shfl_xor(v, d);
    return v;
}

// -------------------------------------------------------------------------------------------------------- embedding --
// x[token][j] = emb.w[j] . (code / 15) + emb.b[j]; a thread four features of one token
__global__ __launch_bounds__(256) void tg_embed_kernel(const uint8_t *__restrict__ boards, const float *__restrict__ P, float *__restrict__ X,
                                                        int tokens)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x), t = i >> 4, j = i & 15;
    if (t >= tokens) return;
    const float v = (float)boards[t] / 15.0f;
    *reinterpret_cast<f4 *>(X + (size_t)t * kD + 4 * j) = load_w(P + kPlainEmb + 4 * j) * splat(v) + load_w(P + kPlainEmb + kD + 4 * j);
}

// its backward: part[chunk][j] = the chunk's sum of G[token][j] x_token, part[chunk][64 + j] of G[token][j], over kColRows tokens:
// thread (slot, j) adds its four tokens slot, slot + 16, .. in order, the 16 slots are combined pairwise
__device__ inline void slots_to_part(float (&red)[16][2 * kD], float *__restrict__ part)
{
    __syncthreads();
    if (threadIdx.x < 2 * kD) {
        float r[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) r[i] = red[i][threadIdx.x];
#pragma unroll
        for (int w = 8; w > 0; w >>= 1)
#pragma unroll
            for (int i = 0; i < w; ++i) r[i] = r[2 * i] + r[2 * i + 1];
        part[(size_t)blockIdx.x * (2 * kD) + threadIdx.x] = r[0];
    }
}

__global__ __launch_bounds__(256) void tg_embed_bwd_kernel(const float *__restrict__ G, const uint8_t *__restrict__ boards,
                                                            float *__restrict__ part, int tokens)
{
    __shared__ __attribute__((aligned(16))) float red[16][2 * kD];
    const int slot = threadIdx.x >> 4, j = threadIdx.x & 15;
    f4 aw = splat(0.0f), ab = splat(0.0f);
    for (int p = 0; p < kColRows / 16; ++p) {
        const int t = (int)blockIdx.x * kColRows + 16 * p + slot;
        if (t < tokens) {
            const f4 g = load_f4(G + (size_t)t * kD + 4 * j);
            aw = aw + g * splat((float)boards[t] / 15.0f);
            ab = ab + g;
        }
    }
    *reinterpret_cast<f4 *>(&red[slot][4 * j]) = aw;
    *reinterpret_cast<f4 *>(&red[slot][kD + 4 * j]) = ab;
    slots_to_part(red, part);
}

// ----------------------------------------------------------------------------------------------------------- linear --
// Y [n][M] = act(X [n][K] W^T + b (+ RES)): the tile is D[feature 16 o + 4 g + r][row col]; lane (col, g): the A operand
// W[16 o + col][16 c + 4 g ..], the B operand X[row][16 c + 4 g ..], four MFMAs a chunk of 16; K is a multiple of 32. Chunk c of a
// group of eight accumulates into acc[c] (chunks_product, g2048_mfma.h), combined pairwise: the order is fixed. Four wavefronts a
// block = four feature tiles of one row tile; grid (M / 64 up, row tiles).
// With a QDrop the product is a dropout site's, element row M + feature (at most 16,384 x 65,536 = 2^30): sites 1 and 3 (no ReLU)
// (X W^T + b) x m + RES, site 2 relu(..) x m.
template <bool RELU, class... MaybeDrop>
__global__ __launch_bounds__(256) void tg_linear_kernel(const float *__restrict__ X, int K, const float *__restrict__ W,
                                                         const float *__restrict__ bias, const float *__restrict__ res, float *__restrict__ Y,
                                                         int M, int n, MaybeDrop... drop)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const int o = (int)blockIdx.x * 4 + wave;
    if (16 * o >= M) return;
    const int row = (int)blockIdx.y * 16 + col;
    const bool live = row < n;
    const float *wrow = W + (size_t)(16 * o + col) * K + 4 * g, *xrow = X + (size_t)row * K + 4 * g;
    f4 acc[8] = {load_w(bias + 16 * o + 4 * g), splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f), splat(0.0f)};
    int k = 0;
    for (; k + 128 <= K; k += 128) chunks_product<8>(wrow + k, xrow + k, live, acc);
    for (; k < K; k += 32) chunks_product<2>(wrow + k, xrow + k, live, acc);
    if (!live) return;
    f4 v = sum8(acc);
    const size_t at = (size_t)row * M + 16 * o + 4 * g;
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
    *reinterpret_cast<f4 *>(Y + at) = v;
}

// -------------------------------------------------------------------------------------------------------- attention --
// A block a board, a wavefront a head. S[key 4 g + r][query col] = K . Q over the head's 16 features (A = K[key col][4 g ..],
// B = Q[query col][4 g ..]), / 4; softmax over the keys of a query: four registers and two cross-lane steps; the probabilities
// are, as they stand, the B operand of O[d 4 g + r][query col] = V^T . P (A = V[key 4 g + r][d col]). prob [board][head][query][key]
// keeps them for the backward. With a QDrop (site 0, element ((board 4 + head) 16 + query) 16 + key: prob's own index) the B operand
// is p x m, each lane hashing the four elements it holds; prob keeps the unmasked p.
template <class... MaybeDrop>
__global__ __launch_bounds__(256) void tg_attention_kernel(const float *__restrict__ qkv, float *__restrict__ att, float *__restrict__ prob,
                                                            MaybeDrop... drop)
{
    const int lane = threadIdx.x & 63, head = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const size_t tok0 = (size_t)blockIdx.x * kTok;
    const float *base = qkv + tok0 * kQkv + head * kHead;
    const f4 q = load_f4(base + (size_t)col * kQkv + 4 * g), k = load_f4(base + (size_t)col * kQkv + kD + 4 * g);
    f4 vt;
#pragma unroll
    for (int r = 0; r < 4; ++r) vt[r] = base[(size_t)(4 * g + r) * kQkv + 2 * kD + col];
    f4 s = splat(0.0f);
#pragma unroll
    for (int r = 0; r < 4; ++r) s = __builtin_amdgcn_mfma_f32_16x16x4f32(k[r], q[r], s, 0, 0, 0);
    s = s * splat(0.25f);                                                   // 1 / sqrt(head_dim)
    const float m = lanes_max(fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3])));
    f4 p{expf(s[0] - m), expf(s[1] - m), expf(s[2] - m), expf(s[3] - m)};
    const float sum = lanes_sum((p[0] + p[1]) + (p[2] + p[3]));
    p = p / splat(sum);
    f4 pm = p;
    if constexpr (sizeof...(MaybeDrop) != 0) {
        const size_t at = (((size_t)blockIdx.x * kHeads + head) * kTok + col) * kTok + 4 * g;
#pragma unroll
        for (int r = 0; r < 4; ++r) pm[r] *= qdrop_mult(drop..., (uint32_t)at + (uint32_t)r);
    }
    f4 o = splat(0.0f);
#pragma unroll
    for (int r = 0; r < 4; ++r) o = __builtin_amdgcn_mfma_f32_16x16x4f32(vt[r], pm[r], o, 0, 0, 0);
    *reinterpret_cast<f4 *>(att + (tok0 + col) * kD + head * kHead + 4 * g) = o;
    *reinterpret_cast<f4 *>(prob + (((size_t)blockIdx.x * kHeads + head) * kTok + col) * kTok + 4 * g) = p;
}

// Its backward, the same geometry. Both orientations of dP = dO V^T are one product each with the operands swapped:
//   dP[key 4 g + r][query col] (A = V[key col][4 g ..], B = dO[query col][4 g ..]) with P in the same layout gives the row sums
//   D[query col] = sum over the keys of dP o P and dS in the layout that is the B operand of dQ^T = K^T . dS;
//   dP[query 4 g + r][key col] (A = dO, B = V) with P[query 4 g + r][key col] and D of query 4 g + r (from the lane that holds it)
//   gives dS in the layout that is the B operand of dK^T = Q^T . dS, and P itself is the B operand of dV^T = dO^T . P.
// dS = P o (dP - D); dQ and dK carry the 1 / 4 of the scores. With a QDrop (site 0) and M the multipliers, P the kept unmasked
// probabilities: dP = M o (dO V^T) in both orientations, dV^T = dO^T . (P o M), D and dS as above; mq is M[query col][key 4 g + r],
// mk is M[query 4 g + r][key col], each hashed with its own element index.
template <class... MaybeDrop>
__global__ __launch_bounds__(256) void tg_attention_bwd_kernel(const float *__restrict__ qkv, const float *__restrict__ prob,
                                                                const float *__restrict__ datt, float *__restrict__ dqkv, MaybeDrop... drop)
{
    const int lane = threadIdx.x & 63, head = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const size_t tok0 = (size_t)blockIdx.x * kTok;
    const float *base = qkv + tok0 * kQkv + head * kHead, *dbase = datt + tok0 * kD + head * kHead;
    const float *pb = prob + ((size_t)blockIdx.x * kHeads + head) * kTok * kTok;
    const f4 v = load_f4(base + (size_t)col * kQkv + 2 * kD + 4 * g), dO = load_f4(dbase + (size_t)col * kD + 4 * g);
    const f4 pq = load_f4(pb + col * kTok + 4 * g);                         // P[query col][key 4 g + r]
    f4 kt, qt, dot, pk;                                                     // K, Q, dO of token 4 g + r at feature col; P[query 4 g + r][key col]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        kt[r] = base[(size_t)(4 * g + r) * kQkv + kD + col];
        qt[r] = base[(size_t)(4 * g + r) * kQkv + col];
        dot[r] = dbase[(size_t)(4 * g + r) * kD + col];
        pk[r] = pb[(4 * g + r) * kTok + col];
    }
    f4 dpq = splat(0.0f), dpk = splat(0.0f);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        dpq = __builtin_amdgcn_mfma_f32_16x16x4f32(v[r], dO[r], dpq, 0, 0, 0);
        dpk = __builtin_amdgcn_mfma_f32_16x16x4f32(dO[r], v[r], dpk, 0, 0, 0);
    }
    f4 pv = pk;                                                             // the B operand of dV^T: P o M
    if constexpr (sizeof...(MaybeDrop) != 0) {
        const uint32_t e0 = (uint32_t)(((size_t)blockIdx.x * kHeads + head) * kTok * kTok);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            dpq[r] *= qdrop_mult(drop..., e0 + (uint32_t)(col * kTok + 4 * g + r));
            const float mk = qdrop_mult(drop..., e0 + (uint32_t)((4 * g + r) * kTok + col));
            dpk[r] *= mk;
            pv[r] *= mk;
        }
    }
    const float D = lanes_sum(sum4(dpq * pq));                              // of query col, on every lane of that column
    f4 dsq, dsk;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        dsq[r] = pq[r] * (dpq[r] - D);
        dsk[r] = pk[r] * (dpk[r] - __shfl(D, 4 * g + r));
    }
    f4 dq = splat(0.0f), dk = splat(0.0f), dv = splat(0.0f);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        dq = __builtin_amdgcn_mfma_f32_16x16x4f32(kt[r], dsq[r], dq, 0, 0, 0);
        dk = __builtin_amdgcn_mfma_f32_16x16x4f32(qt[r], dsk[r], dk, 0, 0, 0);
        dv = __builtin_amdgcn_mfma_f32_16x16x4f32(dot[r], pv[r], dv, 0, 0, 0);
    }
    float *out = dqkv + (tok0 + col) * kQkv + head * kHead + 4 * g;
    *reinterpret_cast<f4 *>(out) = dq * splat(0.25f);
    *reinterpret_cast<f4 *>(out + kD) = dk * splat(0.25f);
    *reinterpret_cast<f4 *>(out + 2 * kD) = dv;
}

// -------------------------------------------------------------------------------------------------------- LayerNorm --
// Y = LayerNorm(S) over the 64 features of a token, biased variance; norm: weight[64] bias[64]; eps: one float on the device;
// stat[token] = (mean, rstd), kept for the backward. 16 lanes a token, a block 16 tokens.
__global__ __launch_bounds__(256) void tg_ln_kernel(const float *__restrict__ S, const float *__restrict__ norm, const float *__restrict__ eps,
                                                     float *__restrict__ Y, float2 *__restrict__ stat, int tokens)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x), t = i >> 4, j = i & 15;
    const bool live = t < tokens;
    const f4 s = live ? load_f4(S + (size_t)t * kD + 4 * j) : splat(0.0f);
    const float mean = sum16(sum4(s)) / (float)kD;
    const f4 v = s - splat(mean);
    const float rstd = 1.0f / sqrtf(sum16(sum4(v * v)) / (float)kD + eps[0]);
    if (!live) return;
    *reinterpret_cast<f4 *>(Y + (size_t)t * kD + 4 * j) = v * splat(rstd) * load_w(norm + 4 * j) + load_w(norm + kD + 4 * j);
    if (j == 0) stat[t] = make_float2(mean, rstd);
}

// Its backward over a chunk of kColRows tokens a block: with xhat = (s - mean) rstd and gy = g . gamma,
// ds = rstd (gy - mean(gy) - xhat mean(gy . xhat)); part[chunk][0..63] = the chunk's sum of g . xhat (d gamma), part[chunk][64..127]
// of g (d beta): thread (slot, j) adds its four tokens in order, the 16 slots are combined pairwise (tokens past the last are zero).
__global__ __launch_bounds__(256) void tg_ln_bwd_kernel(const float *__restrict__ G, const float *__restrict__ S, const float2 *__restrict__ stat,
                                                         const float *__restrict__ gamma, float *__restrict__ dS, float *__restrict__ part,
                                                         int tokens)
{
    __shared__ __attribute__((aligned(16))) float red[16][2 * kD];
    const int slot = threadIdx.x >> 4, j = threadIdx.x & 15;
    const f4 ga = load_w(gamma + 4 * j);
    f4 ag = splat(0.0f), ab = splat(0.0f);
    for (int p = 0; p < kColRows / 16; ++p) {
        const int t = (int)blockIdx.x * kColRows + 16 * p + slot;
        const bool live = t < tokens;
        const f4 s = live ? load_f4(S + (size_t)t * kD + 4 * j) : splat(0.0f), g = live ? load_f4(G + (size_t)t * kD + 4 * j) : splat(0.0f);
        const float2 st = live ? stat[t] : make_float2(0.0f, 0.0f);
        const f4 xhat = (s - splat(st.x)) * splat(st.y), gy = g * ga;
        const float c1 = sum16(sum4(gy)) / (float)kD, c2 = sum16(sum4(gy * xhat)) / (float)kD;
        if (live) *reinterpret_cast<f4 *>(dS + (size_t)t * kD + 4 * j) = (gy - splat(c1) - xhat * splat(c2)) * splat(st.y);
        ag = ag + g * xhat;
        ab = ab + g;
    }
    *reinterpret_cast<f4 *>(&red[slot][4 * j]) = ag;
    *reinterpret_cast<f4 *>(&red[slot][kD + 4 * j]) = ab;
    slots_to_part(red, part);
}

// ------------------------------------------------------------------------------------------------ split weight gradient --
// qg_dw_kernel's tile over ONE chunk of kRowChunk rows (blockIdx.z): part[chunk][M][K] = the chunk's dY^T . X, bpart[chunk][M] = the
// chunk's sum of dY. The chunks are rows [kRowChunk c, min(n, kRowChunk (c + 1))): a function of n alone. Rows past n and rows
// of dY past M read as zero. Four wavefronts a block = four column tiles; grid (K / 64 up, M / 16 up, chunks).
__global__ __launch_bounds__(256) void tg_dw_split_kernel(const float *__restrict__ dY, int ldy, int M, const float *__restrict__ X, int K,
                                                           float *__restrict__ part, float *__restrict__ bpart, int n)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const int ko = (int)blockIdx.x * 4 + wave, mo = blockIdx.y, chunk = blockIdx.z;
    if (16 * ko >= K) return;
    const int mrow = 16 * mo + col;
    const bool mlive = mrow < M;
    const float *ycol = dY + mrow, *xcol = X + 16 * ko + col;
    const int row0 = chunk * kRowChunk, row1 = min(n, row0 + kRowChunk);
    f4 acc[8];
    float bs[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        acc[c] = splat(0.0f);
        bs[c] = 0.0f;
    }
    for (int r0 = row0; r0 < row1; r0 += 128) {
        f4 a[8], b[8];
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = r0 + 16 * c + 4 * g + r;
                a[c][r] = row < row1 && mlive ? ycol[(size_t)row * ldy] : 0.0f;
                b[c][r] = row < row1 ? xcol[(size_t)row * K] : 0.0f;
            }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][r], b[c][r], acc[c], 0, 0, 0);
#pragma unroll
        for (int c = 0; c < 8; ++c) bs[c] += sum4(a[c]);
    }
    const f4 v = sum8(acc);
    float *out = part + (size_t)chunk * M * K;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * mo + 4 * g + r;
        if (row < M) out[(size_t)row * K + 16 * ko + col] = v[r];
    }
    if (ko == 0) {
        const float s = lanes_sum(((bs[0] + bs[1]) + (bs[2] + bs[3])) + ((bs[4] + bs[5]) + (bs[6] + bs[7])));
        if (g == 0 && mlive) bpart[(size_t)chunk * M + mrow] = s;
    }
}

// out[e] = the chunks' part[chunk][e] added in order, four partial sums (chunk & 3) combined pairwise; e < width
__global__ __launch_bounds__(256) void tg_combine_kernel(const float *__restrict__ part, int chunks, size_t width, float *__restrict__ out)
{
    const size_t e = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= width) return;
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int i = 0;
    for (; i + 4 <= chunks; i += 4)
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] += part[(size_t)(i + u) * width + e];
#pragma unroll
    for (int u = 0; u < 3; ++u)
        if (i + u < chunks) a[u] += part[(size_t)(i + u) * width + e];
    out[e] = (a[0] + a[1]) + (a[2] + a[3]);
}

// ------------------------------------------------------------------------------------------------------------ heads --
// A thread a board: z[0..3] = actor(h), z[4] = critic(h) over K = 64 (four partial sums (k & 3) of fused multiply-adds, combined
// pairwise), p = softmax(z[0..3]); the row's loss terms and dz by g2048_ppo_head.h; d2[k] = 0 where h[k] <= 0, else sum_j dz[j] W[j][k].
// LOSS false: probs and value alone (the training-mode forward of the advantage block); what follows them is not read or written.
template <bool LOSS>
__global__ __launch_bounds__(64) void tg_head_kernel(const float *__restrict__ H, const float *__restrict__ Pt, const long long *__restrict__ actions,
                                                      const float *__restrict__ old_log_probs, const float *__restrict__ adv,
                                                      const float *__restrict__ returns, float clip, float value_coef, float ent_coef,
                                                      float4 *__restrict__ probs, float *__restrict__ value, float *__restrict__ terms, size_t tstride,
                                                      float *__restrict__ dz_out, float *__restrict__ d2, int n)
{
    const int i = (int)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float *Wa = Pt + kPlActW, *Wc = Pt + kPlCriW;
    float hv[kFc2], z[5];
#pragma unroll
    for (int k = 0; k < kFc2; k += 4) {
        const f4 v = load_f4(H + (size_t)i * kFc2 + k);
        hv[k] = v[0], hv[k + 1] = v[1], hv[k + 2] = v[2], hv[k + 3] = v[3];
    }
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const float *w = j < 4 ? Wa + j * kFc2 : Wc;
        float a[4] = {j < 4 ? Pt[kPlActB + j] : Pt[kPlCriB], 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < kFc2; k += 4)
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = fmaf(w[k + u], hv[k + u], a[u]);
        z[j] = (a[0] + a[1]) + (a[2] + a[3]);
    }
    const float4 p4 = softmax4(f4{z[0], z[1], z[2], z[3]});
    probs[i] = p4;
    value[i] = z[4];
    if constexpr (!LOSS) return;
    const float p[4] = {p4.x, p4.y, p4.z, p4.w};
    float dz[5];
    {
        float da[4];
        ppo_actor_row(p, (int)(actions[i] & 3), old_log_probs[i], adv[i], clip, ent_coef, 1.0f / (float)n, terms[i], terms[2 * tstride + i], da);
#pragma unroll
        for (int j = 0; j < 4; ++j) dz[j] = da[j];
    }
    dz[4] = ppo_critic_row(z[4], returns[i], value_coef, n, terms[tstride + i]);
    *reinterpret_cast<f4 *>(dz_out + (size_t)i * 8) = f4{dz[0], dz[1], dz[2], dz[3]};
    *reinterpret_cast<f4 *>(dz_out + (size_t)i * 8 + 4) = f4{dz[4], 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < kFc2; k += 4) {
        f4 v;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float s = dz[0] * Wa[k + u];
#pragma unroll
            for (int j = 1; j < 4; ++j) s = fmaf(dz[j], Wa[j * kFc2 + k + u], s);
            s = fmaf(dz[4], Wc[k + u], s);
            v[u] = hv[k + u] <= 0.0f ? 0.0f : s;
        }
        *reinterpret_cast<f4 *>(d2 + (size_t)i * kFc2 + k) = v;
    }
}

// out[0 .. N) = 0: the training-mode pass clears a layer's two LayerNorm-eps slots of grad with a launch, not with a memset node
// (a captured graph of update() replayed a memset node of the pass with another byte on the MI355X's runtime: docs/LOG.md R32)
template <int N>
__global__ __launch_bounds__(64) void tg_zero_kernel(float *__restrict__ out)
{
    if (threadIdx.x < N) out[threadIdx.x] = 0.0f;
}

// ------------------------------------------------------------------------------------------------------------- host --
inline bool good_shape(size_t n, int dim_ff, int n_layers)
{
    return n >= 1 && n <= G2048_TLEARN_BATCH_MAX && good_encoder_shape(dim_ff, n_layers);
}

// one call of the pass. backward false: the forward launches and the two heads alone (probs, value); the loss inputs, grad and
// losses4 are then not looked at. p4, seed, call_index: the training-mode pass's (tg_pass<true>), else unused.
struct TgCall {
    const void *boards;
    const float *plain;
    const int64_t *actions;
    const float *old_log_probs, *advantages, *returns;
    size_t n;
    int dim_ff, n_layers;
    float clip_epsilon, value_coef, entropy_coef;
    float *grad, *losses4, *probs, *value;
    void *workspace;
    size_t workspace_bytes;
    void *stream;
    bool backward;
    const double *p4;
    uint64_t seed, call_index;
};

// the argument checks of both passes, all before any device call; `needed`: the workspace's bytes, `query`: the call that gives them
inline int tg_check(const char *entry, const TgCall &c, size_t needed, const char *query)
{
    if (!c.boards || !c.plain || !c.probs || !c.value || !c.workspace ||
        (c.backward && (!c.actions || !c.old_log_probs || !c.advantages || !c.returns || !c.grad || !c.losses4)))
        return fail(G2048_ERR_ARG, "%s: null pointer", entry);
    if (!aligned(c.boards, 16) || !aligned(c.plain, 16) || !aligned(c.grad, 16) || !aligned(c.probs, 16) || !aligned(c.workspace, 16) ||
        !aligned(c.actions, 8) || !aligned(c.old_log_probs, 4) || !aligned(c.advantages, 4) || !aligned(c.returns, 4) ||
        !aligned(c.losses4, 4) || !aligned(c.value, 4))
        return fail(G2048_ERR_ARG, "%s: misaligned pointer (boards, plain weights, grad, probs, workspace: 16 bytes; actions: 8; the rest: 4)",
                    entry);
    if (c.n > G2048_TLEARN_BATCH_MAX)
        return fail(G2048_ERR_ARG, "%s: n must not exceed G2048_TLEARN_BATCH_MAX = %d boards (16,384 tokens; a larger batch is not "
                                   "truncated)", entry, G2048_TLEARN_BATCH_MAX);
    if (!good_encoder_shape(c.dim_ff, c.n_layers))
        return fail(G2048_ERR_ARG, "%s: dim_ff must be a multiple of 32 (32 .. 65536) and n_layers 1 .. 64", entry);
    if (c.backward && (!good_coef(c.clip_epsilon) || !good_coef(c.value_coef) || !good_coef(c.entropy_coef)))
        return fail(G2048_ERR_ARG, "%s: clip_epsilon, value_coef and entropy_coef must be finite and not negative", entry);
    if (c.workspace_bytes < needed)
        return fail(G2048_ERR_ARG, "%s: workspace of %zu bytes, %s(n, dim_ff, n_layers) is %zu", entry, c.workspace_bytes, query, needed);
    return G2048_OK;
}

// The launch sequence, after tg_check. kDrop false: the eval-mode pass. kDrop true: site s of layer l is live where p4[s] > 0 and
// then launches the QDrop instantiation; with all four 0 the sequence and the bits are the eval-mode pass's.
// kBf16: the bf16 feed-forward mode (g2048_tbf16.h). A layer's seven products with dim_ff as an extent are g2048_tpolicy_bf16.h's, h and dh
// are bf16, and the forward packs every layer's bf16 weight copies once, before that layer's linear1.
template <bool kDrop, bool kBf16 = false>
int tg_pass(const char *entry, const TgCall &c, uint32_t domain = 0)
{
    const size_t n = c.n;
    const int dim_ff = c.dim_ff;
    const Workspace ws(n, dim_ff, c.n_layers, kBf16);
    hipStream_t s = static_cast<hipStream_t>(c.stream);
    float *base = static_cast<float *>(c.workspace);
    const float *P = c.plain, *none = nullptr;
    float *G = c.grad;
    const auto *cells = static_cast<const uint8_t *>(c.boards);
    const int ni = (int)n, T = 16 * ni, ff = dim_ff;
    const size_t nl = (size_t)c.n_layers;
    const unsigned ttiles = (unsigned)n, ntiles = (unsigned)((n + 15) / 16);        // row tiles of the token arrays, of the board arrays
    const int rchunks = (int)row_chunks((size_t)T), cchunks = (int)col_chunks((size_t)T);
    const size_t tail = kPlainLayer0 + nl * pl_layer(ff);
    const float *Pt = P + tail;
    float *Gt = G + tail;

    // site k of layer l: at(k) is its QDrop where it is live, else null
    const auto sites = [&](size_t l) { return DropSites(domain, c.seed, c.call_index, (int)l, kDrop ? c.p4 : nullptr); };
    const auto linear = [&](bool relu_out, const QDrop *d, const float *X, int K, const float *W, const float *b, const float *res, float *Y, int M,
                            int rows, unsigned tiles) {
        const dim3 grid((unsigned)(M + 63) / 64, tiles);
        if (relu_out)
            launch_site<kDrop>(d, [](auto... q) { return tg_linear_kernel<true, decltype(q)...>; }, grid, dim3(256), s, X, K, W, b, res, Y, M, rows);
        else
            launch_site<kDrop>(d, [](auto... q) { return tg_linear_kernel<false, decltype(q)...>; }, grid, dim3(256), s, X, K, W, b, res, Y, M, rows);
    };
    const auto norm = [&](const float *S, const float *np, const float *eps, float *Y, float *stat) {
        hipLaunchKernelGGL(tg_ln_kernel, dim3(ttiles), dim3(256), 0, s, S, np, eps, Y, reinterpret_cast<float2 *>(stat), T);
    };

    // the bf16 mode's feed-forward launches: a layer's packed weights (once a call, in the forward; the backward reads them again),
    // linear1 (+ ReLU, site 2) into the bf16 h, linear2 (site 3). Copy k of layer l: 0 W1, 1 its transpose, 2 W2, 3 its transpose.
    __bf16 *hb = reinterpret_cast<__bf16 *>(base + ws.h()), *dhb = reinterpret_cast<__bf16 *>(base + ws.dh());
    const __bf16 *nomask = nullptr;
    const auto packed = [&](size_t l, int k) {
        return reinterpret_cast<__bf16 *>(base + (kBf16 ? ws.wb() : 0)) + (4 * l + (size_t)k) * (size_t)kD * ff;
    };
    const auto pack_ff = [&](const auto *L, size_t l) {  // generic, as the two below: only the bf16 mode instantiates their kernels
        hipLaunchKernelGGL(tb_pack_kernel<>, dim3(blocks_for((size_t)kD * ff, 256), 2), dim3(256), 0, s, L + kPlW1, ff, kD, packed(l, 0), packed(l, 1),
                           L + pl_w2(ff), kD, ff, packed(l, 2), packed(l, 3));
    };
    const auto linear1_bf = [&](const QDrop *d, const float *L, size_t l, const auto *x1) {
        launch_site<kDrop>(d, [](auto... q) { return tb_linear_kernel<false, true, float, __bf16, decltype(q)...>; },
                           dim3((unsigned)(ff + 63) / 64, ttiles), dim3(256), s, x1, kD, static_cast<const __bf16 *>(packed(l, 0)), L + pl_b1(ff), none,
                           nomask, hb, ff, T);
    };

    // ---- the forward, its activations kept
    float *h = base + ws.h(), *a1 = base + ws.a1(), *a2 = base + ws.a2();
    hipLaunchKernelGGL(tg_embed_kernel, dim3(ttiles), dim3(256), 0, s, cells, P, base + ws.x(0), T);
    for (size_t l = 0; l < nl; ++l) {
        const float *L = P + kPlainLayer0 + l * pl_layer(ff), *norms = L + pl_norm(ff);
        const float *x0 = base + ws.x(l);
        float *qkv = base + ws.qkv(l), *prob = base + ws.prob(l), *att = base + ws.att(l), *pre1 = base + ws.pre1(l), *x1 = base + ws.x1(l),
              *pre2 = base + ws.pre2(l), *stat = base + ws.stat(l);
        const DropSites st = sites(l);
        linear(false, nullptr, x0, kD, L + kPlInW, L + kPlInB, none, qkv, kQkv, T, ttiles);
        launch_site<kDrop>(st.at(0), [](auto... q) { return tg_attention_kernel<decltype(q)...>; }, dim3((unsigned)n), dim3(256), s,
                           static_cast<const float *>(qkv), att, prob);
        linear(false, st.at(1), att, kD, L + kPlOutW, L + kPlOutB, x0, pre1, kD, T, ttiles);
        norm(pre1, norms, norms + 4 * kD, x1, stat);
        if constexpr (kBf16) {
            pack_ff(L, l);
            linear1_bf(st.at(2), L, l, x1);
            launch_site<kDrop>(st.at(3), [](auto... q) { return tb_linear_kernel<false, false, __bf16, float, decltype(q)...>; }, dim3(1, ttiles),
                               dim3(256), s, static_cast<const __bf16 *>(hb), ff, static_cast<const __bf16 *>(packed(l, 2)), L + pl_b2(ff),
                               static_cast<const float *>(x1), nomask, pre2, kD, T);
        } else {
            linear(true, st.at(2), x1, kD, L + kPlW1, L + pl_b1(ff), none, h, ff, T, ttiles);
            linear(false, st.at(3), h, ff, L + pl_w2(ff), L + pl_b2(ff), x1, pre2, kD, T, ttiles);
        }
        norm(pre2, norms + 2 * kD, norms + 4 * kD + 1, base + ws.x(l + 1), stat + 2 * (size_t)T);
    }
    const float *xL = base + ws.x(nl);                                      // [n][1024]: the flatten is a view
    linear(true, nullptr, xL, kFlat, Pt + kPlFc1W, Pt + kPlFc1B, none, a1, kFc1, ni, ntiles);
    linear(true, nullptr, a1, kFc1, Pt + kPlFc2W, Pt + kPlFc2B, none, a2, kFc2, ni, ntiles);

    // ---- the loss head
    float *dz = base + ws.dz(), *terms = base + ws.terms(), *d2 = base + ws.d2(), *d1 = base + ws.d1();
    if (!c.backward) {
        if constexpr (kDrop)
            hipLaunchKernelGGL(tg_head_kernel<false>, dim3(blocks_for(n, 64)), dim3(64), 0, s, static_cast<const float *>(a2), Pt,
                               static_cast<const long long *>(nullptr), none, none, none, 0.0f, 0.0f, 0.0f, reinterpret_cast<float4 *>(c.probs),
                               c.value, terms, ws.tstride(), dz, d2, ni);
        return check_launch(entry);
    }
    hipLaunchKernelGGL(tg_head_kernel<true>, dim3(blocks_for(n, 64)), dim3(64), 0, s, static_cast<const float *>(a2), Pt,
                       reinterpret_cast<const long long *>(c.actions), c.old_log_probs, c.advantages, c.returns, c.clip_epsilon, c.value_coef,
                       c.entropy_coef, reinterpret_cast<float4 *>(c.probs), c.value, terms, ws.tstride(), dz, d2, ni);
    hipLaunchKernelGGL(pg_loss_kernel, dim3(1), dim3(256), 0, s, static_cast<const float *>(terms), ws.tstride(), c.value_coef, c.entropy_coef,
                       c.losses4, ni);

    // ---- the backward
    float *ga = base + ws.ga(), *gb = base + ws.gb(), *ds = base + ws.ds(), *datt = base + ws.datt(), *dqkv = base + ws.dqkv(), *dh = base + ws.dh(),
          *wpart = base + ws.wpart(), *bpart = base + ws.bpart(), *cpart = base + ws.cpart();
    const auto dx = [&](const QDrop *d, const float *dY, int M, const float *W, int K, const float *res, const float *mask, float *dX, int rows,
                        unsigned tiles) {
        launch_site<kDrop>(d, [](auto... q) { return qg_dx_kernel<decltype(q)...>; }, dim3((unsigned)(K + 63) / 64, tiles), dim3(256), s, dY, M, W, K,
                           res, mask, dX, rows);
    };
    const auto dw = [&](const float *dY, int ldy, int M, const float *X, int K, float *dW, float *db) {      // over the n boards
        hipLaunchKernelGGL(qg_dw_kernel, dim3((unsigned)(K + 63) / 64, (unsigned)(M + 15) / 16), dim3(256), 0, s, dY, ldy, M, X, K, dW, db, ni);
    };
    const auto combine = [&](const float *part, int chunks, size_t width, float *out) {
        hipLaunchKernelGGL(tg_combine_kernel, dim3(blocks_for(width, 256)), dim3(256), 0, s, part, chunks, width, out);
    };
    const auto dw_split = [&](const float *dY, int M, const float *X, int K, float *dW, float *db) {         // over the 16 n tokens
        hipLaunchKernelGGL(tg_dw_split_kernel, dim3((unsigned)(K + 63) / 64, (unsigned)(M + 15) / 16, (unsigned)rchunks), dim3(256), 0, s, dY, M, M,
                           X, K, wpart, bpart, T);
        combine(wpart, rchunks, (size_t)M * K, dW);
        combine(bpart, rchunks, (size_t)M, db);
    };
    const auto dw_split_bf = [&](const auto *dY, int M, const auto *X, int K, float *dW, float *db) {       // the same in the bf16 mode
        using TA = std::remove_cv_t<std::remove_pointer_t<decltype(dY)>>;
        using TB = std::remove_cv_t<std::remove_pointer_t<decltype(X)>>;
        hipLaunchKernelGGL((tb_dw_split_kernel<TA, TB>), dim3((unsigned)(K + 63) / 64, (unsigned)(M + 63) / 64, (unsigned)rchunks), dim3(256), 0, s, dY,
                           M, X, K, wpart, bpart, T, kRowChunk);
        combine(wpart, rchunks, (size_t)M * K, dW);
        combine(bpart, rchunks, (size_t)M, db);
    };
    const auto norm_bwd = [&](const float *g, const float *pre, const float *stat, const float *gamma, float *dnorm) {
        hipLaunchKernelGGL(tg_ln_bwd_kernel, dim3((unsigned)cchunks), dim3(256), 0, s, g, pre, reinterpret_cast<const float2 *>(stat), gamma, ds,
                           cpart, T);
        combine(cpart, cchunks, 2 * kD, dnorm);
    };
    // ds x the multipliers of site 1 or 3: what enters the dropped projection's dW and dX (ds itself where the site is off)
    const auto scaled = [&](const QDrop *d) -> const float * {
        if constexpr (kDrop) {
            if (d) {
                float *dsm = base + ws.dsm();
                hipLaunchKernelGGL(qt_scale_kernel<QDrop>, dim3(blocks_for((size_t)T * kD, 256)), dim3(256), 0, s, static_cast<const float *>(ds),
                                   dsm, *d, (uint32_t)((size_t)T * kD));
                return dsm;
            }
        }
        return ds;
    };
    dw(dz, 8, 4, a2, kFc2, Gt + kPlActW, Gt + kPlActB);
    dw(dz + 4, 8, 1, a2, kFc2, Gt + kPlCriW, Gt + kPlCriB);
    dw(d2, kFc2, kFc2, a1, kFc1, Gt + kPlFc2W, Gt + kPlFc2B);
    dx(nullptr, d2, kFc2, Pt + kPlFc2W, kFc1, none, a1, d1, ni, ntiles);
    dw(d1, kFc1, kFc1, xL, kFlat, Gt + kPlFc1W, Gt + kPlFc1B);
    dx(nullptr, d1, kFc1, Pt + kPlFc1W, kFlat, none, none, ga, ni, ntiles);  // [n][1024] = [16 n][64]: the gradient at the last norm's output
    for (size_t l = nl; l-- > 0;) {
        const size_t lo = kPlainLayer0 + l * pl_layer(ff);
        const float *L = P + lo, *norms = L + pl_norm(ff);
        float *GL = G + lo, *gnorms = GL + pl_norm(ff);
        const float *x0 = base + ws.x(l), *qkv = base + ws.qkv(l), *prob = base + ws.prob(l), *att = base + ws.att(l), *x1 = base + ws.x1(l),
                    *stat = base + ws.stat(l);
        const DropSites st = sites(l);
        if constexpr (kBf16) {
            linear1_bf(st.at(2), L, l, x1);                                                   // the hidden layer again, the same mask
            norm_bwd(ga, base + ws.pre2(l), stat + 2 * (size_t)T, norms + 2 * kD, gnorms + 2 * kD);
            const float *d3 = scaled(st.at(3));
            dw_split_bf(d3, kD, static_cast<const __bf16 *>(hb), ff, GL + pl_w2(ff), GL + pl_b2(ff));
            launch_site<kDrop>(st.at(2), [](auto... q) { return tb_linear_kernel<true, false, float, __bf16, decltype(q)...>; },
                               dim3((unsigned)(ff + 63) / 64, ttiles), dim3(256), s, d3, kD, static_cast<const __bf16 *>(packed(l, 3)), none, none,
                               static_cast<const __bf16 *>(hb), dhb, ff, T);
            dw_split_bf(static_cast<const __bf16 *>(dhb), ff, x1, kD, GL + kPlW1, GL + pl_b1(ff));
            hipLaunchKernelGGL((tb_linear_kernel<true, false, __bf16, float>), dim3(1, ttiles), dim3(256), 0, s, static_cast<const __bf16 *>(dhb), ff,
                               static_cast<const __bf16 *>(packed(l, 1)), none, static_cast<const float *>(ds), nomask, gb, kD, T);
        } else {
            linear(true, st.at(2), x1, kD, L + kPlW1, L + pl_b1(ff), none, h, ff, T, ttiles);  // the hidden layer again, the same mask
            norm_bwd(ga, base + ws.pre2(l), stat + 2 * (size_t)T, norms + 2 * kD, gnorms + 2 * kD);
            const float *d3 = scaled(st.at(3));
            dw_split(d3, kD, h, ff, GL + pl_w2(ff), GL + pl_b2(ff));
            dx(st.at(2), d3, kD, L + pl_w2(ff), ff, none, h, dh, T, ttiles);
            dw_split(dh, ff, x1, kD, GL + kPlW1, GL + pl_b1(ff));
            dx(nullptr, dh, ff, L + kPlW1, kD, ds, none, gb, T, ttiles);
        }
        norm_bwd(gb, base + ws.pre1(l), stat, norms, gnorms);
        const float *d1o = scaled(st.at(1));
        dw_split(d1o, kD, att, kD, GL + kPlOutW, GL + kPlOutB);
        dx(nullptr, d1o, kD, L + kPlOutW, kD, none, none, datt, T, ttiles);
        launch_site<kDrop>(st.at(0), [](auto... q) { return tg_attention_bwd_kernel<decltype(q)...>; }, dim3((unsigned)n), dim3(256), s, qkv, prob,
                           static_cast<const float *>(datt), dqkv);
        dw_split(dqkv, kQkv, x0, kD, GL + kPlInW, GL + kPlInB);
        dx(nullptr, dqkv, kQkv, L + kPlInW, kD, ds, none, ga, T, ttiles);
        if constexpr (kDrop)                                                                                            // the eps slots
            hipLaunchKernelGGL(tg_zero_kernel<2>, dim3(1), dim3(64), 0, s, gnorms + 4 * kD);
        else if (const int rc = check_hip(hipMemsetAsync(gnorms + 4 * kD, 0, 2 * sizeof(float), s), entry))
            return rc;
    }
    hipLaunchKernelGGL(tg_embed_bwd_kernel, dim3((unsigned)cchunks), dim3(256), 0, s, static_cast<const float *>(ga), cells, cpart, T);
    combine(cpart, cchunks, 2 * kD, G + kPlainEmb);
    return check_launch(entry);
}

}  // namespace
