// g2048_qnet_forward.h -- the parts of the hybrid agent's Q-network (g2048_qnet.hip has the description) that more than one
// kernel file expands: the blob's layout, the per-wavefront forward pass as two macros with their helpers, select_action in its
// two halves, the LDS column of a planned decision, the wavefront's LDS fence and the host checks of epsilon and the beam
// settings. Included by g2048_qnet.hip (the forward, the select / beam kernels, the game-playing kernel) and by
// g2048_qnet_collect.hip (the experience collector, a library of its own); both expand exactly this text, so a board's Q-values
// and its action are the same bits in every one of them. Compile with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/g2048.h"
#include "g2048_board.h"
#include "g2048_host.h"
#include "g2048_lookahead.h"
#include "g2048_mfma.h"
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

// ---------------------------------------------------------------------------------------------------------- forward --
// The forward pass in two pieces that qnet_forward_kernel, the game-playing kernel (qnet_play_kernel) and the experience
// collector (qnet_collect_kernel, g2048_qnet_collect.hip) share. All of them
// expand exactly this text, and a wavefront's pass depends on nothing but its own 32 boards and the blob, so the kernels give
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

// LDS accesses of one wavefront complete in program order; this only keeps the compiler from moving them across the point
// where lanes read what other lanes of the wavefront wrote.
__device__ inline void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------------------------------------------ host checks --
inline bool good_epsilon(float e) { return e >= 0.0f && e <= 1.0f; }      // false for NaN

// the settings of the reference's beam_search: G2048_OK, or the error as `entry`'s
inline int check_beam_settings(const char *entry, int beam_width, int search_depth, int threshold)
{
    if (beam_width < 1 || beam_width > 64) return fail(G2048_ERR_ARG, "%s: beam_width must lie in 1 .. 64", entry);
    if (search_depth < 1) return fail(G2048_ERR_ARG, "%s: search_depth must be at least 1", entry);
    if (threshold < 1) return fail(G2048_ERR_ARG, "%s: threshold (a tile value) must be at least 1", entry);
    return G2048_OK;
}

}  // namespace
