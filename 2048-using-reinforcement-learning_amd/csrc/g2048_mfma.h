// g2048_mfma.h -- the fragment toolkit of the three network files (g2048_policy.hip, g2048_tpolicy.hip, g2048_qnet.hip) and of the
// batch passes: the vector types, the small f32 helpers, the one MFMA step over a packed weight fragment, the kernel that packs a
// matrix into such fragments, and for the batch passes the load of a plain weight row (load_w) and the product over it
// (chunks_product). Device code, included by the library's .hip files and the headers they share.
//
// A fragment is 64 lanes x 16 bytes = 1 KiB: the MFMA A operand of one 16-row tile of weights over one chunk of K, a lane's
// share one 16-byte load. Lane l (g = l >> 4) holds row 16 o + (l & 15) of the matrix. A chunk is
//   f32  (mfma_f32_16x16x4f32)     16 input features = 4 MFMAs; word r of the lane is k = 16 c + 4 g + r;
//   bf16 (mfma_f32_16x16x32_bf16)  32 input features = 1 MFMA; element j of the lane is k = 32 c + 16 (j >> 2) + 4 g + (j & 3),
// which is the order in which the previous product's result tiles hold their features, so a result register is the next B operand
// as it stands (fragment_word is the one place that spells this out).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace g2048 {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kFrag = 64 * 16;                       // bytes of one fragment

__device__ __host__ inline uint32_t bf16_rne(float v)
{
    const uint32_t u = __float_as_uint(v);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;        // finite inputs: round to nearest even by integer add
}

__device__ inline f4 relu(f4 v)
{
    return f4{fmaxf(v[0], 0.0f), fmaxf(v[1], 0.0f), fmaxf(v[2], 0.0f), fmaxf(v[3], 0.0f)};
}

// torch.relu: a NaN stays a NaN (fmaxf returns the operand that is none). Finite values as relu's.
__device__ inline f4 relu_nan(f4 v)
{
    f4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = v[i] > 0.0f ? v[i] : v[i] != v[i] ? v[i] : 0.0f;
    return r;
}

__device__ inline f4 load_f4(const void *p) { return *reinterpret_cast<const f4 *>(p); }
__device__ inline f4 splat(float v) { return f4{v, v, v, v}; }

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));      // 16 bytes of a plain f32 buffer: 4-byte aligned at worst
__device__ inline f4 load_w(const float *p) { const f4u v = *reinterpret_cast<const f4u *>(p); return f4{v[0], v[1], v[2], v[3]}; }

// Two result tiles as one bf16 B operand. INT_RNE: by bf16_rne's integer add (g2048_policy.hip, whose forward kernel was
// written and measured with it); otherwise the float -> __bf16 cast, gfx950's v_cvt_pk_bf16_f32 (round to nearest even, two
// values per instruction). Finite values round the same either way.
template <bool INT_RNE = false>
__device__ inline bf16x8 to_bf16x8(f4 lo, f4 hi)
{
    if constexpr (INT_RNE) {
        const u4 u{bf16_rne(lo[0]) | (bf16_rne(lo[1]) << 16), bf16_rne(lo[2]) | (bf16_rne(lo[3]) << 16),
                   bf16_rne(hi[0]) | (bf16_rne(hi[1]) << 16), bf16_rne(hi[2]) | (bf16_rne(hi[3]) << 16)};
        return __builtin_bit_cast(bf16x8, u);
    } else {
        return bf16x8{(__bf16)lo[0], (__bf16)lo[1], (__bf16)lo[2], (__bf16)lo[3], (__bf16)hi[0], (__bf16)hi[1], (__bf16)hi[2], (__bf16)hi[3]};
    }
}

// acc[e] += W(fragment at `frag`) . act[e] over one chunk (f32: act[e][0] is the chunk's tile, 4 MFMAs; bf16: act[e][0..1], one MFMA).
// TRANSPOSED: acc[e] += act[e]^T . W^T instead, the activation as the A operand and the same fragment as the B operand.
template <bool BF16, int E, bool TRANSPOSED = false, bool INT_RNE = false>
__device__ inline void chunk_mma(const unsigned char *frag, const f4 (&act)[E][2], f4 (&acc)[E])
{
    const f4 a = load_f4(frag);
    if constexpr (BF16) {
        const bf16x8 w = __builtin_bit_cast(bf16x8, a);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const bf16x8 x = to_bf16x8<INT_RNE>(act[e][0], act[e][1]);
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

// The batch passes' product over a plain row-major W (the Q-network's g2048_qnet_batch_fwd.h, the transformer policy's
// g2048_tpolicy_grad_pass.h): acc (features 16 o + 4 g + r of row `col` of the tile) += W[16 o ..][K] . X[row][K]. Lane (col, g): the
// A operand is W[16 o + col][16 c + 4 g ..], the B operand X[row][16 c + 4 g ..], four MFMAs a chunk. N chunks at once, every load
// issued before the first MFMA (K is a multiple of 32: the chunks come in pairs). Chunk c of a group of eight accumulates into
// acc[c]: eight independent partial sums, so that consecutive MFMAs do not wait on each other and the rounding error of a long K
// grows like a blocked sum's, not like one serial chain's. The order is fixed all the same.
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

// nn.Softmax(dim=-1) of one board's four logits: exp(z - max) / sum, in f32
__device__ __forceinline__ float4 softmax4(f4 z)
{
    const float m = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
    const float e0 = expf(z[0] - m), e1 = expf(z[1] - m), e2 = expf(z[2] - m), e3 = expf(z[3] - m);
    const float sum = ((e0 + e1) + e2) + e3;
    return make_float4(e0 / sum, e1 / sum, e2 / sum, e3 / sum);
}

// ------------------------------------------------------------------------------------------------------------- pack --
// Packed 32-bit word `word` (0..3) of a lane of group g in chunk c of a row tile: f32 one weight, bf16 two (RNE), taken from
// weight(k) at the k of the header. The fragment-word addressing of every pack kernel.
template <bool BF16, class Weight>
__device__ inline uint32_t fragment_word(int c, int g, int word, Weight weight)
{
    if constexpr (BF16) {
        uint32_t pair[2];
        for (int q = 0; q < 2; ++q) {
            const int j = 2 * word + q;
            pair[q] = bf16_rne(weight(32 * c + 16 * (j >> 2) + 4 * g + (j & 3)));
        }
        return pair[0] | (pair[1] << 16);
    } else {
        return __float_as_uint(weight(16 * c + 4 * g + word));
    }
}

namespace {                                          // per translation unit: two of them launch it, and share no host stub

// One thread per packed word of a matrix of rows_a + rows_b rows (a over b, e.g. actor over critic in a head tile; rows past them
// zero) and K columns, its fragments ordered [row tile o][chunk c]: the word holds W[16 o + (l & 15)][col(k)], where packed column
// k is the plain column (k % inner) * stride + k / inner (the identity for inner = K, stride = 1).
template <bool BF16>
__global__ __launch_bounds__(256) void pack_matrix_kernel(const float *__restrict__ a, int rows_a, const float *__restrict__ b, int rows_b,
                                                           int K, int inner, int stride, unsigned words, uint32_t *__restrict__ packed)
{
    const unsigned w = blockIdx.x * 256u + threadIdx.x;
    if (w >= words) return;
    const int chunks = K / (BF16 ? 32 : 16);
    const int frag = (int)(w / 256u), lane = (int)(w % 256u) / 4, word = (int)(w % 4u);
    const int o = frag / chunks, c = frag % chunks;
    const int row = 16 * o + (lane & 15), g = lane >> 4;
    packed[w] = fragment_word<BF16>(c, g, word, [&](int k) {
        const size_t col = (size_t)(k % inner) * stride + k / inner;
        if (row < rows_a) return a[(size_t)row * K + col];
        if (row < rows_a + rows_b) return b[(size_t)(row - rows_a) * K + col];
        return 0.0f;
    });
}

}  // namespace

}  // namespace g2048
