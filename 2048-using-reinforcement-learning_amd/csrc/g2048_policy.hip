// g2048_policy.hip -- the PPO actor / critic forward pass of the reference (agents/ppo_agent.py:61-136, eval mode) on the
// matrix cores of gfx950 (C-ABI: include/g2048.h, g2048_policy_*).
//
//   policy_pack_kernel     rearranges a network's plain f32 weights (torch's row-major [out][in], BatchNorm already folded
//                          in) into the packed blob the forward kernel streams: every lane's MFMA A operand is one 16-byte
//                          load, and a wavefront reads one contiguous KiB per fragment.
//   policy_forward_kernel  16 -> 256 -> 128 -> 64 -> {4 | 1} for 16 * E boards per wavefront, reading the packed uint8 boards
//                          directly (x = code / 15, PPOAgent.normalize_state). Bias initialises the accumulator, ReLU is
//                          applied on the way out of it, the 4-way softmax runs in f32 in registers. blockIdx.y picks the
//                          network (0 actor, 1 critic), so one launch serves both.
//
// Layout of the computation. Every layer is computed transposed, Y^T = W . X^T: the MFMA's A operand is a 16-row tile of
// weights, its B operand 16 boards' activations, and the result tile holds output features in its rows (register r of lane l:
// feature 4 * (l >> 4) + r) and boards in its columns (l & 15). That is already the lane -> k map of the next layer's B
// operand, up to a permutation of k, so activations never leave the VGPRs: the packed weights carry the same permutation.
//   f32  (mfma_f32_16x16x4f32, exact f32):  a chunk is 16 input features = 4 MFMAs; MFMA r of input tile t reads, on lane l,
//        feature 16 t + 4 (l >> 4) + r: register r of the previous layer's tile t, as it stands.
//   bf16 (mfma_f32_16x16x32_bf16):          a chunk is 32 input features = 1 MFMA; element j of lane l is feature
//        32 s + 16 (j >> 2) + 4 (l >> 4) + (j & 3): registers 0..3 of tiles 2s and 2s + 1, rounded to bf16 (RNE).
// Layer 1 (K = 16) and layer 2 are fused: each 32-feature slice of h1 is made and consumed at once, so only layer 2's
// accumulators stay live across the loop. No split-K, no atomics: each output is one lane's own accumulation in a fixed order.
// Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/g2048.h"

extern "C" void g2048_set_last_error_(const char *msg);

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

int fail(int code, const char *msg)
{
    g2048_set_last_error_(msg);
    return code;
}

int check_launch(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char buf[200];
        snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
        g2048_set_last_error_(buf);
        return G2048_ERR_HIP;
    }
    return G2048_OK;
}

inline bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

// ------------------------------------------------------------------------------------------------ shapes and layouts --
constexpr int kIn = 16, kH1 = 256, kH2 = 128, kH3 = 64, kOutPad = 16;

// plain f32 layout (g2048_policy_pack's input): W1 b1 W2 b2 W3 b3 W4 b4, each weight [out][in]
constexpr int kPlainW1 = 0, kPlainB1 = kPlainW1 + kH1 * kIn, kPlainW2 = kPlainB1 + kH1, kPlainB2 = kPlainW2 + kH2 * kH1,
              kPlainW3 = kPlainB2 + kH2, kPlainB3 = kPlainW3 + kH3 * kH2, kPlainW4 = kPlainB3 + kH3;

// packed layout: four fragment sections, then the biases (f32, padded to 16 per layer-4 tile). A fragment is 64 lanes x 16 B
// = 1 KiB; section L holds [chunk c][output tile o] fragments. Chunk = 16 input features (f32) or 32 (bf16).
template <bool BF16> struct Packed {
    static constexpr int kChunk = BF16 ? 32 : 16;
    static constexpr int chunks(int k) { return (k + kChunk - 1) / kChunk; }
    static constexpr int kFrag = 64 * 16;
    static constexpr size_t kL1 = 0;
    static constexpr size_t kL2 = kL1 + (size_t)chunks(kIn) * (kH1 / 16) * kFrag;
    static constexpr size_t kL3 = kL2 + (size_t)chunks(kH1) * (kH2 / 16) * kFrag;
    static constexpr size_t kL4 = kL3 + (size_t)chunks(kH2) * (kH3 / 16) * kFrag;
    static constexpr size_t kBias = kL4 + (size_t)chunks(kH3) * 1 * kFrag;
    static constexpr size_t kB1 = kBias, kB2 = kB1 + 4 * kH1, kB3 = kB2 + 4 * kH2, kB4 = kB3 + 4 * kH3;
    static constexpr size_t kBytes = kB4 + 4 * kOutPad;
};
static_assert(Packed<false>::kBytes % 16 == 0 && Packed<true>::kBytes % 16 == 0, "packed sections stay 16-byte aligned");

__device__ __host__ inline uint32_t bf16_rne(float v)
{
    const uint32_t u = __float_as_uint(v);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;        // finite inputs: round to nearest even by integer add
}

// ------------------------------------------------------------------------------------------------------------- pack --
// One thread per packed 32-bit word (f32: one weight; bf16: two). Padding (layer 1's missing features in bf16, layer 4's
// rows past n_out) is written as zero, so the blob is fully defined.
template <bool BF16>
__global__ __launch_bounds__(256) void policy_pack_kernel(const float *__restrict__ plain, int n_out, uint32_t *__restrict__ packed)
{
    using P = Packed<BF16>;
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t byte = w * 4;
    if (byte >= P::kBytes) return;
    if (byte >= P::kBias) {
        const int i = (int)((byte - P::kBias) / 4);
        float v;
        if (i < kH1) v = plain[kPlainB1 + i];
        else if (i < kH1 + kH2) v = plain[kPlainB2 + i - kH1];
        else if (i < kH1 + kH2 + kH3) v = plain[kPlainB3 + i - kH1 - kH2];
        else {
            const int o = i - kH1 - kH2 - kH3;
            v = o < n_out ? plain[kPlainW4 + n_out * kH3 + o] : 0.0f;
        }
        packed[w] = __float_as_uint(v);
        return;
    }
    int K, N, wofs, rows;
    size_t base;
    if (byte >= P::kL4) { base = P::kL4; K = kH3; N = kOutPad; wofs = kPlainW4; rows = n_out; }
    else if (byte >= P::kL3) { base = P::kL3; K = kH2; N = kH3; wofs = kPlainW3; rows = kH3; }
    else if (byte >= P::kL2) { base = P::kL2; K = kH1; N = kH2; wofs = kPlainW2; rows = kH2; }
    else { base = P::kL1; K = kIn; N = kH1; wofs = kPlainW1; rows = kH1; }
    const size_t rel = byte - base;
    const int frag = (int)(rel / P::kFrag), lane = (int)(rel % P::kFrag) / 16, word = (int)(rel % 16) / 4;
    const int c = frag / (N / 16), o = frag % (N / 16);
    const int row = 16 * o + (lane & 15), h = lane >> 4;
    auto weight = [&](int k) { return (row < rows && k < K) ? plain[wofs + row * K + k] : 0.0f; };
    if (BF16) {
        uint32_t pair[2];
        for (int q = 0; q < 2; ++q) {
            const int j = 2 * word + q;
            pair[q] = bf16_rne(weight(32 * c + 16 * (j >> 2) + 4 * h + (j & 3)));
        }
        packed[w] = pair[0] | (pair[1] << 16);
    } else {
        packed[w] = __float_as_uint(weight(16 * c + 4 * h + word));
    }
}

// ---------------------------------------------------------------------------------------------------------- forward --
constexpr int kWaves = 4;

__device__ inline f4 relu(f4 v)
{
    return f4{fmaxf(v[0], 0.0f), fmaxf(v[1], 0.0f), fmaxf(v[2], 0.0f), fmaxf(v[3], 0.0f)};
}

__device__ inline bf16x8 to_bf16x8(f4 lo, f4 hi)
{
    const u4 u{bf16_rne(lo[0]) | (bf16_rne(lo[1]) << 16), bf16_rne(lo[2]) | (bf16_rne(lo[3]) << 16),
               bf16_rne(hi[0]) | (bf16_rne(hi[1]) << 16), bf16_rne(hi[2]) | (bf16_rne(hi[3]) << 16)};
    return __builtin_bit_cast(bf16x8, u);
}

__device__ inline f4 load_f4(const unsigned char *p) { return *reinterpret_cast<const f4 *>(p); }

// acc[e] += W(fragment at `frag`) . act[e] over one chunk. f32: act holds one 16-feature tile per e (4 MFMAs);
// bf16: act holds two tiles per e (one MFMA).
template <bool BF16, int E>
__device__ inline void chunk_mma(const unsigned char *frag, const f4 (&act)[E][2], f4 (&acc)[E])
{
    const f4 a = load_f4(frag);
    if constexpr (BF16) {
        const bf16x8 w = __builtin_bit_cast(bf16x8, a);
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, to_bf16x8(act[e][0], act[e][1]), acc[e], 0, 0, 0);
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int e = 0; e < E; ++e) acc[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], act[e][0][r], acc[e], 0, 0, 0);
    }
}

// One layer over activations held as 16-feature tiles act[e][t] (already through ReLU): out[e][o] = bias + W . act.
template <bool BF16, int E, int K, int N>
__device__ inline void dense(const unsigned char *sec, const float *bias, int lane, const f4 (&act)[E][K / 16], f4 (&out)[E][N / 16])
{
    using P = Packed<BF16>;
    constexpr int TPC = P::kChunk / 16;          // input tiles per chunk
#pragma unroll
    for (int o = 0; o < N / 16; ++o) {
        const f4 b = *reinterpret_cast<const f4 *>(bias + 16 * o + 4 * (lane >> 4));
#pragma unroll
        for (int e = 0; e < E; ++e) out[e][o] = b;
    }
#pragma unroll
    for (int c = 0; c < K / P::kChunk; ++c) {
#pragma unroll
        for (int o = 0; o < N / 16; ++o) {
            f4 in[E][2];
            f4 acc[E];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                in[e][0] = act[e][TPC * c];
                in[e][1] = act[e][TPC * c + TPC - 1];
                acc[e] = out[e][o];
            }
            chunk_mma<BF16, E>(sec + ((size_t)(c * (N / 16) + o) * 64 + lane) * 16, in, acc);
#pragma unroll
            for (int e = 0; e < E; ++e) out[e][o] = acc[e];
        }
    }
}

template <bool BF16, int E>
__global__ __launch_bounds__(64 * kWaves) void policy_forward_kernel(
    const uint32_t *__restrict__ boards, const unsigned char *__restrict__ actor, const unsigned char *__restrict__ critic,
    float4 *__restrict__ probs, float *__restrict__ value, size_t n)
{
    using P = Packed<BF16>;
    const int lane = threadIdx.x & 63, h = lane >> 4, col = lane & 15;
    const bool is_critic = blockIdx.y != 0;
    const unsigned char *W = is_critic ? critic : actor;
    const float *bias = reinterpret_cast<const float *>(W + P::kBias);
    const size_t env0 = ((size_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * (16 * E);
    if (env0 >= n) return;                       // whole wavefront past the end (wave-uniform)

    // layer-1 B operand: features 4h .. 4h+3 of board env0 + 16e + col (one 32-bit load; rows past n read as empty)
    f4 x[E][2];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const size_t env = env0 + 16 * e + col;
        const uint32_t cells = env < n ? boards[env * 4 + h] : 0u;
#pragma unroll
        for (int r = 0; r < 4; ++r) x[e][0][r] = (float)((cells >> (8 * r)) & 0xffu) / 15.0f;
        x[e][1] = f4{0.0f, 0.0f, 0.0f, 0.0f};    // bf16: features 16..31 of the only chunk do not exist
    }

    // layers 1 + 2, fused over 32-feature slices of h1
    f4 acc2[E][kH2 / 16];
#pragma unroll
    for (int o = 0; o < kH2 / 16; ++o) {
        const f4 b = *reinterpret_cast<const f4 *>(bias + (P::kB2 - P::kBias) / 4 + 16 * o + 4 * h);
#pragma unroll
        for (int e = 0; e < E; ++e) acc2[e][o] = b;
    }
#pragma unroll 1
    for (int s = 0; s < kH1 / 32; ++s) {
        f4 h1[E][2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int o1 = 2 * s + q;
            const f4 b = *reinterpret_cast<const f4 *>(bias + 16 * o1 + 4 * h);
            f4 acc[E];
#pragma unroll
            for (int e = 0; e < E; ++e) acc[e] = b;
            chunk_mma<BF16, E>(W + P::kL1 + ((size_t)o1 * 64 + lane) * 16, x, acc);
#pragma unroll
            for (int e = 0; e < E; ++e) h1[e][q] = relu(acc[e]);
        }
#pragma unroll
        for (int q = 0; q < 32 / P::kChunk; ++q) {               // f32: two 16-feature chunks; bf16: one 32-feature chunk
            const int c = s * (32 / P::kChunk) + q;
#pragma unroll
            for (int o = 0; o < kH2 / 16; ++o) {
                f4 in[E][2];
                f4 acc[E];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    in[e][0] = h1[e][q];
                    in[e][1] = h1[e][1];
                    acc[e] = acc2[e][o];
                }
                chunk_mma<BF16, E>(W + P::kL2 + ((size_t)(c * (kH2 / 16) + o) * 64 + lane) * 16, in, acc);
#pragma unroll
                for (int e = 0; e < E; ++e) acc2[e][o] = acc[e];
            }
        }
    }
    f4 h2[E][kH2 / 16];
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int o = 0; o < kH2 / 16; ++o) h2[e][o] = relu(acc2[e][o]);

    f4 acc3[E][kH3 / 16];
    dense<BF16, E, kH2, kH3>(W + P::kL3, bias + (P::kB3 - P::kBias) / 4, lane, h2, acc3);
#pragma unroll
    for (int e = 0; e < E; ++e)
#pragma unroll
        for (int o = 0; o < kH3 / 16; ++o) acc3[e][o] = relu(acc3[e][o]);
    f4 out[E][1];
    dense<BF16, E, kH3, kOutPad>(W + P::kL4, bias + (P::kB4 - P::kBias) / 4, lane, acc3, out);

    // rows 0..3 of the output tile sit in lanes 0..15 (h == 0), one board per lane
    if (h != 0) return;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const size_t env = env0 + 16 * e + col;
        if (env >= n) continue;
        const f4 z = out[e][0];
        if (is_critic) {
            value[env] = z[0];
        } else {                                  // nn.Softmax(dim=-1): exp(z - max) / sum, in f32
            const float m = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
            const float e0 = expf(z[0] - m), e1 = expf(z[1] - m), e2 = expf(z[2] - m), e3 = expf(z[3] - m);
            const float sum = ((e0 + e1) + e2) + e3;
            probs[env] = make_float4(e0 / sum, e1 / sum, e2 / sum, e3 / sum);
        }
    }
}

// boards per wavefront: f32 is MFMA-issue bound, two 16-board tiles hide the 40-cycle dependent latency and halve the weight
// stream; bf16 MFMAs are 16x cheaper, so it takes four tiles per fragment load (DESIGN.md "Policy forward")
constexpr int kTilesF32 = 2, kTilesBF16 = 4;

}  // namespace

extern "C" {

size_t g2048_policy_packed_bytes(int precision, int n_out)
{
    if (n_out != 1 && n_out != 4) return 0;
    if (precision == G2048_POLICY_F32) return Packed<false>::kBytes;
    if (precision == G2048_POLICY_BF16) return Packed<true>::kBytes;
    return 0;
}

int g2048_policy_pack(const float *plain_f32, int n_out, int precision, void *packed_out, void *stream)
{
    if (!plain_f32 || !packed_out) return fail(G2048_ERR_ARG, "g2048_policy_pack: null pointer");
    if (!aligned(plain_f32, 4) || !aligned(packed_out, 16)) return fail(G2048_ERR_ARG, "g2048_policy_pack: misaligned pointer");
    if (n_out != 1 && n_out != 4) return fail(G2048_ERR_ARG, "g2048_policy_pack: n_out must be 4 (actor) or 1 (critic)");
    if (precision != G2048_POLICY_F32 && precision != G2048_POLICY_BF16) return fail(G2048_ERR_ARG, "g2048_policy_pack: unknown precision");
    const size_t bytes = g2048_policy_packed_bytes(precision, n_out);
    const dim3 grid((unsigned)((bytes / 4 + 255) / 256));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (precision == G2048_POLICY_BF16)
        hipLaunchKernelGGL(policy_pack_kernel<true>, grid, dim3(256), 0, s, plain_f32, n_out, static_cast<uint32_t *>(packed_out));
    else
        hipLaunchKernelGGL(policy_pack_kernel<false>, grid, dim3(256), 0, s, plain_f32, n_out, static_cast<uint32_t *>(packed_out));
    return check_launch("g2048_policy_pack");
}

int g2048_policy_forward(const void *boards, const void *actor_packed, const void *critic_packed_or_null, float *probs_out,
                         float *value_out_or_null, size_t n, uint32_t opts, void *stream)
{
    if (n == 0) return G2048_OK;
    if (!boards || !actor_packed || !probs_out) return fail(G2048_ERR_ARG, "g2048_policy_forward: null pointer");
    if (!critic_packed_or_null != !value_out_or_null)
        return fail(G2048_ERR_ARG, "g2048_policy_forward: critic_packed and value_out must both be given or both be NULL");
    if (!aligned(boards, 16) || !aligned(actor_packed, 16) || !aligned(critic_packed_or_null, 16) || !aligned(probs_out, 16) ||
        !aligned(value_out_or_null, 4))
        return fail(G2048_ERR_ARG, "g2048_policy_forward: misaligned pointer (boards, packed weights, probs: 16 bytes; value: 4)");
    if (opts != G2048_POLICY_F32 && opts != G2048_POLICY_BF16) return fail(G2048_ERR_ARG, "g2048_policy_forward: unknown opts (precision)");
    const bool bf16 = opts == G2048_POLICY_BF16;
    const size_t per_block = (size_t)kWaves * 16 * (bf16 ? kTilesBF16 : kTilesF32);
    const size_t blocks = (n + per_block - 1) / per_block;
    if (blocks > 0x7fffffffu) return fail(G2048_ERR_ARG, "g2048_policy_forward: n too large for one launch");
    const dim3 grid((unsigned)blocks, critic_packed_or_null ? 2u : 1u);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const auto *b = static_cast<const uint32_t *>(boards);
    const auto *a = static_cast<const unsigned char *>(actor_packed);
    const auto *c = static_cast<const unsigned char *>(critic_packed_or_null);
    if (bf16)
        hipLaunchKernelGGL((policy_forward_kernel<true, kTilesBF16>), grid, dim3(64 * kWaves), 0, s, b, a, c,
                           reinterpret_cast<float4 *>(probs_out), value_out_or_null, n);
    else
        hipLaunchKernelGGL((policy_forward_kernel<false, kTilesF32>), grid, dim3(64 * kWaves), 0, s, b, a, c,
                           reinterpret_cast<float4 *>(probs_out), value_out_or_null, n);
    return check_launch("g2048_policy_forward");
}

}  // extern "C"
