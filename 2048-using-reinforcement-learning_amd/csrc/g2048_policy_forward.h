// g2048_policy_forward.h -- the parts of the PPO actor / critic forward pass (g2048_policy.hip has the description) that more
// than one kernel file expands: the packed blob's layout, the layers as one macro with its helpers, the tile counts per
// precision and the dispatch on them. Included by g2048_policy.hip (the forward kernel, the game-playing kernel) and by
// g2048_ppo_collect.hip (the PPO experience collector, a library of its own); both expand exactly this text, so a board's
// probabilities and value are the same bits in every one of them. Compile with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "g2048_host.h"
#include "g2048_mfma.h"

namespace {

using namespace g2048;

// ------------------------------------------------------------------------------------------------ shapes and layouts --
constexpr int kIn = 16, kH1 = 256, kH2 = 128, kH3 = 64, kOutPad = 16;

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

// ---------------------------------------------------------------------------------------------------------- forward --
// chunk_mma's bf16 operand is rounded by integer add here, not by the __bf16 cast: the forward kernel was written and measured
// with that form, and keeps it
constexpr bool kIntRne = true;

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
            chunk_mma<BF16, E, false, kIntRne>(sec + ((size_t)(c * (N / 16) + o) * 64 + lane) * 16, in, acc);
#pragma unroll
            for (int e = 0; e < E; ++e) out[e][o] = acc[e];
        }
    }
}

// The pieces of the forward pass that the forward kernel, the game-playing kernel (policy_play_kernel) and the experience
// collector (ppo_collect_kernel) share. All compute a board's outputs with exactly these instructions, and a board's outputs do
// not depend on the tile column or the tile e it sits in, so the kernels give bit-identical outputs for the same board and blob.

// layer-1 B operand of one tile: features 4h .. 4h+3 of the board whose row h is `cells` (PPOAgent.normalize_state)
__device__ __forceinline__ void board_operand(uint32_t cells, f4 (&x)[2])
{
#pragma unroll
    for (int r = 0; r < 4; ++r) x[0][r] = (float)((cells >> (8 * r)) & 0xffu) / 15.0f;
    x[1] = f4{0.0f, 0.0f, 0.0f, 0.0f};           // bf16: features 16..31 of the only chunk do not exist
}

// Layers 1..4 of the network at W (bias = W + kBias, P = Packed<BF16>) for the E tiles of B operands x of a wavefront; declares
// out[E][1]: register r of out[e][0] on lane l (l < 16) = output r of board 16 e + l (rows 4.. of the padded layer-4 tile are
// zero weights). A macro, not a function: as an inlined function the same code compiles the forward kernel to another
// schedule that runs 4-6 % slower (measured against the parent build); expanded in place it is instruction for instruction
// the kernel it was. Layers 1 + 2 are fused over 32-feature slices of h1 (f32: two 16-feature chunks; bf16: one 32-feature
// chunk).
#define POLICY_LAYERS_(BF16, E, W, bias, lane, h, x, out) \
    f4 acc2[E][kH2 / 16]; \
_Pragma("unroll") \
    for (int o = 0; o < kH2 / 16; ++o) { \
        const f4 b = *reinterpret_cast<const f4 *>(bias + (P::kB2 - P::kBias) / 4 + 16 * o + 4 * h); \
_Pragma("unroll") \
        for (int e = 0; e < E; ++e) acc2[e][o] = b; \
    } \
_Pragma("unroll 1") \
    for (int s = 0; s < kH1 / 32; ++s) { \
        f4 h1[E][2]; \
_Pragma("unroll") \
        for (int q = 0; q < 2; ++q) { \
            const int o1 = 2 * s + q; \
            const f4 b = *reinterpret_cast<const f4 *>(bias + 16 * o1 + 4 * h); \
            f4 acc[E]; \
_Pragma("unroll") \
            for (int e = 0; e < E; ++e) acc[e] = b; \
            chunk_mma<BF16, E, false, kIntRne>(W + P::kL1 + ((size_t)o1 * 64 + lane) * 16, x, acc); \
_Pragma("unroll") \
            for (int e = 0; e < E; ++e) h1[e][q] = relu(acc[e]); \
        } \
_Pragma("unroll") \
        for (int q = 0; q < 32 / P::kChunk; ++q) { \
            const int c = s * (32 / P::kChunk) + q; \
_Pragma("unroll") \
            for (int o = 0; o < kH2 / 16; ++o) { \
                f4 in[E][2]; \
                f4 acc[E]; \
_Pragma("unroll") \
                for (int e = 0; e < E; ++e) { \
                    in[e][0] = h1[e][q]; \
                    in[e][1] = h1[e][1]; \
                    acc[e] = acc2[e][o]; \
                } \
                chunk_mma<BF16, E, false, kIntRne>(W + P::kL2 + ((size_t)(c * (kH2 / 16) + o) * 64 + lane) * 16, in, acc); \
_Pragma("unroll") \
                for (int e = 0; e < E; ++e) acc2[e][o] = acc[e]; \
            } \
        } \
    } \
    f4 h2[E][kH2 / 16]; \
_Pragma("unroll") \
    for (int e = 0; e < E; ++e) \
_Pragma("unroll") \
        for (int o = 0; o < kH2 / 16; ++o) h2[e][o] = relu(acc2[e][o]); \
    f4 acc3[E][kH3 / 16]; \
    dense<BF16, E, kH2, kH3>(W + P::kL3, bias + (P::kB3 - P::kBias) / 4, lane, h2, acc3); \
_Pragma("unroll") \
    for (int e = 0; e < E; ++e) \
_Pragma("unroll") \
        for (int o = 0; o < kH3 / 16; ++o) acc3[e][o] = relu(acc3[e][o]); \
    f4 out[E][1]; \
    dense<BF16, E, kH3, kOutPad>(W + P::kL4, bias + (P::kB4 - P::kBias) / 4, lane, acc3, out);

// boards per wavefront: f32 is MFMA-issue bound, two 16-board tiles hide the 40-cycle dependent latency and halve the weight
// stream; bf16 MFMAs are 16x cheaper, so it takes four tiles per fragment load (DESIGN.md "Policy forward")
constexpr int kTilesF32 = 2, kTilesBF16 = 4;

// the kernels' two instantiations: f(BF16, boards-of-16 per wavefront) with the constants of the precision asked for
template <class F>
auto with_precision(bool bf16, F &&f)
{
    return bf16 ? f(std::true_type{}, int_c<kTilesBF16>{}) : f(std::false_type{}, int_c<kTilesF32>{});
}

}  // namespace
