// g2048_step_common.h -- what the optimiser-step kernels share (g2048_qnet_step.hip: the Q-network's clipping and AdamW;
// g2048_ppo_step.hip: the PPO networks' clipping and Adam; g2048_tpolicy_step.hip: the transformer policy's, in
// libg2048_tstep_hip.so): fixed-order f64 sums over a wavefront and over a block of 256 threads, the 16-byte groups of a flat f32
// buffer with a short last group, and the host's reading of a float hyper-parameter as the decimal its caller wrote. Included by
// those three files and nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <stdio.h>
#include <stdlib.h>

#include "g2048_mfma.h"

namespace g2048 {

constexpr int kStepThreads = 256;
constexpr size_t kStepGroup = 4 * kStepThreads;      // floats a block takes in one pass: 16 bytes a lane

// the same on every lane: the xor butterfly adds the same pairs everywhere, and a + b is b + a
__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// the block's sum, the same on every thread: the four wavefronts' sums through LDS, added pairwise
__device__ inline double block_sum(double v, double (&red)[kStepThreads / 64])
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// the 1 .. 4 floats at `at` (a multiple of 4): a short group is the buffer's tail, the missing floats read as zero
__device__ inline f4 load_group(const float *__restrict__ p, size_t at, size_t floats)
{
    if (at + 4 <= floats) return load_f4(p + at);
    f4 v = splat(0.0f);
    for (size_t j = 0; at + j < floats; ++j) v[j] = p[at + j];
    return v;
}

__device__ inline void store_group(float *__restrict__ p, size_t at, size_t floats, f4 v)
{
    if (at + 4 <= floats) {
        *reinterpret_cast<f4 *>(p + at) = v;
        return;
    }
    for (size_t j = 0; at + j < floats; ++j) p[at + j] = v[j];
}

// A float hyper-parameter as the decimal its caller wrote: the shortest decimal that rounds to it (0.999f -> 0.999), in f64. The
// update needs 1 - beta, and 1 - (double)0.999f is 1.3e-5 off 0.001: the second moment would be scaled by that much against
// torch's, whose AdamW forms 1 - beta2 from the Python scalar. A value that is no short decimal comes back within half an ulp.
inline double decimal_of(float v)
{
    char s[32];
    for (int digits = 1; digits <= 9; ++digits) {
        snprintf(s, sizeof s, "%.*g", digits, (double)v);
        if (strtof(s, nullptr) == v) break;
    }
    return strtod(s, nullptr);
}

inline bool good_hyper(float v) { return std::isfinite(v) && v >= 0.0f; }

}  // namespace g2048
