// g2048_step_common.h -- what the optimiser-step kernels share (g2048_qnet_step.hip: the Q-network's clipping and AdamW;
// g2048_ppo_step.hip: the PPO networks' clipping and Adam; g2048_tpolicy_step.hip: the transformer policy's, in
// libg2048_tstep_hip.so), each written once because its exact operation order is the contract with torch's bits:
//   host    the reading of a float hyper-parameter as the decimal its caller wrote, the check of the Adam hyper-parameters and the
//           update's scalars built from them, and the split of a flat buffer into at most kStepMaxPartials chunks;
//   both    the clip coefficient and the f64 bias corrections (the Q-network forms them on the host, the other two in their
//           prepare kernels);
//   device  fixed-order f64 sums over a wavefront and over a block of 256 threads, the 16-byte groups of a flat f32 buffer with a
//           short last group, a thread's share of a sum of squares, the block's total of the partial sums, the NaN-loss gate, one
//           Adam update of a group and the LayerNorm-eps slots that keep their bits.
// Included by those three files and nothing else in the library; the host part calls no HIP function, so a host-only build of a
// program that includes this header checks it without a device.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <stdio.h>
#include <stdlib.h>

#include "g2048_mfma.h"

namespace g2048 {

constexpr int kStepThreads = 256;
constexpr size_t kStepGroup = 4 * kStepThreads;      // floats a block takes in one pass: 16 bytes a lane
constexpr size_t kStepMaxPartials = 4 * kStepThreads;        // partials_total reads four partial sums a thread

// floats a block owns: the buffer in at most kStepMaxPartials equal chunks, whole passes of 1,024 floats. A function of the float
// count alone, never of the device.
constexpr size_t step_chunk(size_t floats)
{
    const size_t per = (floats + kStepMaxPartials - 1) / kStepMaxPartials;
    return (per + kStepGroup - 1) / kStepGroup * kStepGroup;
}
constexpr size_t step_partials(size_t floats) { return (floats + step_chunk(floats) - 1) / step_chunk(floats); }
constexpr size_t step_partial_bytes(size_t floats) { return (step_partials(floats) * sizeof(double) + 15) / 16 * 16; }

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

// nullptr, or what is wrong with an Adam step's hyper-parameters, to stand behind "<entry point>: ". lr_eps: every learning rate
// and eps of the call; weight_decay: null where the entry point has none.
inline const char *adam_hyper_defect(const float *lr_eps, int n, float beta1, float beta2, const float *weight_decay, float max_norm)
{
    bool good = good_hyper(beta1) && good_hyper(beta2) && (!weight_decay || good_hyper(*weight_decay));
    for (int i = 0; i < n; ++i) good = good && good_hyper(lr_eps[i]);
    if (!good)
        return weight_decay ? "lr, beta1, beta2, eps and weight_decay must be finite and not negative"
                            : "lr, beta1, beta2 and eps must be finite and not negative";
    if (beta1 >= 1.0f || beta2 >= 1.0f) return "beta1 and beta2 must be below 1";
    if (!(max_norm > 0.0f)) return "max_norm must be above 0 (+inf: no clipping)";
    return nullptr;
}

// what the moments' lines of the update multiply by
struct AdamBetas {
    float one_minus_beta1, beta2, one_minus_beta2;
};

// the betas as the decimals their caller wrote, which the bias corrections take, and the update's scalars formed from those
struct BetaScalars {
    double beta1, beta2;
    AdamBetas update;
};

inline BetaScalars beta_scalars(float beta1, float beta2)
{
    const double b1 = decimal_of(beta1), b2 = decimal_of(beta2);
    return BetaScalars{b1, b2, AdamBetas{(float)(1.0 - b1), beta2, (float)(1.0 - b2)}};
}

// the reciprocal first: how torch evaluates max_norm / tensor
__host__ __device__ inline float clip_coefficient(float norm, float max_norm) { return fminf(1.0f, (1.0f / (norm + 1e-6f)) * max_norm); }

// lr / bc1 and sqrt(bc2) of Adam's step number t (from 1), formed in f64
struct BiasCorrections {
    float step_size, bc2_sqrt;
};

__host__ __device__ inline BiasCorrections bias_corrections(double lr, double beta1, double beta2, double t)
{
    const double bc1 = 1.0 - pow(beta1, t), bc2 = 1.0 - pow(beta2, t);
    return BiasCorrections{(float)(lr / bc1), (float)sqrt(bc2)};
}

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

// a thread's share of the sum of grad[i]^2: the groups at begin, begin + stride, .. below end in order, one f64 sum a vector
// component, combined pairwise. Squares and sums are f64: a float's square is exact there.
__device__ inline double sum_squares(const float *__restrict__ grad, size_t begin, size_t end, size_t stride, size_t floats)
{
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t at = begin; at < end; at += stride) {
        const f4 g = load_group(grad, at, floats);
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] += (double)g[j] * (double)g[j];
    }
    return (a[0] + a[1]) + (a[2] + a[3]);
}

// the sum of a chunked buffer's partial sums, the same on every thread of every block that asks: four a thread, pairwise
__device__ inline double partials_total(const double *__restrict__ partial, int partials, double (&red)[kStepThreads / 64])
{
    double p4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = (int)threadIdx.x + u * kStepThreads;             // partials <= kStepMaxPartials = 4 x 256
        p4[u] = i < partials ? partial[i] : 0.0;
    }
    return block_sum((p4[0] + p4[1]) + (p4[2] + p4[3]), red);
}

// isnan only, the reference's rule: +inf is applied
__device__ inline bool nan_loss(const float *__restrict__ loss_or_null)
{
    if (!loss_or_null) return false;
    const float loss = loss_or_null[0];
    return loss != loss;
}

// the same 16-byte group of the four buffers of an update
struct StepGroup {
    f4 g, p, m, v;
};

__device__ inline StepGroup load_step_group(const float *__restrict__ plain, const float *__restrict__ grad, const float *__restrict__ exp_avg,
                                            const float *__restrict__ exp_avg_sq, size_t at, size_t floats)
{
    StepGroup s;
    s.g = load_group(grad, at, floats);
    s.p = load_group(plain, at, floats);
    s.m = load_group(exp_avg, at, floats);
    s.v = load_group(exp_avg_sq, at, floats);
    return s;
}

__device__ inline void store_step_group(float *__restrict__ plain, float *__restrict__ grad, float *__restrict__ exp_avg,
                                        float *__restrict__ exp_avg_sq, size_t at, size_t floats, const StepGroup &s)
{
    store_group(grad, at, floats, s.g);
    store_group(plain, at, floats, s.p);
    store_group(exp_avg, at, floats, s.m);
    store_group(exp_avg_sq, at, floats, s.v);
}

// One Adam update of a group, every operation rounded to f32 on its own (-ffp-contract=off) in the order of torch's single-tensor
// Adam and AdamW:
//   g = grad c;  [kDecay: p = plain decay, decay = 1 - lr wd;]  m += (g - m)(1 - beta1);  v = v beta2 + (g g)(1 - beta2);
//   p -= step_size (m / (sqrt(v) / bc2_sqrt + eps))
template <bool kDecay>
__device__ inline StepGroup adam_update(const StepGroup &s, float c, float decay, AdamBetas k, BiasCorrections bc, float eps)
{
    StepGroup o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o.g[j] = s.g[j] * c;
        o.p[j] = kDecay ? s.p[j] * decay : s.p[j];
        o.m[j] = s.m[j] + (o.g[j] - s.m[j]) * k.one_minus_beta1;
        o.v[j] = s.v[j] * k.beta2 + (o.g[j] * o.g[j]) * k.one_minus_beta2;
        o.p[j] = o.p[j] - bc.step_size * (o.m[j] / (sqrtf(o.v[j]) / bc.bc2_sqrt + eps));
    }
    return o;
}

// A LayerNorm-eps slot -- the last two floats of a layer's block of layer_len floats, the layers lying in [base, layers_end) -- is
// a setting, not a parameter: all four buffers keep their bits there. base is a multiple of 4, so the group at `at` lies before
// the layers or from their start on; past them it is not looked at.
__device__ inline void keep_eps_slots(StepGroup &o, const StepGroup &s, size_t at, size_t base, unsigned layers_end, unsigned layer_len)
{
    if (at < base || at >= layers_end) return;
    const unsigned r = (unsigned)(at - base) % layer_len;
    if (r + 5 < layer_len) return;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (r + j == layer_len - 2 || r + j == layer_len - 1) {
            o.g[j] = s.g[j];
            o.p[j] = s.p[j];
            o.m[j] = s.m[j];
            o.v[j] = s.v[j];
        }
}

}  // namespace g2048
