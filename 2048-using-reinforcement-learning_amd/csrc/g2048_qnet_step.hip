// g2048_qnet_step.hip -- what follows the backward pass in DQNAgent.train_step (agents/hybrid.py:1057-1058) for the hybrid agent's
// Q-network on the device: clip_grad_norm_ and AdamW.step() over the whole PLAIN parameter buffer (include/g2048.h,
// g2048_qnet_pack's input) and the gradient buffer g2048_qnet_loss_grad fills, which is laid out like it. C-ABI:
// g2048_qnet_adamw_step / g2048_qnet_step_workspace. Two launches, no host synchronisation:
//   norm     block b adds grad[i]^2 over its chunk of the buffer in a fixed order and writes ONE partial sum; the chunk is a
//            function of the float count alone (step_chunk), never of the device, and there are at most
//            G2048_QNET_STEP_MAX_PARTIALS of them. Squares, partial sums and the total are f64: a float's square is exact in
//            f64 and the sum of a million of them keeps 1e-6 of the norm with nine digits to spare.
//   update   every block adds ALL partials up again, in the same order, so every block holds the same norm; block 0 writes it
//            out. A norm that is not finite ends the launch there: nothing else is written. Otherwise the block clips and
//            updates its chunk, 16 bytes a lane at a time, every operation rounded to f32 on its own (-ffp-contract=off) in
//            the order of torch's single-tensor AdamW:
//              g = grad c;  p = plain (1 - lr wd);  m += (g - m)(1 - beta1);  v = v beta2 + (g g)(1 - beta2);
//              p -= (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
//            The two LayerNorm-eps slots of every layer are settings, not parameters: all four buffers keep their bits there.
//            A layer's block is = 2 mod 4 floats long, so the pair is the first half of a 16-byte group in one layer and the
//            second half in the next, and with an odd layer count the buffer ends in a group of two floats.
// No atomics, no block waits on another, nothing depends on the compute-unit count: two calls give the same bits.
#include <hip/hip_runtime.h>

#include "../../include/g2048.h"
#include "g2048_host.h"
#include "g2048_step_common.h"      // wave_sum, block_sum, load_group, store_group, decimal_of, good_hyper

namespace {

using namespace g2048;

constexpr size_t kEpsBase = 139616;                  // the first layer's block starts here (a multiple of 4)
constexpr size_t kFcFloats = 4 * 128 + 4;
static_assert(G2048_QNET_STEP_MAX_PARTIALS == 4 * kStepThreads, "the update kernel reads four partial sums a thread");

constexpr size_t layer_floats(size_t ff) { return 66690 + 257 * ff; }
constexpr size_t plain_floats(size_t ff, size_t layers) { return kEpsBase + layers * layer_floats(ff) + kFcFloats; }

// floats a block owns: the buffer in at most G2048_QNET_STEP_MAX_PARTIALS equal chunks, whole passes of 1,024 floats
constexpr size_t step_chunk(size_t floats)
{
    const size_t per = (floats + G2048_QNET_STEP_MAX_PARTIALS - 1) / G2048_QNET_STEP_MAX_PARTIALS;
    return (per + kStepGroup - 1) / kStepGroup * kStepGroup;
}
constexpr size_t step_partials(size_t floats) { return (floats + step_chunk(floats) - 1) / step_chunk(floats); }

// ------------------------------------------------------------------------------------------------------------- norm --
// partial[block] = the sum of grad[i]^2 over the block's chunk: thread t takes the groups t, t + 256, .. of the chunk in order, one
// f64 sum a vector component, combined pairwise; then the butterfly and the four wavefronts
__global__ __launch_bounds__(kStepThreads) void qs_norm_kernel(const float *__restrict__ grad, size_t floats, size_t chunk,
                                                                double *__restrict__ partial)
{
    __shared__ double red[kStepThreads / 64];
    const size_t begin = (size_t)blockIdx.x * chunk, end = begin + chunk < floats ? begin + chunk : floats;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t at = begin + 4 * threadIdx.x; at < end; at += kStepGroup) {
        const f4 g = load_group(grad, at, floats);
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] += (double)g[j] * (double)g[j];
    }
    const double s = block_sum((a[0] + a[1]) + (a[2] + a[3]), red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ----------------------------------------------------------------------------------------------------------- update --
struct StepScalars {
    float decay, one_minus_beta1, beta2, one_minus_beta2, step_size, bc2_sqrt, eps, max_norm;
};

__global__ __launch_bounds__(kStepThreads) void qs_update_kernel(float *__restrict__ plain, float *__restrict__ grad, float *__restrict__ exp_avg,
                                                                  float *__restrict__ exp_avg_sq, size_t floats, size_t chunk,
                                                                  unsigned layer_len, unsigned layers_end, StepScalars k,
                                                                  const double *__restrict__ partial, int partials, float *__restrict__ norm_out)
{
    __shared__ double red[kStepThreads / 64];
    double p4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = (int)threadIdx.x + u * kStepThreads;             // partials <= 1,024 = 4 x 256
        p4[u] = i < partials ? partial[i] : 0.0;
    }
    const float norm = (float)sqrt(block_sum((p4[0] + p4[1]) + (p4[2] + p4[3]), red));
    if (blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = norm;
    if (!__builtin_isfinite(norm)) return;
    const float c = fminf(1.0f, (1.0f / (norm + 1e-6f)) * k.max_norm);      // the reciprocal first: how torch evaluates max_norm / tensor

    const size_t begin = (size_t)blockIdx.x * chunk, end = begin + chunk < floats ? begin + chunk : floats;
    for (size_t at = begin + 4 * threadIdx.x; at < end; at += kStepGroup) {
        const f4 g0 = load_group(grad, at, floats), p0 = load_group(plain, at, floats);
        const f4 m0 = load_group(exp_avg, at, floats), v0 = load_group(exp_avg_sq, at, floats);
        f4 g, p, m, v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            g[j] = g0[j] * c;
            p[j] = p0[j] * k.decay;
            m[j] = m0[j] + (g[j] - m0[j]) * k.one_minus_beta1;
            v[j] = v0[j] * k.beta2 + (g[j] * g[j]) * k.one_minus_beta2;
            p[j] = p[j] - k.step_size * (m[j] / (sqrtf(v[j]) / k.bc2_sqrt + k.eps));
        }
        // a LayerNorm-eps slot: the last two floats of a layer's block. kEpsBase is a multiple of 4, so a group lies before the
        // layers or from their start on; past the layers (fc) the remainder is below 516 and no layer is that short.
        if (at >= kEpsBase && at < layers_end) {
            const unsigned r = (unsigned)(at - kEpsBase) % layer_len;
            if (r + 5 >= layer_len) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (r + j == layer_len - 2 || r + j == layer_len - 1) {
                        g[j] = g0[j];
                        p[j] = p0[j];
                        m[j] = m0[j];
                        v[j] = v0[j];
                    }
            }
        }
        store_group(grad, at, floats, g);
        store_group(plain, at, floats, p);
        store_group(exp_avg, at, floats, m);
        store_group(exp_avg_sq, at, floats, v);
    }
}

}  // namespace

extern "C" {

size_t g2048_qnet_step_workspace(int dim_ff, int n_layers)
{
    if (!good_encoder_shape(dim_ff, n_layers)) return 0;
    return (step_partials(plain_floats((size_t)dim_ff, (size_t)n_layers)) * sizeof(double) + 15) / 16 * 16;
}

int g2048_qnet_adamw_step(float *plain, float *grad, float *exp_avg, float *exp_avg_sq, int dim_ff, int n_layers, float lr, float beta1,
                          float beta2, float eps, float weight_decay, float max_norm, uint64_t step, float *norm_out, void *workspace,
                          void *stream)
{
    if (!plain || !grad || !exp_avg || !exp_avg_sq || !norm_out || !workspace)
        return fail(G2048_ERR_ARG, "g2048_qnet_adamw_step: null pointer");
    if (!aligned(plain, 16) || !aligned(grad, 16) || !aligned(exp_avg, 16) || !aligned(exp_avg_sq, 16) || !aligned(workspace, 16) ||
        !aligned(norm_out, 4))
        return fail(G2048_ERR_ARG, "g2048_qnet_adamw_step: misaligned pointer (plain weights, grad, exp_avg, exp_avg_sq, workspace: 16 bytes; "
                                   "norm: 4)");
    if (!good_encoder_shape(dim_ff, n_layers))
        return fail(G2048_ERR_ARG, "g2048_qnet_adamw_step: dim_ff must be a multiple of 32 (32 .. 65536) and n_layers 1 .. 64");
    if (step == 0) return fail(G2048_ERR_ARG, "g2048_qnet_adamw_step: step counts the updates from 1");
    if (!good_hyper(lr) || !good_hyper(beta1) || !good_hyper(beta2) || !good_hyper(eps) || !good_hyper(weight_decay))
        return fail(G2048_ERR_ARG, "g2048_qnet_adamw_step: lr, beta1, beta2, eps and weight_decay must be finite and not negative");
    if (beta1 >= 1.0f || beta2 >= 1.0f) return fail(G2048_ERR_ARG, "g2048_qnet_adamw_step: beta1 and beta2 must be below 1");
    if (!(max_norm > 0.0f)) return fail(G2048_ERR_ARG, "g2048_qnet_adamw_step: max_norm must be above 0 (+inf: no clipping)");

    const size_t floats = plain_floats((size_t)dim_ff, (size_t)n_layers), chunk = step_chunk(floats), partials = step_partials(floats);
    const double b1 = decimal_of(beta1), b2 = decimal_of(beta2);
    const double bc1 = 1.0 - pow(b1, (double)step), bc2 = 1.0 - pow(b2, (double)step);
    StepScalars k;
    k.decay = (float)(1.0 - (double)lr * (double)weight_decay);
    k.one_minus_beta1 = (float)(1.0 - b1);
    k.beta2 = beta2;
    k.one_minus_beta2 = (float)(1.0 - b2);
    k.step_size = (float)((double)lr / bc1);
    k.bc2_sqrt = (float)sqrt(bc2);
    k.eps = eps;
    k.max_norm = max_norm;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(workspace);
    hipLaunchKernelGGL(qs_norm_kernel, dim3((unsigned)partials), dim3(kStepThreads), 0, s, static_cast<const float *>(grad), floats, chunk, partial);
    hipLaunchKernelGGL(qs_update_kernel, dim3((unsigned)partials), dim3(kStepThreads), 0, s, plain, grad, exp_avg, exp_avg_sq, floats, chunk,
                       (unsigned)layer_floats((size_t)dim_ff), (unsigned)(kEpsBase + (size_t)n_layers * layer_floats((size_t)dim_ff)), k,
                       static_cast<const double *>(partial), (int)partials, norm_out);
    return check_launch("g2048_qnet_adamw_step");
}

}  // extern "C"
