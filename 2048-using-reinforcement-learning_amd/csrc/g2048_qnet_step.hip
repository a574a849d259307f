// g2048_qnet_step.hip -- what follows the backward pass in DQNAgent.train_step (agents/hybrid.py:1057-1058) for the hybrid agent's
// Q-network on the device: clip_grad_norm_ and AdamW.step() over the whole PLAIN parameter buffer (include/g2048.h,
// g2048_qnet_pack's input) and the gradient buffer g2048_qnet_loss_grad fills, which is laid out like it. C-ABI:
// g2048_qnet_adamw_step / g2048_qnet_step_workspace. Two launches, no host synchronisation:
//   norm     block b adds grad[i]^2 over its chunk of the buffer in a fixed order (sum_squares) and writes ONE partial sum; the
//            chunk is a function of the float count alone (step_chunk), never of the device, and there are at most
//            G2048_QNET_STEP_MAX_PARTIALS of them. Squares, partial sums and the total are f64: a float's square is exact in
//            f64 and the sum of a million of them keeps 1e-6 of the norm with nine digits to spare.
//   update   every block adds ALL partials up again, in the same order, so every block holds the same norm; block 0 writes it
//            out. A norm that is not finite ends the launch there: nothing else is written. Otherwise the block clips and
//            updates its chunk, 16 bytes a lane at a time, by adam_update with the decay of torch's single-tensor AdamW,
//            p = plain (1 - lr wd), and with lr / bc1 and sqrt(bc2) formed on the host from the caller's step number.
//            The two LayerNorm-eps slots of every layer are settings, not parameters: all four buffers keep their bits there.
//            A layer's block is = 2 mod 4 floats long, so the pair is the first half of a 16-byte group in one layer and the
//            second half in the next, and with an odd layer count the buffer ends in a group of two floats.
// No atomics, no block waits on another, nothing depends on the compute-unit count: two calls give the same bits.
#include <hip/hip_runtime.h>

#include "../../include/g2048.h"
#include "g2048_host.h"
#include "g2048_step_common.h"      // the sums, the groups, the chunks, adam_update, keep_eps_slots and the host's scalars

namespace {

using namespace g2048;

constexpr size_t kEpsBase = 139616;                  // the first layer's block starts here (a multiple of 4)
constexpr size_t kFcFloats = 4 * 128 + 4;            // past the layers: below 516 floats, and no layer is that short
static_assert(G2048_QNET_STEP_MAX_PARTIALS == kStepMaxPartials, "the update kernel reads four partial sums a thread");

constexpr size_t layer_floats(size_t ff) { return 66690 + 257 * ff; }
constexpr size_t plain_floats(size_t ff, size_t layers) { return kEpsBase + layers * layer_floats(ff) + kFcFloats; }

// ------------------------------------------------------------------------------------------------------------- norm --
// partial[block] = the sum of grad[i]^2 over the block's chunk: thread t takes the groups t, t + 256, .. of the chunk; then the
// butterfly and the four wavefronts
__global__ __launch_bounds__(kStepThreads) void qs_norm_kernel(const float *__restrict__ grad, size_t floats, size_t chunk,
                                                                double *__restrict__ partial)
{
    __shared__ double red[kStepThreads / 64];
    const size_t begin = (size_t)blockIdx.x * chunk, end = begin + chunk < floats ? begin + chunk : floats;
    const double s = block_sum(sum_squares(grad, begin + 4 * threadIdx.x, end, kStepGroup, floats), red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ----------------------------------------------------------------------------------------------------------- update --
struct StepScalars {
    float decay;
    AdamBetas betas;
    BiasCorrections bc;
    float eps, max_norm;
};

__global__ __launch_bounds__(kStepThreads) void qs_update_kernel(float *__restrict__ plain, float *__restrict__ grad, float *__restrict__ exp_avg,
                                                                  float *__restrict__ exp_avg_sq, size_t floats, size_t chunk,
                                                                  unsigned layer_len, unsigned layers_end, StepScalars k,
                                                                  const double *__restrict__ partial, int partials, float *__restrict__ norm_out)
{
    __shared__ double red[kStepThreads / 64];
    const float norm = (float)sqrt(partials_total(partial, partials, red));
    if (blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = norm;
    if (!__builtin_isfinite(norm)) return;
    const float c = clip_coefficient(norm, k.max_norm);

    const size_t begin = (size_t)blockIdx.x * chunk, end = begin + chunk < floats ? begin + chunk : floats;
    for (size_t at = begin + 4 * threadIdx.x; at < end; at += kStepGroup) {
        const StepGroup in = load_step_group(plain, grad, exp_avg, exp_avg_sq, at, floats);
        StepGroup out = adam_update<true>(in, c, k.decay, k.betas, k.bc, k.eps);
        keep_eps_slots(out, in, at, kEpsBase, layers_end, layer_len);
        store_step_group(plain, grad, exp_avg, exp_avg_sq, at, floats, out);
    }
}

}  // namespace

extern "C" {

size_t g2048_qnet_step_workspace(int dim_ff, int n_layers)
{
    if (!good_encoder_shape(dim_ff, n_layers)) return 0;
    return step_partial_bytes(plain_floats((size_t)dim_ff, (size_t)n_layers));
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
    const float lr_eps[2] = {lr, eps};
    if (const char *defect = adam_hyper_defect(lr_eps, 2, beta1, beta2, &weight_decay, max_norm))
        return fail(G2048_ERR_ARG, "g2048_qnet_adamw_step: %s", defect);

    const size_t floats = plain_floats((size_t)dim_ff, (size_t)n_layers), chunk = step_chunk(floats), partials = step_partials(floats);
    const BetaScalars b = beta_scalars(beta1, beta2);
    StepScalars k;
    k.decay = (float)(1.0 - (double)lr * (double)weight_decay);
    k.betas = b.update;
    k.bc = bias_corrections((double)lr, b.beta1, b.beta2, (double)step);
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
