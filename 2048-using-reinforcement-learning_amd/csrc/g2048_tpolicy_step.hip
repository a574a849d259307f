// g2048_tpolicy_step.hip -- what follows backward() in an epoch of PPOAgent.update (agents/ppo_agent.py:403-416) for the transformer
// policy on the device: the NaN check on the loss, clip_grad_norm_ and an Adam step over the whole PLAIN parameter buffer
// (include/g2048.h, g2048_tpolicy_pack's input) and the gradient buffer g2048_tpolicy_loss_grad fills, which is laid out like it.
// C-ABI (include/g2048_tstep.h, libg2048_tstep_hip.so): g2048_tpolicy_adam_step / g2048_tpolicy_step_workspace. Three launches, no
// host synchronisation and no host decision:
//   norm     block b adds grad[i]^2 over its chunk of the buffer in a fixed order (sum_squares) and writes ONE f64 partial sum;
//            the chunk is a function of the float count alone (step_chunk, the Q-network's rule), never of the device, and there
//            are at most kStepMaxPartials of them. The last 16-byte group is short: 1 float with an even layer count, 3 with an
//            odd one.
//   prepare  ONE block adds the partials up (partials_total): the order depends on the float count alone. Thread 0 writes the norm
//            out, reads the loss and the counters, decides whether the call applies, forms the clip coefficient and, in f64 from
//            the applied-step counter, lr / bc1 and sqrt(bc2), and writes them to the workspace and the counters back. Nothing
//            else reads or writes the counters in that launch.
//   update   a 16-byte group a lane. Every block reads the prepared scalars, which no block of that launch writes, and returns at
//            once on a skip. Otherwise adam_update without weight decay.
//            The two LayerNorm-eps slots of every layer are settings, not parameters: all four buffers keep their bits there.
//            The layers start at float 128 and a layer's block is = 2 mod 4 floats long, so the pair is the first half of a
//            16-byte group in layers 0, 2, .. and the second half in layers 1, 3, ...
// No atomics, no block waits on another, no block reads a word another block of its launch writes, nothing depends on the
// compute-unit count: two calls give the same bits.
#include <hip/hip_runtime.h>

#include "../../include/g2048_tstep.h"
#include "g2048_host.h"
#include "g2048_step_common.h"      // the sums, the groups, the chunks, adam_update, keep_eps_slots, the gates' pieces, the host's scalars
#include "g2048_tpolicy_layout.h"   // kPlainLayer0, pl_layer, kPlTail

namespace {

using namespace g2048;

constexpr size_t kEpsBase = kPlainLayer0;            // the first layer's block starts here (a multiple of 4)
static_assert(kEpsBase % 4 == 0 && pl_layer(32) % 4 == 2 && pl_layer(64) % 4 == 2 && kPlTail % 4 == 1,
              "a layer's block is = 2 mod 4 floats long and the buffer ends in a group of 1 or 3 floats");

constexpr size_t plain_floats(size_t ff, size_t layers) { return kEpsBase + layers * (size_t)pl_layer((int)ff) + (size_t)kPlTail; }

// what the prepare launch leaves in the workspace, behind the partial sums, for the update launch
struct Prepared {
    int apply;                      // 0: the call is skipped, nothing is written
    float clip;
    BiasCorrections bc;
};
static_assert(sizeof(Prepared) == 16, "the workspace ends in one 16-byte record");

// ------------------------------------------------------------------------------------------------------------- norm --
// partial[block] = the sum of grad[i]^2 over the block's chunk: thread t takes the groups t, t + 256, .. of the chunk; then the
// butterfly and the four wavefronts
__global__ __launch_bounds__(kStepThreads) void ts_norm_kernel(const float *__restrict__ grad, size_t floats, size_t chunk,
                                                                double *__restrict__ partial)
{
    __shared__ double red[kStepThreads / 64];
    const size_t begin = (size_t)blockIdx.x * chunk, end = begin + chunk < floats ? begin + chunk : floats;
    const double s = block_sum(sum_squares(grad, begin + 4 * threadIdx.x, end, kStepGroup, floats), red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ---------------------------------------------------------------------------------------------------------- prepare --
struct PrepScalars {
    double beta1, beta2, lr;        // the betas as the decimals their caller wrote; lr as the f32 given
    float max_norm;
};

__global__ __launch_bounds__(kStepThreads) void ts_prepare_kernel(const double *__restrict__ partial, int partials,
                                                                   const float *__restrict__ loss_or_null, long long *__restrict__ counters,
                                                                   PrepScalars k, float *__restrict__ norm_out, Prepared *__restrict__ prepared)
{
    __shared__ double red[kStepThreads / 64];
    const float norm = (float)sqrt(partials_total(partial, partials, red));
    if (threadIdx.x != 0) return;
    norm_out[0] = norm;
    Prepared out;
    out.apply = 0;
    out.clip = out.bc.step_size = out.bc.bc2_sqrt = 0.0f;
    if (nan_loss(loss_or_null)) {
        counters[1] += 1;
    } else if (!__builtin_isfinite(norm)) {
        counters[2] += 1;
    } else {
        out.apply = 1;
        const long long t = counters[0] + 1;                           // Adam's step number: skipped calls never counted
        counters[0] = t;
        out.clip = clip_coefficient(norm, k.max_norm);
        out.bc = bias_corrections(k.lr, k.beta1, k.beta2, (double)t);
    }
    *prepared = out;
}

// ----------------------------------------------------------------------------------------------------------- update --
struct UpdateScalars {
    AdamBetas betas;
    float eps;
};

__global__ __launch_bounds__(kStepThreads) void ts_update_kernel(float *__restrict__ plain, float *__restrict__ grad, float *__restrict__ exp_avg,
                                                                  float *__restrict__ exp_avg_sq, size_t floats, unsigned layer_len,
                                                                  unsigned layers_end, UpdateScalars k, const Prepared *__restrict__ prepared)
{
    if (!prepared->apply) return;
    const size_t at = ((size_t)blockIdx.x * kStepThreads + threadIdx.x) * 4;
    if (at >= floats) return;
    const StepGroup in = load_step_group(plain, grad, exp_avg, exp_avg_sq, at, floats);
    StepGroup out = adam_update<false>(in, prepared->clip, 1.0f, k.betas, prepared->bc, k.eps);
    keep_eps_slots(out, in, at, kEpsBase, layers_end, layer_len);
    store_step_group(plain, grad, exp_avg, exp_avg_sq, at, floats, out);
}

}  // namespace

extern "C" {

const char *g2048_tstep_last_error(void) { return g_err; }

int g2048_tstep_abi_version(void) { return G2048_TSTEP_ABI_VERSION; }

size_t g2048_tpolicy_step_workspace(int dim_ff, int n_layers)
{
    if (!good_encoder_shape(dim_ff, n_layers)) return 0;
    return step_partial_bytes(plain_floats((size_t)dim_ff, (size_t)n_layers)) + sizeof(Prepared);
}

int g2048_tpolicy_adam_step(float *plain, float *grad, float *exp_avg, float *exp_avg_sq, int dim_ff, int n_layers,
                            const float *loss_or_null, int64_t *counters3, float lr, float beta1, float beta2, float eps, float max_norm,
                            float *norm_out, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!plain || !grad || !exp_avg || !exp_avg_sq || !counters3 || !norm_out || !workspace)
        return fail(G2048_ERR_ARG, "g2048_tpolicy_adam_step: null pointer");
    if (!aligned(plain, 16) || !aligned(grad, 16) || !aligned(exp_avg, 16) || !aligned(exp_avg_sq, 16) || !aligned(workspace, 16) ||
        !aligned(counters3, 8) || !aligned(norm_out, 4) || !aligned(loss_or_null, 4))
        return fail(G2048_ERR_ARG, "g2048_tpolicy_adam_step: misaligned pointer (plain weights, grad, exp_avg, exp_avg_sq, workspace: 16 "
                                   "bytes; counters: 8; loss, norm: 4)");
    if (!good_encoder_shape(dim_ff, n_layers))
        return fail(G2048_ERR_ARG, "g2048_tpolicy_adam_step: dim_ff must be a multiple of 32 (32 .. 65536) and n_layers 1 .. 64");
    const float lr_eps[2] = {lr, eps};
    if (const char *defect = adam_hyper_defect(lr_eps, 2, beta1, beta2, nullptr, max_norm))
        return fail(G2048_ERR_ARG, "g2048_tpolicy_adam_step: %s", defect);
    const size_t need = g2048_tpolicy_step_workspace(dim_ff, n_layers);
    if (workspace_bytes < need)
        return fail(G2048_ERR_ARG, "g2048_tpolicy_adam_step: workspace of %zu bytes, g2048_tpolicy_step_workspace(dim_ff, n_layers) is %zu",
                    workspace_bytes, need);

    const size_t floats = plain_floats((size_t)dim_ff, (size_t)n_layers), chunk = step_chunk(floats), partials = step_partials(floats);
    const BetaScalars b = beta_scalars(beta1, beta2);
    PrepScalars ps;
    ps.beta1 = b.beta1;
    ps.beta2 = b.beta2;
    ps.lr = (double)lr;
    ps.max_norm = max_norm;
    UpdateScalars us;
    us.betas = b.update;
    us.eps = eps;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(workspace);
    Prepared *prepared = reinterpret_cast<Prepared *>(static_cast<char *>(workspace) + step_partial_bytes(floats));
    const size_t layer_len = (size_t)pl_layer(dim_ff);
    hipLaunchKernelGGL(ts_norm_kernel, dim3((unsigned)partials), dim3(kStepThreads), 0, s, static_cast<const float *>(grad), floats, chunk, partial);
    hipLaunchKernelGGL(ts_prepare_kernel, dim3(1), dim3(kStepThreads), 0, s, static_cast<const double *>(partial), (int)partials, loss_or_null,
                       reinterpret_cast<long long *>(counters3), ps, norm_out, prepared);
    hipLaunchKernelGGL(ts_update_kernel, dim3(blocks_for(floats, kStepGroup)), dim3(kStepThreads), 0, s, plain, grad, exp_avg, exp_avg_sq, floats,
                       (unsigned)layer_len, (unsigned)(kEpsBase + (size_t)n_layers * layer_len), us, static_cast<const Prepared *>(prepared));
    return check_launch("g2048_tpolicy_adam_step");
}

}  // extern "C"
