// g2048_tpolicy_step.hip -- what follows backward() in an epoch of PPOAgent.update (agents/ppo_agent.py:403-416) for the transformer
// policy on the device: the NaN check on the loss, clip_grad_norm_ and an Adam step over the whole PLAIN parameter buffer
// (include/g2048.h, g2048_tpolicy_pack's input) and the gradient buffer g2048_tpolicy_loss_grad fills, which is laid out like it.
// C-ABI (include/g2048_tstep.h, libg2048_tstep_hip.so): g2048_tpolicy_adam_step / g2048_tpolicy_step_workspace. Three launches, no
// host synchronisation and no host decision:
//   norm     block b adds grad[i]^2 over its chunk of the buffer in a fixed order and writes ONE f64 partial sum; the chunk is a
//            function of the float count alone (step_chunk, the Q-network's rule), never of the device, and there are at most
//            kMaxPartials of them. The last 16-byte group is short: 1 float with an even layer count, 3 with an odd one.
//   prepare  ONE block adds the partials up, four a thread, then the butterfly and the four wavefronts: the order depends on the
//            float count alone. Thread 0 writes the norm out, reads the loss and the counters, decides whether the call applies,
//            forms the clip coefficient and, in f64 from the applied-step counter, lr / bc1 and sqrt(bc2), and writes them to the
//            workspace and the counters back. Nothing else reads or writes the counters in that launch.
//   update   a 16-byte group a lane. Every block reads the prepared scalars, which no block of that launch writes, and returns at
//            once on a skip. Otherwise the lines of g2048_ppo_step.hip's update, every operation rounded to f32 on its own
//            (-ffp-contract=off):
//              g = grad c;  m += (g - m)(1 - beta1);  v = v beta2 + (g g)(1 - beta2);  p -= (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
//            The two LayerNorm-eps slots of every layer are settings, not parameters: all four buffers keep their bits there.
//            The layers start at float 128 and a layer's block is = 2 mod 4 floats long, so the pair is the first half of a
//            16-byte group in layers 0, 2, .. and the second half in layers 1, 3, ...
// No atomics, no block waits on another, no block reads a word another block of its launch writes, nothing depends on the
// compute-unit count: two calls give the same bits.
#include <hip/hip_runtime.h>

#include "../../include/g2048_tstep.h"
#include "g2048_host.h"
#include "g2048_step_common.h"      // wave_sum, block_sum, load_group, store_group, decimal_of, good_hyper
#include "g2048_tpolicy_layout.h"   // kPlainLayer0, pl_layer, kPlTail

namespace {

using namespace g2048;

constexpr size_t kEpsBase = kPlainLayer0;            // the first layer's block starts here (a multiple of 4)
constexpr size_t kMaxPartials = 4 * kStepThreads;    // the prepare launch reads four partial sums a thread
static_assert(kEpsBase % 4 == 0 && pl_layer(32) % 4 == 2 && pl_layer(64) % 4 == 2 && kPlTail % 4 == 1,
              "a layer's block is = 2 mod 4 floats long and the buffer ends in a group of 1 or 3 floats");

constexpr size_t plain_floats(size_t ff, size_t layers) { return kEpsBase + layers * (size_t)pl_layer((int)ff) + (size_t)kPlTail; }

// floats a block owns: the buffer in at most kMaxPartials equal chunks, whole passes of 1,024 floats
constexpr size_t step_chunk(size_t floats)
{
    const size_t per = (floats + kMaxPartials - 1) / kMaxPartials;
    return (per + kStepGroup - 1) / kStepGroup * kStepGroup;
}
constexpr size_t step_partials(size_t floats) { return (floats + step_chunk(floats) - 1) / step_chunk(floats); }
constexpr size_t partial_bytes(size_t floats) { return (step_partials(floats) * sizeof(double) + 15) / 16 * 16; }

// what the prepare launch leaves in the workspace, behind the partial sums, for the update launch
struct Prepared {
    int apply;                      // 0: the call is skipped, nothing is written
    float clip, step_size, bc2_sqrt;
};
static_assert(sizeof(Prepared) == 16, "the workspace ends in one 16-byte record");

// ------------------------------------------------------------------------------------------------------------- norm --
// partial[block] = the sum of grad[i]^2 over the block's chunk: thread t takes the groups t, t + 256, .. of the chunk in order, one
// f64 sum a vector component, combined pairwise; then the butterfly and the four wavefronts
__global__ __launch_bounds__(kStepThreads) void ts_norm_kernel(const float *__restrict__ grad, size_t floats, size_t chunk,
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
    double p4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = (int)threadIdx.x + u * kStepThreads;             // partials <= 1,024 = 4 x 256
        p4[u] = i < partials ? partial[i] : 0.0;
    }
    const float norm = (float)sqrt(block_sum((p4[0] + p4[1]) + (p4[2] + p4[3]), red));
    if (threadIdx.x != 0) return;
    norm_out[0] = norm;
    Prepared out;
    out.apply = 0;
    out.clip = out.step_size = out.bc2_sqrt = 0.0f;
    bool nan_loss = false;
    if (loss_or_null) {
        const float loss = loss_or_null[0];
        nan_loss = loss != loss;                                       // isnan only, the reference's rule: +inf is applied
    }
    if (nan_loss) {
        counters[1] += 1;
    } else if (!__builtin_isfinite(norm)) {
        counters[2] += 1;
    } else {
        out.apply = 1;
        const long long t = counters[0] + 1;                           // Adam's step number: skipped calls never counted
        counters[0] = t;
        const double bc1 = 1.0 - pow(k.beta1, (double)t), bc2 = 1.0 - pow(k.beta2, (double)t);
        out.clip = fminf(1.0f, (1.0f / (norm + 1e-6f)) * k.max_norm);  // the reciprocal first: how torch evaluates max_norm / tensor
        out.step_size = (float)(k.lr / bc1);
        out.bc2_sqrt = (float)sqrt(bc2);
    }
    *prepared = out;
}

// ----------------------------------------------------------------------------------------------------------- update --
struct UpdateScalars {
    float one_minus_beta1, beta2, one_minus_beta2, eps;
};

__global__ __launch_bounds__(kStepThreads) void ts_update_kernel(float *__restrict__ plain, float *__restrict__ grad, float *__restrict__ exp_avg,
                                                                  float *__restrict__ exp_avg_sq, size_t floats, unsigned layer_len,
                                                                  unsigned layers_end, UpdateScalars k, const Prepared *__restrict__ prepared)
{
    if (!prepared->apply) return;
    const size_t at = ((size_t)blockIdx.x * kStepThreads + threadIdx.x) * 4;
    if (at >= floats) return;
    const float c = prepared->clip, step_size = prepared->step_size, bc2_sqrt = prepared->bc2_sqrt;
    const f4 g0 = load_group(grad, at, floats), p0 = load_group(plain, at, floats);
    const f4 m0 = load_group(exp_avg, at, floats), v0 = load_group(exp_avg_sq, at, floats);
    f4 g, p, m, v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        g[j] = g0[j] * c;
        m[j] = m0[j] + (g[j] - m0[j]) * k.one_minus_beta1;
        v[j] = v0[j] * k.beta2 + (g[j] * g[j]) * k.one_minus_beta2;
        p[j] = p0[j] - step_size * (m[j] / (sqrtf(v[j]) / bc2_sqrt + k.eps));
    }
    // a LayerNorm-eps slot: the last two floats of a layer's block. kEpsBase is a multiple of 4, so a group lies before the layers
    // or from their start on; past the layers (fc1 on) the group is not looked at.
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

}  // namespace

extern "C" {

const char *g2048_tstep_last_error(void) { return g_err; }

int g2048_tstep_abi_version(void) { return G2048_TSTEP_ABI_VERSION; }

size_t g2048_tpolicy_step_workspace(int dim_ff, int n_layers)
{
    if (!good_encoder_shape(dim_ff, n_layers)) return 0;
    return partial_bytes(plain_floats((size_t)dim_ff, (size_t)n_layers)) + sizeof(Prepared);
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
    if (!good_hyper(lr) || !good_hyper(beta1) || !good_hyper(beta2) || !good_hyper(eps))
        return fail(G2048_ERR_ARG, "g2048_tpolicy_adam_step: lr, beta1, beta2 and eps must be finite and not negative");
    if (beta1 >= 1.0f || beta2 >= 1.0f) return fail(G2048_ERR_ARG, "g2048_tpolicy_adam_step: beta1 and beta2 must be below 1");
    if (!(max_norm > 0.0f)) return fail(G2048_ERR_ARG, "g2048_tpolicy_adam_step: max_norm must be above 0 (+inf: no clipping)");
    const size_t need = g2048_tpolicy_step_workspace(dim_ff, n_layers);
    if (workspace_bytes < need)
        return fail(G2048_ERR_ARG, "g2048_tpolicy_adam_step: workspace of %zu bytes, g2048_tpolicy_step_workspace(dim_ff, n_layers) is %zu",
                    workspace_bytes, need);

    const size_t floats = plain_floats((size_t)dim_ff, (size_t)n_layers), chunk = step_chunk(floats), partials = step_partials(floats);
    const double b1 = decimal_of(beta1), b2 = decimal_of(beta2);
    PrepScalars ps;
    ps.beta1 = b1;
    ps.beta2 = b2;
    ps.lr = (double)lr;
    ps.max_norm = max_norm;
    UpdateScalars us;
    us.one_minus_beta1 = (float)(1.0 - b1);
    us.beta2 = beta2;
    us.one_minus_beta2 = (float)(1.0 - b2);
    us.eps = eps;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(workspace);
    Prepared *prepared = reinterpret_cast<Prepared *>(static_cast<char *>(workspace) + partial_bytes(floats));
    const size_t layer_len = (size_t)pl_layer(dim_ff);
    hipLaunchKernelGGL(ts_norm_kernel, dim3((unsigned)partials), dim3(kStepThreads), 0, s, static_cast<const float *>(grad), floats, chunk, partial);
    hipLaunchKernelGGL(ts_prepare_kernel, dim3(1), dim3(kStepThreads), 0, s, static_cast<const double *>(partial), (int)partials, loss_or_null,
                       reinterpret_cast<long long *>(counters3), ps, norm_out, prepared);
    hipLaunchKernelGGL(ts_update_kernel, dim3(blocks_for(floats, kStepGroup)), dim3(kStepThreads), 0, s, plain, grad, exp_avg, exp_avg_sq, floats,
                       (unsigned)layer_len, (unsigned)(kEpsBase + (size_t)n_layers * layer_len), us, static_cast<const Prepared *>(prepared));
    return check_launch("g2048_tpolicy_adam_step");
}

}  // extern "C"
