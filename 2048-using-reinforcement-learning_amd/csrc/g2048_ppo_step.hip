// g2048_ppo_step.hip -- what follows backward() in an epoch of PPOAgent.update (agents/ppo_agent.py:403-416) for the actor and the
// critic together, on the device: the NaN check on the loss, clip_grad_norm_ per network and an Adam step per network over the two
// PLAIN parameter buffers (include/g2048.h) and the gradient buffers g2048_ppo_loss_grad fills. C-ABI: g2048_ppo_adam_step /
// g2048_ppo_step_workspace. Two launches, no host synchronisation and no host decision:
//   prepare  ONE block of 1,024 threads. Thread t adds grad[i]^2 over the 16-byte groups t, t + 1,024, .. of a buffer in order
//            (sum_squares); then the butterfly and the sixteen wavefronts' sums, pairwise: the order depends on the float count
//            alone. Thread 0 reads the loss and the counters, decides whether the call applies, forms both clip coefficients and,
//            in f64 from the network's OWN applied-step counter, lr / bc1 and sqrt(bc2), writes them to the workspace, the norms
//            to norms_out and the counters back. Nothing else reads the counters in that launch.
//   update   both networks in one grid, a 16-byte group a lane. Every block reads the prepared scalars and returns at once on a
//            skip. Otherwise adam_update without weight decay.
//            The critic's buffers are = 1 mod 4 floats long: their last group is one float.
// No atomics, no block waits on another, nothing depends on the compute-unit count: two calls give the same bits.
#include "../../include/g2048.h"
#include "g2048_host.h"
#include "g2048_step_common.h"      // the sums, the groups, adam_update, the gates' pieces and the host's scalars

namespace {

using namespace g2048;

constexpr size_t kActorFloats = 46272 + 65 * 4, kCriticFloats = 46272 + 65 * 1;
constexpr int kPrepThreads = 1024, kPrepWaves = kPrepThreads / 64;
constexpr unsigned kActorBlocks = (unsigned)((kActorFloats + kStepGroup - 1) / kStepGroup);
constexpr unsigned kCriticBlocks = (unsigned)((kCriticFloats + kStepGroup - 1) / kStepGroup);
static_assert(kActorFloats % 4 == 0 && kCriticFloats % 4 == 1, "the critic's buffers end in a group of one float");

// what the prepare launch leaves in the workspace for the update launch
struct Prepared {
    int apply;                      // 0: the call is skipped, nothing is written
    float clip[2], step_size[2], bc2_sqrt[2];        // actor, critic
};

struct PrepScalars {
    double beta1, beta2, lr[2];     // the betas as the decimals their caller wrote; lr as the f32 given
    float max_norm;
};

// sum of grad[i]^2 over one buffer by the whole block, the same on every thread
__device__ inline double prep_sum(const float *__restrict__ grad, size_t floats, double (&red)[kPrepWaves])
{
    const double w = wave_sum(sum_squares(grad, 4 * (size_t)threadIdx.x, floats, 4 * (size_t)kPrepThreads, floats));
    __syncthreads();                                                   // red may still be read from the buffer before
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
    __syncthreads();
    double s[kPrepWaves];
#pragma unroll
    for (int i = 0; i < kPrepWaves; ++i) s[i] = red[i];
#pragma unroll
    for (int n = kPrepWaves / 2; n > 0; n >>= 1)
#pragma unroll
        for (int i = 0; i < n; ++i) s[i] = s[2 * i] + s[2 * i + 1];
    return s[0];
}

__global__ __launch_bounds__(kPrepThreads) void ps_prepare_kernel(const float *__restrict__ grad_actor, const float *__restrict__ grad_critic,
                                                                  const float *__restrict__ loss_or_null, long long *__restrict__ counters,
                                                                  PrepScalars k, float *__restrict__ norms_out, Prepared *__restrict__ prepared)
{
    __shared__ double red[kPrepWaves];
    const float norm_a = (float)sqrt(prep_sum(grad_actor, kActorFloats, red));
    const float norm_c = (float)sqrt(prep_sum(grad_critic, kCriticFloats, red));
    if (threadIdx.x != 0) return;
    norms_out[0] = norm_a;
    norms_out[1] = norm_c;
    Prepared out;
    out.apply = 0;
    out.clip[0] = out.clip[1] = out.step_size[0] = out.step_size[1] = out.bc2_sqrt[0] = out.bc2_sqrt[1] = 0.0f;
    if (nan_loss(loss_or_null)) {
        counters[2] += 1;
    } else if (!__builtin_isfinite(norm_a) || !__builtin_isfinite(norm_c)) {
        counters[3] += 1;
    } else {
        out.apply = 1;
        const float norm[2] = {norm_a, norm_c};
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const long long t = counters[n] + 1;                       // this network's step number: skipped calls never counted
            counters[n] = t;
            const BiasCorrections bc = bias_corrections(k.lr[n], k.beta1, k.beta2, (double)t);
            out.clip[n] = clip_coefficient(norm[n], k.max_norm);
            out.step_size[n] = bc.step_size;
            out.bc2_sqrt[n] = bc.bc2_sqrt;
        }
    }
    *prepared = out;
}

struct UpdateScalars {
    AdamBetas betas;
    float eps[2];
};

struct NetBuffers {
    float *plain, *grad, *exp_avg, *exp_avg_sq;
};

__global__ __launch_bounds__(kStepThreads) void ps_update_kernel(NetBuffers actor, NetBuffers critic, UpdateScalars k,
                                                                 const Prepared *__restrict__ prepared)
{
    if (!prepared->apply) return;
    const bool is_critic = blockIdx.x >= kActorBlocks;
    const int n = is_critic ? 1 : 0;
    const NetBuffers b = is_critic ? critic : actor;
    const size_t floats = is_critic ? kCriticFloats : kActorFloats;
    const size_t at = ((size_t)(blockIdx.x - (is_critic ? kActorBlocks : 0u)) * kStepThreads + threadIdx.x) * 4;
    if (at >= floats) return;
    const float c = prepared->clip[n], eps = k.eps[n];
    const BiasCorrections bc = {prepared->step_size[n], prepared->bc2_sqrt[n]};
    const StepGroup in = load_step_group(b.plain, b.grad, b.exp_avg, b.exp_avg_sq, at, floats);
    store_step_group(b.plain, b.grad, b.exp_avg, b.exp_avg_sq, at, floats, adam_update<false>(in, c, 1.0f, k.betas, bc, eps));
}

}  // namespace

extern "C" {

size_t g2048_ppo_step_workspace(void) { return (sizeof(Prepared) + 15) / 16 * 16; }

int g2048_ppo_adam_step(float *plain_actor, float *grad_actor, float *exp_avg_actor, float *exp_avg_sq_actor, float *plain_critic,
                        float *grad_critic, float *exp_avg_critic, float *exp_avg_sq_critic, const float *loss_or_null, int64_t *counters,
                        float lr_actor, float lr_critic, float beta1, float beta2, float eps_actor, float eps_critic, float max_norm,
                        float *norms_out, void *workspace, void *stream)
{
    if (!plain_actor || !grad_actor || !exp_avg_actor || !exp_avg_sq_actor || !plain_critic || !grad_critic || !exp_avg_critic ||
        !exp_avg_sq_critic || !counters || !norms_out || !workspace)
        return fail(G2048_ERR_ARG, "g2048_ppo_adam_step: null pointer");
    if (!aligned(plain_actor, 16) || !aligned(grad_actor, 16) || !aligned(exp_avg_actor, 16) || !aligned(exp_avg_sq_actor, 16) ||
        !aligned(plain_critic, 16) || !aligned(grad_critic, 16) || !aligned(exp_avg_critic, 16) || !aligned(exp_avg_sq_critic, 16) ||
        !aligned(workspace, 16) || !aligned(counters, 8) || !aligned(norms_out, 4) || !aligned(loss_or_null, 4))
        return fail(G2048_ERR_ARG, "g2048_ppo_adam_step: misaligned pointer (plain weights, grad, exp_avg, exp_avg_sq, workspace: 16 bytes; "
                                   "counters: 8; loss, norms: 4)");
    const float lr_eps[4] = {lr_actor, lr_critic, eps_actor, eps_critic};
    if (const char *defect = adam_hyper_defect(lr_eps, 4, beta1, beta2, nullptr, max_norm))
        return fail(G2048_ERR_ARG, "g2048_ppo_adam_step: %s", defect);

    const BetaScalars b = beta_scalars(beta1, beta2);
    PrepScalars ps;
    ps.beta1 = b.beta1;
    ps.beta2 = b.beta2;
    ps.lr[0] = (double)lr_actor;
    ps.lr[1] = (double)lr_critic;
    ps.max_norm = max_norm;
    UpdateScalars us;
    us.betas = b.update;
    us.eps[0] = eps_actor;
    us.eps[1] = eps_critic;
    hipStream_t s = static_cast<hipStream_t>(stream);
    Prepared *prepared = static_cast<Prepared *>(workspace);
    hipLaunchKernelGGL(ps_prepare_kernel, dim3(1), dim3(kPrepThreads), 0, s, static_cast<const float *>(grad_actor),
                       static_cast<const float *>(grad_critic), loss_or_null, reinterpret_cast<long long *>(counters), ps, norms_out, prepared);
    hipLaunchKernelGGL(ps_update_kernel, dim3(kActorBlocks + kCriticBlocks), dim3(kStepThreads), 0, s,
                       NetBuffers{plain_actor, grad_actor, exp_avg_actor, exp_avg_sq_actor},
                       NetBuffers{plain_critic, grad_critic, exp_avg_critic, exp_avg_sq_critic}, us, static_cast<const Prepared *>(prepared));
    return check_launch("g2048_ppo_adam_step");
}

}  // extern "C"
