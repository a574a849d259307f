// g2048_qnet_batch.hip -- the hybrid agent's Q-network (agents/hybrid.py:700-727, HybridDQN, eval mode) on a BATCH of boards as the
// reference's train_step calls it (:1038-1046): the encoder layer is not batch_first and is fed x.unsqueeze(1), so the n boards
// are ONE sequence of n tokens that attend to each other (8 heads of 16, scores q.k / 4, softmax over all n keys). This is a
// different function from g2048_qnet_forward's (every board its own sequence of one token); they agree at n = 1. With it, the
// no-gradient block of train_step: the online network's argmax, the target network's Q at it and the Double-DQN target
// (g2048_dqn_targets). C-ABI: include/g2048.h, g2048_qnet_forward_batch / g2048_qnet_batch_workspace / g2048_dqn_targets. The kernels,
// the workspace (FwdWorkspace) and the launch sequence (qb_forward_pass<kDrop>) are g2048_qnet_batch_fwd.h's, shared with the gradient
// pass and the training library; this file keeps the entry points and g2048_dqn_targets.
//
// Shape of the work. n is small (the reference's batch is 256), so the pass is a short sequence of launches, one phase each,
// every phase's grid spread over board tiles x feature tiles (or query tiles x heads); between phases the activations lie
// row-major [board][feature] in the caller's workspace. 2 + 5 n_layers launches:
//   conv      conv1 + ReLU + conv2 + ReLU on the VALU, one block a board -> feat [n][1024] (feature = channel * 16 + position)
//   linear    Y = act(X W^T + b) on the f32 matrix cores, one wavefront a 16-board x 16-feature tile: the embedding (K 1024),
//             in_proj whole (Q, K, V: 384 outputs), linear1 + ReLU
//   attention one wavefront a (16-query tile, head): the key tiles streamed with an online softmax (running maximum subtracted,
//             keys past n masked out of the maximum and the sum, their V rows read as zero); scores and P.V on the matrix cores
//   proj_norm x = LayerNorm(x + H W^T + b), a block of eight wavefronts a 16-board tile, one wavefront a 16-feature tile of the
//             product, the 16 x 128 tile through LDS, then one wavefront two boards' statistics: out_proj + norm1 (K 128) and
//             linear2 + norm2 (K dim_ff); the last one computes fc on the normalised rows and writes Q instead of x
// Weights are read from the PLAIN f32 buffer (g2048_qnet_pack's input, state-dict order) as they lie: with boards as the MFMA N
// dimension a lane's A operand over 16 input features is the 16 bytes W[row][16 c + 4 g ..], one load from the row-major matrix.
// There is no second blob, and DeviceQNetwork.refresh() refreshes this path by refreshing `plain`. A layer's parameters start at
// an odd multiple of 8 bytes (two eps floats per layer), hence the 4-byte-aligned vector type of the weight loads.
// f32 only: the first layer's logits reach 1e9 on tile values up to 131,072 and its softmax is nearly one-hot; bf16 logits would
// pick keys at random. Every output element is one wavefront's fixed-order accumulation: no split-K, no atomics, so a call is
// bit-repeatable; rows past n are neither read nor written. No cooperative launch, no block waits on another: phase boundaries
// are launch boundaries. Compile with -ffp-contract=off (g2048_dqn_targets follows torch's operation order).
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/g2048.h"
#include "g2048_host.h"
#include "g2048_mfma.h"
#include "g2048_qnet_batch_fwd.h"

namespace {

// ------------------------------------------------------------------------------------------------------ dqn targets --
// hybrid.py:1042-1046 on given Q: next_action = argmax of the online Q (unmasked, first maximum), next_q = the target Q at it,
// target = shaped + (1 - done) * gamma * next_q in torch's order of operations, every step rounded to f32, no contraction.
__global__ __launch_bounds__(256) void dqn_targets_kernel(const float4 *__restrict__ q_online, const float4 *__restrict__ q_target,
                                                           const float *__restrict__ shaped, const float *__restrict__ dones, float gamma,
                                                           long long *__restrict__ next_actions, float *__restrict__ targets, int n)
{
#pragma clang fp contract(off)
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    const float4 qo = q_online[i], qt = q_target[i];
    const float o[4] = {qo.x, qo.y, qo.z, qo.w}, tq[4] = {qt.x, qt.y, qt.z, qt.w};
    int a = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (o[k] > o[a]) a = k;
    float t = (1.0f - dones[i]) * gamma;
    t = t * tq[a];
    next_actions[i] = a;
    targets[i] = shaped[i] + t;
}

}  // namespace

extern "C" {

size_t g2048_qnet_batch_workspace(size_t n, int dim_ff)
{
    if (n == 0 || n > G2048_QNET_BATCH_MAX || !good_encoder_shape(dim_ff, 1)) return 0;
    return FwdWorkspace(n, dim_ff).floats() * sizeof(float);
}

int g2048_qnet_forward_batch(const void *boards, const float *plain_f32, float *q_out, size_t n, int dim_ff, int n_layers,
                             void *workspace, void *stream)
{
    return qb_forward_pass<false>("g2048_qnet_forward_batch", QbCall{boards, plain_f32, nullptr, nullptr, nullptr, n, dim_ff, n_layers, nullptr,
                                                                     nullptr, nullptr, q_out, workspace, stream, false, nullptr, 0, 0});
}

int g2048_dqn_targets(const float *q_online_next, const float *q_target_next, const float *shaped, const float *dones, float gamma,
                      int64_t *next_actions_out, float *targets_out, size_t n, void *stream)
{
    if (n == 0) return G2048_OK;
    if (!q_online_next || !q_target_next || !shaped || !dones || !next_actions_out || !targets_out)
        return fail(G2048_ERR_ARG, "g2048_dqn_targets: null pointer");
    if (!aligned(q_online_next, 16) || !aligned(q_target_next, 16) || !aligned(shaped, 4) || !aligned(dones, 4) ||
        !aligned(next_actions_out, 8) || !aligned(targets_out, 4))
        return fail(G2048_ERR_ARG, "g2048_dqn_targets: misaligned pointer (the two Q: 16 bytes; actions: 8; the rest: 4)");
    if (!std::isfinite(gamma)) return fail(G2048_ERR_ARG, "g2048_dqn_targets: gamma must be finite");
    if (n > 0x7fffffffu) return fail(G2048_ERR_ARG, "g2048_dqn_targets: n too large for one launch");
    hipLaunchKernelGGL(dqn_targets_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4 *>(q_online_next), reinterpret_cast<const float4 *>(q_target_next), shaped, dones, gamma,
                       reinterpret_cast<long long *>(next_actions_out), targets_out, (int)n);
    return check_launch("g2048_dqn_targets");
}

}  // extern "C"
