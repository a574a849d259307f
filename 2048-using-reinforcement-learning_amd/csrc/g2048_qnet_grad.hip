// g2048_qnet_grad.hip -- the gradient half of DQNAgent.train_step (agents/hybrid.py:1038, :1049-1055) for the hybrid agent's
// Q-network on the device: the batch forward of g2048_qnet_batch.hip with its activations kept, the prioritised Huber loss
//   d = q[i, a_i] - target_i;  td_i = 0.5 d^2 if |d| < 1 else |d| - 0.5;  loss = mean(w_i td_i)
// and the backward pass through the whole network, the gradients written in the PLAIN parameter layout (include/g2048.h,
// g2048_qnet_pack's input), where a stock torch optimiser reads them through views. C-ABI: g2048_qnet_loss_grad /
// g2048_qnet_grad_workspace. Eval mode: the reference's live dropout is not in this entry point; the same pass with it is
// g2048_qnet_loss_grad_dropout of libg2048_train_hip.so (g2048_qnet_train.hip, include/g2048_train.h), and acting (g2048_qnet_forward,
// the play kernels) stays without it. f32 only, 8 heads, the n boards ONE sequence, for the reasons g2048_qnet_batch.hip gives. The
// kernels of the backward and the launch sequence (qg_pass<kDrop>) are g2048_qnet_grad_bwd.h's, which the training pass shares; this
// file keeps the entry point and the size query.
//
// The forward is that file's kernels (g2048_qnet_batch_fwd.h), launched in the same order on the same operands, so q_out has
// the bits of g2048_qnet_forward_batch; per layer it keeps the layer input, qkv, the attention output with the rows' maximum and
// sum, both sums before the LayerNorms, norm1's output, the ReLU'd hidden layer, and conv1's and conv2's ReLU'd outputs.
//
// The backward is one phase per launch:
//   head      the Huber derivative w_i / n . clamp(d, -1, 1) at the taken action (actions[i] & 3), td, the loss terms, dx = dq . fc.weight
//   sum       the loss: one block's fixed-order sum of the n terms
//   ln        LayerNorm backward for a tile of 16 boards (mean and rstd recomputed as the forward computes them), with the tile's
//             share of dgamma = sum dy . xhat and dbeta = sum dy; `tiles` then adds the tiles' shares in order
//   dx        (g2048_grad_products.h) dX = dY . W (+ the residual's other gradient path, or x the ReLU mask) on the f32 matrix cores, one wavefront a
//             16-board x 16-feature tile, the A operand a column slice of the row-major W
//   dw        (g2048_grad_products.h) dW[M][K] = sum_n dY[n][M] . X[n][K] and db = sum_n dY on the f32 matrix cores: the boards are the contraction, one
//             wavefront owns a 16 x 16 tile of dW over all n
//   att_dq    one wavefront a (query tile, head): P recomputed from qkv with the forward's maximum and sum, D_i = sum dO_i . O_i,
//             dS_ij = P_ij (dO_i . V_j - D_i), dQ_i = 1/4 sum_j dS_ij K_j
//   att_dkv   one wavefront a (key tile, head): dV_j = sum_i P_ij dO_i, dK_j = 1/4 sum_i dS_ij Q_i
//   conv      on the VALU: dW2 / db2 (a block an output channel), the transposed convolution into conv1's output with its ReLU mask
//             (a block a board), dW1 / db1 (a block a channel)
// The rules are g2048_qnet_batch.hip's: no atomics, no split-K across blocks, every output element one wavefront's (or one
// thread's, then one block's tree's) fixed-order accumulation, so two calls give the same bits; nothing past row n or past the
// stated sizes is read or written; no block waits on another; long sums run in several independent partial sums (eight board
// tiles or feature chunks at a time, four key or query tiles) combined pairwise. grad_out is overwritten, never accumulated into.
// Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/g2048.h"
#include "g2048_host.h"
#include "g2048_grad_products.h"
#include "g2048_mfma.h"
#include "g2048_qnet_batch_fwd.h"
#include "g2048_qnet_grad_bwd.h"

extern "C" {

size_t g2048_qnet_grad_workspace(size_t n, int dim_ff, int n_layers)
{
    if (n == 0 || n > G2048_QNET_BATCH_MAX || !good_encoder_shape(dim_ff, n_layers)) return 0;
    return GradWorkspace(n, dim_ff, n_layers).floats() * sizeof(float);
}

int g2048_qnet_loss_grad(const void *boards, const float *plain_f32, const int64_t *actions, const float *targets, const float *weights,
                         size_t n, int dim_ff, int n_layers, float *grad_out, float *td_out, float *loss_out, float *q_out,
                         void *workspace, void *stream)
{
    return qg_pass<false>("g2048_qnet_loss_grad", QbCall{boards, plain_f32, actions, targets, weights, n, dim_ff, n_layers, grad_out, td_out, loss_out,
                                                         q_out, workspace, stream, true, nullptr, 0, 0});
}

}  // extern "C"
