// g2048_qnet_grad.hip -- the gradient half of DQNAgent.train_step (agents/hybrid.py:1038, :1049-1055) for the hybrid agent's
// Q-network on the device: the batch forward of g2048_qnet_batch.hip with its activations kept, the prioritised Huber loss
//   d = q[i, a_i] - target_i;  td_i = 0.5 d^2 if |d| < 1 else |d| - 0.5;  loss = mean(w_i td_i)
// and the backward pass through the whole network, the gradients written in the PLAIN parameter layout (include/g2048.h,
// g2048_qnet_pack's input), where a stock torch optimiser reads them through views. C-ABI: g2048_qnet_loss_grad /
// g2048_qnet_grad_workspace. Eval mode: the reference's live dropout is not in this entry point; the same pass with it is
// g2048_qnet_loss_grad_dropout of libg2048_train_hip.so (g2048_qnet_train.hip, include/g2048_train.h), and acting (g2048_qnet_forward,
// the play kernels) stays without it. f32 only, 8 heads, the n boards ONE sequence, for the reasons g2048_qnet_batch.hip gives. The
// kernels of the backward are g2048_qnet_grad_bwd.h's, which the training pass shares.
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
    if (n == 0) return G2048_OK;
    if (!boards || !plain_f32 || !actions || !targets || !weights || !grad_out || !td_out || !loss_out || !q_out || !workspace)
        return fail(G2048_ERR_ARG, "g2048_qnet_loss_grad: null pointer");
    if (!aligned(boards, 16) || !aligned(plain_f32, 16) || !aligned(grad_out, 16) || !aligned(q_out, 16) || !aligned(workspace, 16) ||
        !aligned(actions, 8) || !aligned(targets, 4) || !aligned(weights, 4) || !aligned(td_out, 4) || !aligned(loss_out, 4))
        return fail(G2048_ERR_ARG, "g2048_qnet_loss_grad: misaligned pointer (boards, plain weights, grad, q, workspace: 16 bytes; actions: 8; "
                                   "the rest: 4)");
    if (n > G2048_QNET_BATCH_MAX)
        return fail(G2048_ERR_ARG, "g2048_qnet_loss_grad: n must not exceed G2048_QNET_BATCH_MAX = %d (the boards are one sequence; "
                                   "a larger batch is not truncated)", G2048_QNET_BATCH_MAX);
    if (!good_encoder_shape(dim_ff, n_layers))
        return fail(G2048_ERR_ARG, "g2048_qnet_loss_grad: dim_ff must be a multiple of 32 (32 .. 65536) and n_layers 1 .. 64");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const GradWorkspace ws(n, dim_ff, n_layers);
    float *base = static_cast<float *>(workspace);
    const float *P = plain_f32;
    float *G = grad_out;
    const int ni = (int)n, ff = dim_ff;
    const size_t nl = (size_t)n_layers;
    const unsigned tiles = (unsigned)(ws.np / 16);
    const float *none = nullptr;
    float *nowhere = nullptr;
    const float *fc = P + kPlLayer0 + nl * pl_layer(ff);

    // ---- the forward of g2048_qnet_forward_batch, its activations kept
    const auto linear = [&](auto RELU, const float *X, int K, const float *W, const float *b, float *Y, int M) {
        hipLaunchKernelGGL(qb_linear_kernel<decltype(RELU)::value>, dim3((unsigned)(M + 63) / 64, tiles), dim3(256), 0, s, X, K, W, b, Y, M, ni);
    };
    float *feat = base + ws.feat(), *c1 = base + ws.c1();
    hipLaunchKernelGGL(qb_conv_kernel, dim3((unsigned)n), dim3(256), 0, s, static_cast<const uint8_t *>(boards), P, feat, c1);
    linear(std::false_type{}, feat, kFlat, P + kPlEmbW, P + kPlEmbB, base + ws.x(0), kD);
    for (size_t l = 0; l < nl; ++l) {
        const float *L = P + kPlLayer0 + l * pl_layer(ff), *norms = L + pl_norm(ff);
        const bool last = l == nl - 1;
        float *x0 = base + ws.x(l), *qkv = base + ws.qkv(l), *att = base + ws.att(l), *x1 = base + ws.x1(l), *h = base + ws.h(l);
        linear(std::false_type{}, x0, kD, L + kPlInW, L + kPlInB, qkv, kQkv);
        hipLaunchKernelGGL(qb_attention_kernel, dim3(tiles, kHeads), dim3(64), 0, s, static_cast<const float *>(qkv), att, ni,
                           base + ws.amax(l), base + ws.asum(l));
        hipLaunchKernelGGL(qb_proj_norm_kernel, dim3(tiles), dim3(512), 0, s, static_cast<const float *>(att), kD, L + kPlOutW, L + kPlOutB, norms,
                           norms + 4 * kD, static_cast<const float *>(x0), x1, base + ws.pre1(l), none, static_cast<float4 *>(nullptr), ni);
        linear(std::true_type{}, x1, kD, L + kPlW1, L + pl_b1(ff), h, ff);
        hipLaunchKernelGGL(qb_proj_norm_kernel, dim3(tiles), dim3(512), 0, s, static_cast<const float *>(h), ff, L + pl_w2(ff), L + pl_b2(ff),
                           norms + 2 * kD, norms + 4 * kD + 1, static_cast<const float *>(x1), base + ws.x(l + 1), base + ws.pre2(l),
                           last ? fc : none, reinterpret_cast<float4 *>(q_out), ni);
    }

    // ---- the loss and the backward
    const auto dx = [&](const float *dY, int M, const float *W, int K, const float *res, const float *mask, float *dX) {
        hipLaunchKernelGGL(qg_dx_kernel, dim3((unsigned)(K + 63) / 64, tiles), dim3(256), 0, s, dY, M, W, K, res, mask, dX, ni);
    };
    const auto dw = [&](const float *dY, int ldy, int M, const float *X, int K, float *dW, float *db) {
        hipLaunchKernelGGL(qg_dw_kernel, dim3((unsigned)(K + 63) / 64, (unsigned)(M + 15) / 16), dim3(256), 0, s, dY, ldy, M, X, K, dW, db, ni);
    };
    float *part = base + ws.part();
    const auto ln = [&](const float *g, const float *pre, const float *norm, const float *eps, float *ds, float *dnorm, float *zero) {
        hipLaunchKernelGGL(qg_ln_kernel, dim3(tiles), dim3(512), 0, s, g, pre, norm, eps, ds, part, ni);
        hipLaunchKernelGGL(qg_tiles_kernel, dim3(1), dim3(256), 0, s, static_cast<const float *>(part), (int)tiles, dnorm, zero);
    };
    float *ga = base + ws.ga(), *gb = base + ws.gb(), *ds = base + ws.ds(), *datt = base + ws.datt(), *dqkv = base + ws.dqkv(),
          *dh = base + ws.dh(), *dz1 = base + ws.dz1(), *dd = base + ws.dd(), *dq = base + ws.dq(), *term = base + ws.term();
    hipLaunchKernelGGL(qg_head_kernel, dim3((unsigned)n), dim3(128), 0, s, reinterpret_cast<const float4 *>(q_out),
                       reinterpret_cast<const long long *>(actions), targets, weights, fc, td_out, reinterpret_cast<float4 *>(dq), term, ga, ni);
    hipLaunchKernelGGL(qg_sum_kernel, dim3(1), dim3(256), 0, s, static_cast<const float *>(term), loss_out, ni);
    {
        float *Gfc = G + kPlLayer0 + nl * pl_layer(ff);
        dw(dq, 4, 4, base + ws.x(nl), kD, Gfc, Gfc + 4 * kD);
    }
    for (size_t l = nl; l-- > 0;) {
        const size_t lo = kPlLayer0 + l * pl_layer(ff);
        const float *L = P + lo, *norms = L + pl_norm(ff);
        float *GL = G + lo, *gnorms = GL + pl_norm(ff);
        const float *x0 = base + ws.x(l), *qkv = base + ws.qkv(l), *att = base + ws.att(l), *x1 = base + ws.x1(l), *h = base + ws.h(l);
        ln(ga, base + ws.pre2(l), norms + 2 * kD, norms + 4 * kD + 1, ds, gnorms + 2 * kD, gnorms + 4 * kD);
        dw(ds, kD, kD, h, ff, GL + pl_w2(ff), GL + pl_b2(ff));
        dx(ds, kD, L + pl_w2(ff), ff, none, h, dh);
        dw(dh, ff, ff, x1, kD, GL + kPlW1, GL + pl_b1(ff));
        dx(dh, ff, L + kPlW1, kD, ds, none, gb);
        ln(gb, base + ws.pre1(l), norms, norms + 4 * kD, ds, gnorms, nowhere);
        dw(ds, kD, kD, att, kD, GL + kPlOutW, GL + kPlOutB);
        dx(ds, kD, L + kPlOutW, kD, none, none, datt);
        hipLaunchKernelGGL(qg_att_dq_kernel, dim3(tiles, kHeads), dim3(64), 0, s, qkv, att, static_cast<const float *>(datt),
                           static_cast<const float *>(base + ws.amax(l)), static_cast<const float *>(base + ws.asum(l)), dqkv, dd, ni);
        hipLaunchKernelGGL(qg_att_dkv_kernel, dim3(tiles, kHeads), dim3(64), 0, s, qkv, static_cast<const float *>(datt),
                           static_cast<const float *>(base + ws.amax(l)), static_cast<const float *>(base + ws.asum(l)),
                           static_cast<const float *>(dd), dqkv, ni);
        dw(dqkv, kQkv, kQkv, x0, kD, GL + kPlInW, GL + kPlInB);
        dx(dqkv, kQkv, L + kPlInW, kD, ds, none, ga);
    }
    dw(ga, kD, kD, feat, kFlat, G + kPlEmbW, G + kPlEmbB);
    dx(ga, kD, P + kPlEmbW, kFlat, none, feat, dh);
    hipLaunchKernelGGL(qg_conv_dw2_kernel, dim3(kC2), dim3(512), 0, s, static_cast<const float *>(dh), static_cast<const float *>(c1),
                       G + kPlC2W, G + kPlC2B, ni);
    hipLaunchKernelGGL(qg_conv_dz1_kernel, dim3((unsigned)n), dim3(256), 0, s, static_cast<const float *>(dh), static_cast<const float *>(c1), P, dz1);
    hipLaunchKernelGGL(qg_conv_dw1_kernel, dim3(kC1), dim3(256), 0, s, static_cast<const float *>(dz1), static_cast<const uint8_t *>(boards),
                       G + kPlC1W, G + kPlC1B, ni);
    return check_launch("g2048_qnet_loss_grad");
}

}  // extern "C"
