// g2048_qnet_train.hip -- libg2048_train_hip.so (include/g2048_train.h): the hybrid agent's Q-network in TRAINING mode, with the
// reference's live dropout. DQNAgent.train_step (agents/hybrid.py:1038-1044) never calls .eval(), so its three forwards run
// nn.TransformerEncoderLayer's four dropout sites; g2048_qnet_forward_batch_dropout is g2048_qnet_forward_batch and
// g2048_qnet_loss_grad_dropout is g2048_qnet_loss_grad with them, g2048_qnet_dropout_mask writes a site's keep bits for the tests.
// A library of its own because the main library's export table is closed (ABI 5); the kernels are the main library's, shared as
// headers (g2048_qnet_batch_fwd.h, g2048_grad_products.h, g2048_qnet_grad_bwd.h) and instantiated here a second time with a QDrop
// (g2048_qnet_drop.h) as their trailing argument. So are the launch sequences: qb_forward_pass<true> (g2048_qnet_batch_fwd.h) and
// qg_pass<true> (g2048_qnet_grad_bwd.h) are the main library's with kDrop set; this file keeps the entry points and the size query.
// Acting has no dropout: g2048_qnet_forward and the play kernels are not here.
//
// Where the masks go (site s of layer L, element e; the rule: g2048_qnet_drop.h):
//   forward   s = 0  qb_attention_kernel: the probabilities x m before P.V, the row's maximum and sum of the unmasked scores
//             s = 1  qb_proj_norm_kernel (out_proj): (H W^T + b) x m before the residual add
//             s = 2  qb_linear_kernel<RELU> (linear1): relu(..) x m
//             s = 3  qb_proj_norm_kernel (linear2): as s = 1
//             The pass keeps the DROPPED attention output and the DROPPED hidden layer, nothing more: no mask is stored.
//   backward  s = 3, 1  the gradient ds leaving the LayerNorm backward goes to the residual as it is, and x m (qt_scale_kernel of g2048_qnet_drop.h, one
//             elementwise launch into a second array) into the dW / dX products of linear2 / out_proj
//             s = 2  qg_dx_kernel through linear2: x m next to the ReLU mask; linear2's dW reads the dropped hidden layer
//             s = 0  qg_att_dq_kernel / qg_att_dkv_kernel: dP_ij = m_ij (dO_i . V_j), dV_j = sum_i P_ij m_ij dO_i, each hashing the
//             tile it recomputes; D_i = dO_i . O_i holds with the dropped O, so dd stays as it is
// A site with p == 0 is not hashed: its launch is the instantiation without a QDrop, which is the main library's kernel. With all
// four 0 the launch sequence is g2048_qnet_forward_batch's / g2048_qnet_loss_grad's and so are the bits.
// The rules are g2048_qnet_grad.hip's: no atomics, every output element one fixed-order accumulation, two calls with the same
// (seed, call index) give the same bits, nothing past row n or the stated sizes is read or written. Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/g2048_train.h"
#include "g2048_host.h"
#include "g2048_grad_products.h"
#include "g2048_mfma.h"
#include "g2048_qnet_batch_fwd.h"
#include "g2048_qnet_drop.h"
#include "g2048_qnet_grad_bwd.h"

extern "C" {

const char *g2048_train_last_error(void) { return g_err; }

int g2048_train_abi_version(void) { return G2048_TRAIN_ABI_VERSION; }

size_t g2048_qnet_train_workspace(size_t n, int dim_ff, int n_layers)
{
    if (n == 0 || n > G2048_QNET_BATCH_MAX || !good_encoder_shape(dim_ff, n_layers)) return 0;
    return TrainWorkspace(n, dim_ff, n_layers).floats() * sizeof(float);
}

int g2048_qnet_forward_batch_dropout(const void *boards, const float *plain_f32, float *q_out, size_t n, int dim_ff, int n_layers,
                                     const double *p4, uint64_t seed, uint64_t call_index, void *workspace, void *stream)
{
    return qb_forward_pass<true>("g2048_qnet_forward_batch_dropout", QbCall{boards, plain_f32, nullptr, nullptr, nullptr, n, dim_ff, n_layers, nullptr,
                                                                            nullptr, nullptr, q_out, workspace, stream, false, p4, seed, call_index});
}

int g2048_qnet_loss_grad_dropout(const void *boards, const float *plain_f32, const int64_t *actions, const float *targets, const float *weights,
                                 size_t n, int dim_ff, int n_layers, const double *p4, uint64_t seed, uint64_t call_index, float *grad_out,
                                 float *td_out, float *loss_out, float *q_out, void *workspace, void *stream)
{
    return qg_pass<true>("g2048_qnet_loss_grad_dropout", QbCall{boards, plain_f32, actions, targets, weights, n, dim_ff, n_layers, grad_out, td_out,
                                                                loss_out, q_out, workspace, stream, true, p4, seed, call_index});
}

int g2048_qnet_dropout_mask(uint64_t seed, uint64_t call_index, int layer, int site, double p, size_t n, int dim_ff, size_t first_row,
                            size_t rows, uint8_t *keep_out, void *stream)
{
    // at most 32,768 x 4,096 or 4,096 x 65,536 elements
    return dropout_mask("g2048_qnet_dropout_mask", kDomQnetDropout, G2048_QNET_BATCH_MAX, "G2048_QNET_BATCH_MAX", seed, call_index, layer, site, p, n,
                        dim_ff, site == 0 ? (size_t)kHeads * n : n, site == 0 ? n : site == 2 ? (size_t)dim_ff : (size_t)kD, first_row, rows,
                        keep_out, stream);
}

}  // extern "C"
