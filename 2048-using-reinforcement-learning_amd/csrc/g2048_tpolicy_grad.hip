// g2048_tpolicy_grad.hip -- libg2048_tlearn_hip.so (include/g2048_tlearn.h): PPOAgent.update()'s loss (agents/ppo_agent.py:378-400)
// on the two heads of the reference's transformer policy (models/transformer.py:4-40, eval mode) and its gradient with respect to
// every parameter, written in the network's plain parameter layout (g2048_tpolicy_layout.h), where a stock torch optimiser reads
// it through views. A library of its own because the other two export tables are closed. f32 only.
//
// The fused forward of g2048_tpolicy.hip never leaves the VGPRs, which keeps nothing for a backward pass. This pass is a sequence
// of launches over a token-major f32 workspace [16 n tokens][features] (token 16 board + cell), in which the flatten before fc1 is
// a view [n][1024] and every projection is a product over 16 n rows:
//   forward   embedding; per layer in_proj (tg_linear_kernel), attention per (board, head) as three 16 x 16 x 16 products on the f32
//             MFMA with the probabilities kept (tg_attention_kernel), out_proj + residual, LayerNorm with mean and rstd kept
//             (tg_ln_kernel), linear1 + ReLU, linear2 + residual, LayerNorm; then fc1, fc2 and the head tile.
//   head      a thread a board: both heads on the VALU, softmax, the row's loss terms by g2048_ppo_head.h (the MLP learner's
//             arithmetic), d loss / d logits, d loss / d value and the gradient into relu(fc2)'s output; pg_loss_kernel sums the rows.
//   backward  heads, fc2, fc1 (qg_dw_kernel / qg_dx_kernel of g2048_grad_products.h over n rows); per layer in reverse LayerNorm
//             backward (tg_ln_bwd_kernel), linear2 / ReLU mask / linear1, the residual's two paths (qg_dx_kernel's `res`), out_proj,
//             attention backward per (board, head) (tg_attention_bwd_kernel: dV = P^T dO, dP = dO V^T, dS = P o (dP - rowsum(dP o P)),
//             dQ = dS K / 4, dK = dS^T Q / 4), in_proj; finally the embedding (tg_embed_bwd_kernel).
// Kept and recomputed. Kept per layer: the layer's input, qkv, the attention probabilities, the attention output, both sums before
// the LayerNorms with their mean and rstd, and norm1's output. NOT kept: the [16 n][dim_ff] hidden layer relu(linear1 ..). It is by
// far the largest activation (128 MiB a layer at n = 1,024, dim_ff 2,048) and one product rebuilds it, so the backward recomputes
// it per layer into the one buffer the forward used (bit for bit the forward's: the same kernel on the same inputs).
// Weight gradients over 16 n rows. qg_dw_kernel gives an output tile to one wavefront that walks all rows; for this network's
// small matrices (out_proj is 16 tiles) over 16,384 rows that leaves the chip idle. tg_dw_split_kernel is the same tile over one
// chunk of kRowChunk rows -- a constant: the split depends on the row count alone, never on the launch geometry -- writing
// partial tiles and partial bias sums to the workspace, and tg_combine_kernel adds the chunks in a fixed order. The column sums of
// the LayerNorm parameters and the embedding use the same scheme with chunks of kColRows rows.
// The rules are the other two gradient passes': no atomics, every output element one fixed-order accumulation (two calls give the
// same bits), nothing past row n or outside the stated workspace read or written, no workspace element read before this call
// wrote it. Compile with -ffp-contract=off.
// The workspace, the kernels and the launch sequence are g2048_tpolicy_grad_pass.h's, shared with the training-mode pass of
// g2048_tpolicy_train.hip; this library instantiates every kernel without a dropout site.
#include "g2048_tpolicy_grad_pass.h"

extern "C" {

const char *g2048_tlearn_last_error(void) { return g_err; }

int g2048_tlearn_abi_version(void) { return G2048_TLEARN_ABI_VERSION; }

size_t g2048_tpolicy_grad_workspace(size_t n, int dim_ff, int n_layers)
{
    if (!good_shape(n, dim_ff, n_layers)) return 0;
    return Workspace(n, dim_ff, n_layers).floats() * sizeof(float);
}

int g2048_tpolicy_loss_grad(const void *boards, const float *plain_f32, const int64_t *actions, const float *old_log_probs,
                            const float *advantages, const float *returns, size_t n, int dim_ff, int n_layers, float clip_epsilon,
                            float value_coef, float entropy_coef, float *grad_out, float *losses4_out, float *probs_out, float *value_out,
                            void *workspace, size_t workspace_bytes, void *stream)
{
    const char *entry = "g2048_tpolicy_loss_grad";
    if (n == 0) return G2048_OK;
    const TgCall c{boards, plain_f32, actions, old_log_probs, advantages, returns, n, dim_ff, n_layers, clip_epsilon, value_coef, entropy_coef,
                   grad_out, losses4_out, probs_out, value_out, workspace, workspace_bytes, stream, true, nullptr, 0, 0};
    const size_t needed = n <= G2048_TLEARN_BATCH_MAX && good_encoder_shape(dim_ff, n_layers) ? Workspace(n, dim_ff, n_layers).floats() * sizeof(float) : 0;
    if (const int rc = tg_check(entry, c, needed, "g2048_tpolicy_grad_workspace")) return rc;
    return tg_pass<false>(entry, c);
}

}  // extern "C"
