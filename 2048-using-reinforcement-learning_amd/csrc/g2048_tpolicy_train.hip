// g2048_tpolicy_train.hip -- libg2048_ttrain_hip.so (include/g2048_ttrain.h): the transformer policy in TRAINING mode, with the
// encoder's live dropout. models/transformer.py builds nn.TransformerEncoderLayer with dropout 0.1 and PPOAgent.update() never calls
// .eval(), so the two critic forwards of its advantage block and the forward of every epoch run the layer's four dropout sites:
// g2048_tpolicy_loss_grad_dropout is g2048_tpolicy_loss_grad with them, g2048_tpolicy_forward_dropout the forward alone (what the
// advantage block needs), g2048_tpolicy_dropout_mask writes a site's keep bits for the tests. A library of its own because the
// learner library's export table is closed; the workspace, the kernels and the launch sequence are the learner library's, shared
// as g2048_tpolicy_grad_pass.h and instantiated here a second time with a QDrop (g2048_qnet_drop.h, RNG domain kDomTpolicyDropout)
// as their trailing argument. Acting has no dropout: the fused kernel of g2048_tpolicy.hip is not here.
//
// Where the masks go, what is kept (the UNMASKED attention probabilities and nothing of any mask) and the identity the attention's
// backward uses are in that header's head comment. Sites 1 and 3 in the backward are one elementwise launch (qt_scale_kernel of g2048_qnet_drop.h) into
// one extra [16 n][64] array, not fused into the dW / dX products, so qg_dx_kernel and tg_dw_split_kernel stay as they are.
// A site with p == 0 is not hashed: its launch is the instantiation without a QDrop, which is the learner library's kernel. With all
// four 0 the kernel launches are g2048_tpolicy_loss_grad's in its order and so are the bits; the one difference is that a layer's two
// LayerNorm-eps slots of grad are cleared by a one-block launch (tg_zero_kernel) where that pass enqueues a memset.
// The rules are g2048_tpolicy_grad.hip's: no atomics, every output element one fixed-order accumulation, two calls with the same
// (seed, call index) give the same bits, nothing past row n or the stated workspace is read or written. Compile with
// -ffp-contract=off.
#include "../../include/g2048_ttrain.h"
#include "g2048_tpolicy_grad_pass.h"

namespace {

size_t train_bytes(size_t n, int dim_ff, int n_layers)
{
    return good_shape(n, dim_ff, n_layers) ? Workspace(n, dim_ff, n_layers).train_floats() * sizeof(float) : 0;
}

int run(const char *entry, const TgCall &c)
{
    if (c.n == 0) return G2048_OK;
    if (!c.p4) return fail(G2048_ERR_ARG, "%s: null pointer", entry);
    if (const int rc = tg_check(entry, c, train_bytes(c.n, c.dim_ff, c.n_layers), "g2048_tpolicy_train_workspace")) return rc;
    if (const int rc = check_p(entry, c.p4)) return rc;
    return tg_pass<true>(entry, c, kDomTpolicyDropout);
}

}  // namespace

extern "C" {

const char *g2048_ttrain_last_error(void) { return g_err; }

int g2048_ttrain_abi_version(void) { return G2048_TTRAIN_ABI_VERSION; }

size_t g2048_tpolicy_train_workspace(size_t n, int dim_ff, int n_layers) { return train_bytes(n, dim_ff, n_layers); }

int g2048_tpolicy_loss_grad_dropout(const void *boards, const float *plain_f32, const int64_t *actions, const float *old_log_probs,
                                    const float *advantages, const float *returns, size_t n, int dim_ff, int n_layers, const double *p4,
                                    uint64_t seed, uint64_t call_index, float clip_epsilon, float value_coef, float entropy_coef,
                                    float *grad_out, float *losses4_out, float *probs_out, float *value_out, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    return run("g2048_tpolicy_loss_grad_dropout",
               TgCall{boards, plain_f32, actions, old_log_probs, advantages, returns, n, dim_ff, n_layers, clip_epsilon, value_coef, entropy_coef,
                      grad_out, losses4_out, probs_out, value_out, workspace, workspace_bytes, stream, true, p4, seed, call_index});
}

int g2048_tpolicy_forward_dropout(const void *boards, const float *plain_f32, size_t n, int dim_ff, int n_layers, const double *p4,
                                  uint64_t seed, uint64_t call_index, float *probs_out, float *value_out, void *workspace,
                                  size_t workspace_bytes, void *stream)
{
    return run("g2048_tpolicy_forward_dropout",
               TgCall{boards, plain_f32, nullptr, nullptr, nullptr, nullptr, n, dim_ff, n_layers, 0.0f, 0.0f, 0.0f, nullptr, nullptr, probs_out,
                      value_out, workspace, workspace_bytes, stream, false, p4, seed, call_index});
}

int g2048_tpolicy_dropout_mask(uint64_t seed, uint64_t call_index, int layer, int site, double p, size_t n, int dim_ff, size_t first_row,
                               size_t rows, uint8_t *keep_out, void *stream)
{
    // at most 65,536 x 16 or 16,384 x 65,536 = 2^30 elements
    return dropout_mask("g2048_tpolicy_dropout_mask", kDomTpolicyDropout, G2048_TLEARN_BATCH_MAX, "G2048_TLEARN_BATCH_MAX", seed, call_index, layer,
                        site, p, n, dim_ff, site == 0 ? (size_t)kHeads * kTok * n : (size_t)kTok * n,
                        site == 0 ? (size_t)kTok : site == 2 ? (size_t)dim_ff : (size_t)kD, first_row, rows, keep_out, stream);
}

}  // extern "C"
