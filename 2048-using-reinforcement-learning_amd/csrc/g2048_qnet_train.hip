// g2048_qnet_train.hip -- libg2048_train_hip.so (include/g2048_train.h): the hybrid agent's Q-network in TRAINING mode, with the
// reference's live dropout. DQNAgent.train_step (agents/hybrid.py:1038-1044) never calls .eval(), so its three forwards run
// nn.TransformerEncoderLayer's four dropout sites; g2048_qnet_forward_batch_dropout is g2048_qnet_forward_batch and
// g2048_qnet_loss_grad_dropout is g2048_qnet_loss_grad with them, g2048_qnet_dropout_mask writes a site's keep bits for the tests.
// A library of its own because the main library's export table is closed (ABI 5); the kernels are the main library's, shared as
// headers (g2048_qnet_batch_fwd.h, g2048_grad_products.h, g2048_qnet_grad_bwd.h) and instantiated here a second time with a QDrop
// (g2048_qnet_drop.h) as their trailing argument. Acting has no dropout: g2048_qnet_forward and the play kernels are not here.
//
// Where the masks go (site s of layer L, element e; the rule: g2048_qnet_drop.h):
//   forward   s = 0  qb_attention_kernel: the probabilities x m before P.V, the row's maximum and sum of the unmasked scores
//             s = 1  qb_proj_norm_kernel (out_proj): (H W^T + b) x m before the residual add
//             s = 2  qb_linear_kernel<RELU> (linear1): relu(..) x m
//             s = 3  qb_proj_norm_kernel (linear2): as s = 1
//             The pass keeps the DROPPED attention output and the DROPPED hidden layer, nothing more: no mask is stored.
//   backward  s = 3, 1  the gradient ds leaving the LayerNorm backward goes to the residual as it is, and x m (qt_scale_kernel, one
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

namespace {

// g2048_qnet_forward_batch's workspace (g2048_qnet_batch.hip), in floats: x [np][128], qkv [np][384], att [np][128],
// h [np][max(1024, dim_ff)] (feat, then the hidden layer)
struct FwdWorkspace {
    size_t np, hw;
    FwdWorkspace(size_t n, int ff) : np((n + 15) / 16 * 16), hw((size_t)(ff > kFlat ? ff : kFlat)) {}
    size_t x() const { return 0; }
    size_t qkv() const { return np * kD; }
    size_t att() const { return qkv() + np * kQkv; }
    size_t h() const { return att() + np * kD; }
};

// the training pass's workspace: GradWorkspace, then dsm [np][128], the LayerNorm backward's ds x a site's multipliers
struct TrainWorkspace : GradWorkspace {
    using GradWorkspace::GradWorkspace;
    size_t dsm() const { return GradWorkspace::floats(); }
    size_t floats() const { return dsm() + np * kD; }
};

// the four sites of one layer of one call; on[s]: p[s] > 0
struct Sites {
    QDrop d[4];
    bool on[4];
    Sites(uint64_t seed, uint64_t call_index, int layer, const double *p)
    {
        for (int s = 0; s < 4; ++s) {
            on[s] = p[s] > 0.0;
            d[s] = qdrop_site(kDomQnetDropout, seed, call_index, layer, s, p[s]);
        }
    }
};

// `dropped` with the site's QDrop as its last argument where the site is live, else `plain`: the main library's kernel
template <class Plain, class Dropped, class... Args>
void launch_site(bool on, const QDrop &d, Plain plain, Dropped dropped, dim3 grid, dim3 block, hipStream_t s, Args... args)
{
    if (on)
        hipLaunchKernelGGL(dropped, grid, block, 0, s, args..., d);
    else
        hipLaunchKernelGGL(plain, grid, block, 0, s, args...);
}

// Y[i] = X[i] m_i over the n x 128 elements of site 1 or 3 (element row 128 + feature = i)
__global__ __launch_bounds__(256) void qt_scale_kernel(const float *__restrict__ X, float *__restrict__ Y, QDrop drop, uint32_t count)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < count) Y[i] = X[i] * qdrop_mult(drop, i);
}

// keep[i] = the keep bit of element first + i of a site, i < count
__global__ __launch_bounds__(256) void qt_mask_kernel(uint8_t *__restrict__ keep, QDrop drop, uint32_t first, uint32_t count)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < count) keep[i] = qdrop_keep(drop, first + i) ? 1 : 0;
}

int check_p(const char *entry, const double *p4)
{
    if (!p4) return fail(G2048_ERR_ARG, "%s: null pointer", entry);
    for (int s = 0; s < 4; ++s)
        if (!good_qdrop(p4[s])) return fail(G2048_ERR_ARG, "%s: p[%d] must be finite, 0 <= p < 1", entry, s);
    return G2048_OK;
}

// the encoder layers of both passes' forward: layer l from x0 into x_next (q on the last), att and h the DROPPED ones
struct LayerBuffers {
    const float *x0;
    float *qkv, *att, *x1, *pre1, *h, *x_next, *pre2, *amax, *asum;
};

void forward_layer(hipStream_t s, const float *L, int ff, const Sites &st, const LayerBuffers &b, const float *fc_or_null, float *q_out, int ni,
                   unsigned tiles)
{
    const float *norms = L + pl_norm(ff), *none = nullptr;
    hipLaunchKernelGGL((qb_linear_kernel<false>), dim3((unsigned)(kQkv + 63) / 64, tiles), dim3(256), 0, s, b.x0, kD, L + kPlInW, L + kPlInB, b.qkv,
                       kQkv, ni);
    launch_site(st.on[0], st.d[0], qb_attention_kernel<>, qb_attention_kernel<QDrop>, dim3(tiles, kHeads), dim3(64), s,
                static_cast<const float *>(b.qkv), b.att, ni, b.amax, b.asum);
    launch_site(st.on[1], st.d[1], qb_proj_norm_kernel<>, qb_proj_norm_kernel<QDrop>, dim3(tiles), dim3(512), s, static_cast<const float *>(b.att),
                kD, L + kPlOutW, L + kPlOutB, norms, norms + 4 * kD, b.x0, b.x1, b.pre1, none, static_cast<float4 *>(nullptr), ni);
    launch_site(st.on[2], st.d[2], qb_linear_kernel<true>, qb_linear_kernel<true, false, QDrop>, dim3((unsigned)(ff + 63) / 64, tiles), dim3(256), s,
                static_cast<const float *>(b.x1), kD, L + kPlW1, L + pl_b1(ff), b.h, ff, ni);
    launch_site(st.on[3], st.d[3], qb_proj_norm_kernel<>, qb_proj_norm_kernel<QDrop>, dim3(tiles), dim3(512), s, static_cast<const float *>(b.h),
                ff, L + pl_w2(ff), L + pl_b2(ff), norms + 2 * kD, norms + 4 * kD + 1, static_cast<const float *>(b.x1), b.x_next, b.pre2,
                fc_or_null, reinterpret_cast<float4 *>(q_out), ni);
}

}  // namespace

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
    const char *entry = "g2048_qnet_forward_batch_dropout";
    if (n == 0) return G2048_OK;
    if (!boards || !plain_f32 || !q_out || !workspace) return fail(G2048_ERR_ARG, "%s: null pointer", entry);
    if (!aligned(boards, 16) || !aligned(plain_f32, 16) || !aligned(q_out, 16) || !aligned(workspace, 16))
        return fail(G2048_ERR_ARG, "%s: misaligned pointer (boards, plain weights, q, workspace: 16 bytes)", entry);
    if (n > G2048_QNET_BATCH_MAX)
        return fail(G2048_ERR_ARG, "%s: n must not exceed G2048_QNET_BATCH_MAX = %d (the boards are one sequence; a larger batch is not "
                                   "truncated)", entry, G2048_QNET_BATCH_MAX);
    if (!good_encoder_shape(dim_ff, n_layers))
        return fail(G2048_ERR_ARG, "%s: dim_ff must be a multiple of 32 (32 .. 65536) and n_layers 1 .. 64", entry);
    if (const int rc = check_p(entry, p4)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const FwdWorkspace ws(n, dim_ff);
    float *base = static_cast<float *>(workspace), *x = base + ws.x(), *qkv = base + ws.qkv(), *att = base + ws.att(), *h = base + ws.h();
    const float *P = plain_f32;
    const int ni = (int)n, ff = dim_ff;
    const unsigned tiles = (unsigned)(ws.np / 16);
    float *nowhere = nullptr;
    hipLaunchKernelGGL(qb_conv_kernel, dim3((unsigned)n), dim3(256), 0, s, static_cast<const uint8_t *>(boards), P, h, nowhere);
    hipLaunchKernelGGL((qb_linear_kernel<false>), dim3((unsigned)(kD + 63) / 64, tiles), dim3(256), 0, s, static_cast<const float *>(h), kFlat,
                       P + kPlEmbW, P + kPlEmbB, x, kD, ni);
    for (int l = 0; l < n_layers; ++l) {
        const bool last = l == n_layers - 1;
        const LayerBuffers b{x, qkv, att, x, nowhere, h, last ? nowhere : x, nowhere, nowhere, nowhere};
        forward_layer(s, P + kPlLayer0 + (size_t)l * pl_layer(ff), ff, Sites(seed, call_index, l, p4), b,
                      last ? P + kPlLayer0 + (size_t)n_layers * pl_layer(ff) : nullptr, q_out, ni, tiles);
    }
    return check_launch(entry);
}

int g2048_qnet_loss_grad_dropout(const void *boards, const float *plain_f32, const int64_t *actions, const float *targets, const float *weights,
                                 size_t n, int dim_ff, int n_layers, const double *p4, uint64_t seed, uint64_t call_index, float *grad_out,
                                 float *td_out, float *loss_out, float *q_out, void *workspace, void *stream)
{
    const char *entry = "g2048_qnet_loss_grad_dropout";
    if (n == 0) return G2048_OK;
    if (!boards || !plain_f32 || !actions || !targets || !weights || !grad_out || !td_out || !loss_out || !q_out || !workspace)
        return fail(G2048_ERR_ARG, "%s: null pointer", entry);
    if (!aligned(boards, 16) || !aligned(plain_f32, 16) || !aligned(grad_out, 16) || !aligned(q_out, 16) || !aligned(workspace, 16) ||
        !aligned(actions, 8) || !aligned(targets, 4) || !aligned(weights, 4) || !aligned(td_out, 4) || !aligned(loss_out, 4))
        return fail(G2048_ERR_ARG, "%s: misaligned pointer (boards, plain weights, grad, q, workspace: 16 bytes; actions: 8; the rest: 4)", entry);
    if (n > G2048_QNET_BATCH_MAX)
        return fail(G2048_ERR_ARG, "%s: n must not exceed G2048_QNET_BATCH_MAX = %d (the boards are one sequence; a larger batch is not "
                                   "truncated)", entry, G2048_QNET_BATCH_MAX);
    if (!good_encoder_shape(dim_ff, n_layers))
        return fail(G2048_ERR_ARG, "%s: dim_ff must be a multiple of 32 (32 .. 65536) and n_layers 1 .. 64", entry);
    if (const int rc = check_p(entry, p4)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const TrainWorkspace ws(n, dim_ff, n_layers);
    float *base = static_cast<float *>(workspace);
    const float *P = plain_f32;
    float *G = grad_out;
    const int ni = (int)n, ff = dim_ff;
    const size_t nl = (size_t)n_layers;
    const unsigned tiles = (unsigned)(ws.np / 16);
    const float *none = nullptr;
    float *nowhere = nullptr;
    const float *fc = P + kPlLayer0 + nl * pl_layer(ff);

    // ---- the forward of g2048_qnet_forward_batch_dropout, its activations kept
    float *feat = base + ws.feat(), *c1 = base + ws.c1();
    hipLaunchKernelGGL(qb_conv_kernel, dim3((unsigned)n), dim3(256), 0, s, static_cast<const uint8_t *>(boards), P, feat, c1);
    hipLaunchKernelGGL((qb_linear_kernel<false>), dim3((unsigned)(kD + 63) / 64, tiles), dim3(256), 0, s, static_cast<const float *>(feat), kFlat,
                       P + kPlEmbW, P + kPlEmbB, base + ws.x(0), kD, ni);
    for (size_t l = 0; l < nl; ++l) {
        const bool last = l == nl - 1;
        const LayerBuffers b{base + ws.x(l), base + ws.qkv(l), base + ws.att(l), base + ws.x1(l), base + ws.pre1(l), base + ws.h(l),
                             base + ws.x(l + 1), base + ws.pre2(l), base + ws.amax(l), base + ws.asum(l)};
        forward_layer(s, P + kPlLayer0 + l * pl_layer(ff), ff, Sites(seed, call_index, (int)l, p4), b, last ? fc : none, q_out, ni, tiles);
    }

    // ---- the loss and the backward
    const auto dx = [&](const float *dY, int M, const float *W, int K, const float *res, const float *mask, float *dX) {
        hipLaunchKernelGGL(qg_dx_kernel<>, dim3((unsigned)(K + 63) / 64, tiles), dim3(256), 0, s, dY, M, W, K, res, mask, dX, ni);
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
          *dh = base + ws.dh(), *dz1 = base + ws.dz1(), *dd = base + ws.dd(), *dq = base + ws.dq(), *term = base + ws.term(),
          *dsm = base + ws.dsm();
    // ds x the multipliers of site 1 or 3: what enters the dropped projection's dW and dX (ds itself where the site is off)
    const auto scaled = [&](bool on, const QDrop &d) -> const float * {
        if (!on) return ds;
        hipLaunchKernelGGL(qt_scale_kernel, dim3(blocks_for(n * kD, 256)), dim3(256), 0, s, static_cast<const float *>(ds), dsm, d,
                           (uint32_t)(n * kD));
        return dsm;
    };
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
        const float *amax = base + ws.amax(l), *asum = base + ws.asum(l);
        const Sites st(seed, call_index, (int)l, p4);
        ln(ga, base + ws.pre2(l), norms + 2 * kD, norms + 4 * kD + 1, ds, gnorms + 2 * kD, gnorms + 4 * kD);
        const float *d3 = scaled(st.on[3], st.d[3]);
        dw(d3, kD, kD, h, ff, GL + pl_w2(ff), GL + pl_b2(ff));
        launch_site(st.on[2], st.d[2], qg_dx_kernel<>, qg_dx_kernel<QDrop>, dim3((unsigned)(ff + 63) / 64, tiles), dim3(256), s, d3, kD,
                    L + pl_w2(ff), ff, none, h, dh, ni);
        dw(dh, ff, ff, x1, kD, GL + kPlW1, GL + pl_b1(ff));
        dx(dh, ff, L + kPlW1, kD, ds, none, gb);
        ln(gb, base + ws.pre1(l), norms, norms + 4 * kD, ds, gnorms, nowhere);
        const float *d1 = scaled(st.on[1], st.d[1]);
        dw(d1, kD, kD, att, kD, GL + kPlOutW, GL + kPlOutB);
        dx(d1, kD, L + kPlOutW, kD, none, none, datt);
        launch_site(st.on[0], st.d[0], qg_att_dq_kernel<>, qg_att_dq_kernel<QDrop>, dim3(tiles, kHeads), dim3(64), s, qkv, att,
                    static_cast<const float *>(datt), amax, asum, dqkv, dd, ni);
        launch_site(st.on[0], st.d[0], qg_att_dkv_kernel<>, qg_att_dkv_kernel<QDrop>, dim3(tiles, kHeads), dim3(64), s, qkv,
                    static_cast<const float *>(datt), amax, asum, static_cast<const float *>(dd), dqkv, ni);
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
    return check_launch(entry);
}

int g2048_qnet_dropout_mask(uint64_t seed, uint64_t call_index, int layer, int site, double p, size_t n, int dim_ff, size_t first_row,
                            size_t rows, uint8_t *keep_out, void *stream)
{
    const char *entry = "g2048_qnet_dropout_mask";
    if (n == 0 || rows == 0) return G2048_OK;
    if (!keep_out) return fail(G2048_ERR_ARG, "%s: null pointer", entry);
    if (n > G2048_QNET_BATCH_MAX) return fail(G2048_ERR_ARG, "%s: n must not exceed G2048_QNET_BATCH_MAX = %d", entry, G2048_QNET_BATCH_MAX);
    if (!good_encoder_shape(dim_ff, 1)) return fail(G2048_ERR_ARG, "%s: dim_ff must be a multiple of 32 (32 .. 65536)", entry);
    if (layer < 0 || layer >= 64) return fail(G2048_ERR_ARG, "%s: layer must be 0 .. 63", entry);
    if (site < 0 || site > 3) return fail(G2048_ERR_ARG, "%s: site must be 0 .. 3", entry);
    if (!good_qdrop(p)) return fail(G2048_ERR_ARG, "%s: p must be finite, 0 <= p < 1", entry);
    const size_t height = site == 0 ? (size_t)kHeads * n : n, width = site == 0 ? n : site == 2 ? (size_t)dim_ff : (size_t)kD;
    if (first_row > height || rows > height - first_row)
        return fail(G2048_ERR_ARG, "%s: rows %zu .. %zu lie past the site's matrix of %zu rows", entry, first_row, first_row + rows, height);
    // at most 32,768 x 4,096 or 4,096 x 65,536 elements: 32 bits hold every index
    hipLaunchKernelGGL(qt_mask_kernel, dim3(blocks_for(rows * width, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), keep_out,
                       qdrop_site(kDomQnetDropout, seed, call_index, layer, site, p), (uint32_t)(first_row * width), (uint32_t)(rows * width));
    return check_launch(entry);
}

}  // extern "C"
