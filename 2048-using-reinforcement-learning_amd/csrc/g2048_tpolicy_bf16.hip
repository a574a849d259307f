// g2048_tpolicy_bf16.hip -- libg2048_tbf16_hip.so (include/g2048_tbf16.h): the transformer policy's loss and gradient pass with the
// seven feed-forward products of every encoder layer in bf16 on the matrix cores, h and dh stored as bf16. A library of its own
// because the training library's export table is closed. The workspace, the f32 kernels and the launch sequence are
// g2048_tpolicy_grad_pass.h's, instantiated here a third time as tg_pass<true, true>; the three bf16 products and the pack launch are
// g2048_tpolicy_bf16.h's. What is rounded where is in the public header. The rules are g2048_tpolicy_grad.hip's: no atomics, every
// output element one fixed-order accumulation, two calls with the same (seed, call index) give the same bits, nothing past row n
// or the stated workspace is read or written. Compile with -ffp-contract=off.
// Below the pass: the three products as entry points of their own for the tests (the header's testing section).
#include "../../include/g2048_tbf16.h"
#include "g2048_tpolicy_grad_pass.h"

namespace {

constexpr size_t kTestRows = 16 * G2048_TLEARN_BATCH_MAX;

size_t bf16_bytes(size_t n, int dim_ff, int n_layers)
{
    return good_shape(n, dim_ff, n_layers) ? Workspace(n, dim_ff, n_layers, true).bf16_floats() * sizeof(float) : 0;
}

// the checks the three product entry points share; `kind`: (input is bf16) | (output or second input is bf16) << 1
int test_check(const char *entry, size_t n, int contraction, int contraction_unit, int other, bool pointers, bool all_aligned, int kind,
               size_t needed, size_t workspace_bytes)
{
    if (!pointers) return fail(G2048_ERR_ARG, "%s: null pointer", entry);
    if (!all_aligned) return fail(G2048_ERR_ARG, "%s: misaligned pointer (every array: 16 bytes)", entry);
    if (n > kTestRows) return fail(G2048_ERR_ARG, "%s: n must not exceed %zu rows", entry, kTestRows);
    if (contraction < contraction_unit || contraction % contraction_unit || other < 16 || other % 16 || contraction > 65536 || other > 65536)
        return fail(G2048_ERR_ARG, "%s: extents must be multiples of 16 (the contraction: of %d) in 16 .. 65536", entry, contraction_unit);
    if (kind == 3) return fail(G2048_ERR_ARG, "%s: at most one of the two arrays is bf16", entry);
    if (workspace_bytes < needed) return fail(G2048_ERR_ARG, "%s: workspace of %zu bytes, %zu needed", entry, workspace_bytes, needed);
    return G2048_OK;
}

void pack_one(const float *w, int rows, int cols, __bf16 *plain, __bf16 *trans, hipStream_t s)
{
    hipLaunchKernelGGL(tb_pack_kernel<>, dim3(blocks_for((size_t)rows * cols, 256), 1), dim3(256), 0, s, w, rows, cols, plain, trans,
                       static_cast<const float *>(nullptr), 0, 0, static_cast<__bf16 *>(nullptr), static_cast<__bf16 *>(nullptr));
}

template <bool DX, bool RELU, class TX, class TY>
void product(const void *x, int K, const __bf16 *w, const float *bias, const float *res, const void *mask, void *y, int M, size_t n, hipStream_t s)
{
    hipLaunchKernelGGL((tb_linear_kernel<DX, RELU, TX, TY>), dim3((unsigned)(M + 63) / 64, (unsigned)((n + 15) / 16)), dim3(256), 0, s,
                       static_cast<const TX *>(x), K, w, bias, res, static_cast<const __bf16 *>(mask), static_cast<TY *>(y), M, (int)n);
}

template <bool DX, bool RELU>
void product_kind(int kind, const void *x, int K, const __bf16 *w, const float *bias, const float *res, const void *mask, void *y, int M, size_t n,
                  hipStream_t s)
{
    if (kind == 0) product<DX, RELU, float, float>(x, K, w, bias, res, mask, y, M, n, s);
    else if (kind == 2) product<DX, RELU, float, __bf16>(x, K, w, bias, res, mask, y, M, n, s);
    else product<DX, RELU, __bf16, float>(x, K, w, bias, res, mask, y, M, n, s);
}

template <class TA, class TB>
void weight_gradient(const void *dy, int M, const void *x, int K, float *part, float *bpart, size_t n, int chunks, hipStream_t s)
{
    hipLaunchKernelGGL((tb_dw_split_kernel<TA, TB>), dim3((unsigned)(K + 63) / 64, (unsigned)(M + 63) / 64, (unsigned)chunks), dim3(256), 0, s,
                       static_cast<const TA *>(dy), M, static_cast<const TB *>(x), K, part, bpart, (int)n, kRowChunk);
}

}  // namespace

extern "C" {

const char *g2048_tbf16_last_error(void) { return g_err; }

int g2048_tbf16_abi_version(void) { return G2048_TBF16_ABI_VERSION; }

size_t g2048_tpolicy_bf16_workspace(size_t n, int dim_ff, int n_layers) { return bf16_bytes(n, dim_ff, n_layers); }

int g2048_tpolicy_loss_grad_bf16(const void *boards, const float *plain_f32, const int64_t *actions, const float *old_log_probs,
                                 const float *advantages, const float *returns, size_t n, int dim_ff, int n_layers, const double *p4, uint64_t seed,
                                 uint64_t call_index, float clip_epsilon, float value_coef, float entropy_coef, float *grad_out, float *losses4_out,
                                 float *probs_out, float *value_out, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *entry = "g2048_tpolicy_loss_grad_bf16";
    if (n == 0) return G2048_OK;
    const TgCall c{boards, plain_f32, actions, old_log_probs, advantages, returns, n, dim_ff, n_layers, clip_epsilon, value_coef, entropy_coef,
                   grad_out, losses4_out, probs_out, value_out, workspace, workspace_bytes, stream, true, p4, seed, call_index};
    if (const int rc = tg_check(entry, c, bf16_bytes(n, dim_ff, n_layers), "g2048_tpolicy_bf16_workspace")) return rc;
    if (p4)
        if (const int rc = check_p(entry, p4)) return rc;
    return tg_pass<true, true>(entry, c, kDomTpolicyDropout);
}

int g2048_tbf16_test_linear(const void *x, int x_bf16, const float *w, const float *bias, const float *res, void *y, int y_bf16, int relu, size_t n,
                            int K, int M, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *entry = "g2048_tbf16_test_linear";
    if (n == 0) return G2048_OK;
    const int kind = (x_bf16 ? 1 : 0) | (y_bf16 ? 2 : 0);
    if (const int rc = test_check(entry, n, K, 32, M, x && w && y && workspace,
                                  aligned(x, 16) && aligned(w, 16) && aligned(bias, 16) && aligned(res, 16) && aligned(y, 16) && aligned(workspace, 16),
                                  kind, (size_t)M * K * 2, workspace_bytes))
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    __bf16 *wb = static_cast<__bf16 *>(workspace);
    pack_one(w, M, K, wb, nullptr, s);
    if (relu) product_kind<false, true>(kind, x, K, wb, bias, res, nullptr, y, M, n, s);
    else product_kind<false, false>(kind, x, K, wb, bias, res, nullptr, y, M, n, s);
    return check_launch(entry);
}

int g2048_tbf16_test_dx(const void *dy, int dy_bf16, const float *w, const float *res, const void *mask_bf16, void *dx, int dx_bf16, size_t n, int M,
                        int K, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *entry = "g2048_tbf16_test_dx";
    if (n == 0) return G2048_OK;
    const int kind = (dy_bf16 ? 1 : 0) | (dx_bf16 ? 2 : 0);
    if (const int rc = test_check(entry, n, M, 32, K, dy && w && dx && workspace,
                                  aligned(dy, 16) && aligned(w, 16) && aligned(res, 16) && aligned(mask_bf16, 16) && aligned(dx, 16) &&
                                      aligned(workspace, 16),
                                  kind, (size_t)M * K * 2, workspace_bytes))
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    __bf16 *wt = static_cast<__bf16 *>(workspace);                         // [K][M]: the contraction along the rows
    pack_one(w, M, K, nullptr, wt, s);
    product_kind<true, false>(kind, dy, M, wt, nullptr, res, mask_bf16, dx, K, n, s);
    return check_launch(entry);
}

int g2048_tbf16_test_dw(const void *dy, int dy_bf16, const void *x, int x_bf16, float *dw, float *db, size_t n, int M, int K, void *workspace,
                        size_t workspace_bytes, void *stream)
{
    const char *entry = "g2048_tbf16_test_dw";
    if (n == 0) return G2048_OK;
    const int kind = (dy_bf16 ? 1 : 0) | (x_bf16 ? 2 : 0);
    const size_t chunks = row_chunks(n <= kTestRows ? n : 1);
    if (const int rc = test_check(entry, n, M, 16, K, dy && x && dw && db && workspace,
                                  aligned(dy, 16) && aligned(x, 16) && aligned(dw, 16) && aligned(db, 16) && aligned(workspace, 16), kind,
                                  chunks * ((size_t)M * K + M) * sizeof(float), workspace_bytes))
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *part = static_cast<float *>(workspace), *bpart = part + chunks * (size_t)M * K;
    if (kind == 0) weight_gradient<float, float>(dy, M, x, K, part, bpart, n, (int)chunks, s);
    else if (kind == 2) weight_gradient<float, __bf16>(dy, M, x, K, part, bpart, n, (int)chunks, s);
    else weight_gradient<__bf16, float>(dy, M, x, K, part, bpart, n, (int)chunks, s);
    hipLaunchKernelGGL(tg_combine_kernel, dim3(blocks_for((size_t)M * K, 256)), dim3(256), 0, s, static_cast<const float *>(part), (int)chunks,
                       (size_t)M * K, dw);
    hipLaunchKernelGGL(tg_combine_kernel, dim3(blocks_for((size_t)M, 256)), dim3(256), 0, s, static_cast<const float *>(bpart), (int)chunks, (size_t)M,
                       db);
    return check_launch(entry);
}

}  // extern "C"
