// g2048_ppo_grad.hip -- the gradient half of PPOAgent.update (agents/ppo_agent.py:357-400) on the device: the TRAINING-mode
// forward of the reference's actor and critic (16-256-128-64-{4|1}, BatchNorm1d on batch statistics after the first two ReLUs,
// its running statistics moving by momentum 0.1), the returns / advantages block, the clipped-surrogate + value + entropy loss
// and the backward pass through both networks, the gradients written in the networks' plain parameter layout (include/g2048.h),
// where a stock torch optimiser reads them through views. C-ABI: g2048_ppo_train_workspace / g2048_ppo_forward_train /
// g2048_ppo_advantages / g2048_ppo_loss_grad, and with the reference's live dropout (nn.Dropout after each BatchNorm)
// g2048_ppo_forward_train_dropout / g2048_ppo_loss_grad_dropout / g2048_ppo_dropout_mask. f32 only.
//
// One phase per launch, per network:
//   fc1       relu(x W^T + b) for K = 16: one chunk of the f32 matrix cores' product, one wavefront a 16-row x 16-feature tile
//   bn        batch statistics and the normalised rows on the VALU: a block 32 features, 32 row groups; a thread adds its rows in
//             eight partial sums in a fixed order, the block combines the groups pairwise. Mean and rstd are kept for the backward.
//   fc2, fc3  qb_linear_kernel (g2048_qnet_batch_fwd.h)
//   head      a thread a row: fc4 (K = 64, 4 or 1 outputs) on the VALU, softmax; with the loss asked for, the row's loss terms,
//             d loss / d logits and the gradient into relu(fc3)'s output with its mask (M = 4 or 1 is below qg_dx_kernel's tile)
//   dw, dx    qg_dw_kernel / qg_dx_kernel (g2048_grad_products.h)
//   bn_bwd    dgamma = sum dy xhat, dbeta = sum dy, dx = gamma rstd (dy - dbeta / n - xhat dgamma / n) x the ReLU mask below it,
//             the sums as in bn
//   loss      one block's fixed-order sums of the rows' terms
//   dropout   (p > 0 only) the bn launch multiplies its output by m, the bn_bwd launch the incoming dy, m = 1 / (1 - p) or 0 from
//             one draw of the counter RNG per element (qdrop_mult): the backward regenerates it, no mask is stored. With p == 0
//             the kernels launched are the instantiations without it (pg_bn_kernel<> / pg_bn_bwd_kernel<>), whose code is unchanged.
// n == 1: the reference skips both BatchNorms; so does this (their gradients are written as 0, the running statistics stay). It
// does not skip the dropout: with p > 0 one elementwise launch each way (pg_drop_kernel / pg_drop_bwd_kernel) applies m.
// No atomics, no split-K across blocks, no block waits on another; every output element is one fixed-order accumulation, so two
// calls give the same bits; nothing past row n or past the stated sizes is read or written, and no row past n of the workspace
// is relied on. The gradient buffers are overwritten, never accumulated into. Compile with -ffp-contract=off.
// A NaN or an infinity in an input shows in the loss parts and the gradients as it does in stock torch: every ReLU, clamp and
// minimum of this pass is a comparison that passes a NaN on (relu_nan, clamp_nan, min_nan), not fmaxf / fminf, which drop it, and
// a ReLU's backward is torch's threshold_backward, zero where the output is <= 0: where the output is a NaN the gradient passes.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/g2048.h"
#include "g2048_board.h"             // rng_draw_lo, the per-element draw
#include "g2048_grad_products.h"
#include "g2048_host.h"
#include "g2048_mfma.h"
#include "g2048_ppo_head.h"
#include "g2048_qnet_batch_fwd.h"
#include "g2048_rng.h"

namespace {

constexpr int kIn = 16, kH1 = 256, kH2 = 128, kH3 = 64;
// plain layout of one network, in floats (include/g2048.h); fc4.bias follows fc4.weight's 64 n_out floats
constexpr int kFc1W = 0, kFc1B = kFc1W + kH1 * kIn, kBn1W = kFc1B + kH1, kBn1B = kBn1W + kH1, kFc2W = kBn1B + kH1, kFc2B = kFc2W + kH2 * kH1,
              kBn2W = kFc2B + kH2, kBn2B = kBn2W + kH2, kFc3W = kBn2B + kH2, kFc3B = kFc3W + kH3 * kH2, kFc4W = kFc3B + kH3;
static_assert(kFc4W == 46272, "the plain layout of include/g2048.h");
constexpr int kRun1 = 0, kRun2 = 2 * kH1, kRunFloats = 2 * kH1 + 2 * kH2;      // running: mean1 var1 mean2 var2
constexpr float kBnEps = 1e-5f, kMomentum = 0.1f;

// workspace of one network, in floats, every array [np] rows (np = n rounded up to a tile of 16; rows past n are never touched)
struct NetWorkspace {
    size_t np;
    explicit NetWorkspace(size_t n) : np((n + 15) / 16 * 16) {}
    size_t h1() const { return 0; }                                   // relu(fc1 x)
    size_t b1() const { return h1() + np * kH1; }                     // BN1's output
    size_t h2() const { return b1() + np * kH1; }
    size_t b2() const { return h2() + np * kH2; }
    size_t h3() const { return b2() + np * kH2; }
    size_t out() const { return h3() + np * kH3; }                    // [np][4]: probabilities or values, when the caller keeps none
    size_t dz() const { return out() + np * 4; }                      // [np][n_out]
    size_t d3() const { return dz() + np * 4; }
    size_t d2() const { return d3() + np * kH3; }
    size_t d1() const { return d2() + np * kH2; }
    size_t stat() const { return d1() + np * kH1; }                   // mean1 rstd1 mean2 rstd2
    size_t floats() const { return stat() + kRunFloats; }
};
// the whole workspace: actor, critic, then the rows' three loss terms
inline size_t workspace_floats(size_t n) { return 2 * NetWorkspace(n).floats() + 3 * NetWorkspace(n).np; }

// -------------------------------------------------------------------------------------------------------------- fc1 --
// Y [n][256] = relu(X [n][16] W^T + b): qb_linear_kernel's tile for one chunk of K. Lane (col, g): the A operand W[16 o + col][4 g ..],
// the B operand X[row][4 g ..]; grid (4, row tiles), four wavefronts a block.
__global__ __launch_bounds__(256) void pg_fc1_kernel(const float *__restrict__ X, const float *__restrict__ W, const float *__restrict__ bias,
                                                      float *__restrict__ Y, int n)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
    const int o = (int)blockIdx.x * 4 + wave;
    const int row = (int)blockIdx.y * 16 + col;
    const bool live = row < n;
    f4 acc = load_w(bias + 16 * o + 4 * g);
    const f4 w = load_w(W + (size_t)(16 * o + col) * kIn + 4 * g), x = live ? load_f4(X + (size_t)row * kIn + 4 * g) : splat(0.0f);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[r], x[r], acc, 0, 0, 0);
    if (live) *reinterpret_cast<f4 *>(Y + (size_t)row * kH1 + 16 * o + 4 * g) = relu_nan(acc);
}

// ---------------------------------------------------------------------------------------------------------- dropout --
// One dropout site of one launch is a QDrop (g2048_qnet_drop.h, through g2048_qnet_batch_fwd.h), domain kDomDropout: element
// (row, feature) of site s (0 after bn1, 1 after bn2) of network w (0 actor, 1 critic) is element row F + feature of stream 2 w + s.
inline QDrop drop_site(uint64_t seed, uint64_t call_index, int net, int site, double p)
{
    return QDrop(kDomDropout, seed, call_index, (uint32_t)(2 * net + site), p);
}

// keep[i] = the keep bit of element i of a site, i < count
__global__ __launch_bounds__(256) void pg_drop_mask_kernel(uint8_t *__restrict__ keep, QDrop drop, uint32_t count)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < count) keep[i] = qdrop_keep(drop, i) ? 1 : 0;
}

// n == 1, where no BatchNorm launch carries the dropout: Y = X m over count elements of a site
__global__ __launch_bounds__(256) void pg_drop_kernel(const float *__restrict__ X, float *__restrict__ Y, QDrop drop, uint32_t count)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < count) Y[i] = X[i] * qdrop_mult(drop, i);
}

// its backward, in place: D = d loss / d Y leaves as d loss / d H, X = relu(H) (zero where X <= 0)
__global__ __launch_bounds__(256) void pg_drop_bwd_kernel(float *__restrict__ D, const float *__restrict__ X, QDrop drop, uint32_t count)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const float v = D[i] * qdrop_mult(drop, i);
    D[i] = X[i] <= 0.0f ? 0.0f : v;
}

// -------------------------------------------------------------------------------------------------------- BatchNorm --
// A block of 1,024 = 32 features x 32 row groups; thread (group, feature) owns the rows group, group + 32, ..: partial sum u of eight
// takes every eighth of them (eight independent loads in flight), the eight are combined pairwise, then the 32 groups pairwise
// through LDS. The same on every thread of a feature.
constexpr int kBnGroups = 32, kBnParts = 8;

// body(u, row) for every row of the thread, u = the partial sum the row belongs to
template <class Body>
__device__ inline void bn_rows(int grp, int n, Body body)
{
    int i = grp;
    for (; i + (kBnParts - 1) * kBnGroups < n; i += kBnParts * kBnGroups)
#pragma unroll
        for (int u = 0; u < kBnParts; ++u) body(u, i + kBnGroups * u);
#pragma unroll
    for (int u = 0; u < kBnParts - 1; ++u)
        if (i + kBnGroups * u < n) body(u, i + kBnGroups * u);
}

__device__ inline float bn_block_sum(const float (&a)[kBnParts], float (&red)[kBnGroups][32], int grp, int f)
{
    __syncthreads();                                 // the previous sum's readers are done with red
    red[grp][f] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    __syncthreads();
    float r[kBnGroups];
#pragma unroll
    for (int i = 0; i < kBnGroups; ++i) r[i] = red[i][f];
#pragma unroll
    for (int w = kBnGroups / 2; w > 0; w >>= 1)
#pragma unroll
        for (int i = 0; i < w; ++i) r[i] = r[2 * i] + r[2 * i + 1];
    return r[0];
}

// Y = (X - mean) rstd gamma + beta over the n rows of X [n][F] (n >= 2), mean and the biased variance of the batch; stat: mean [F],
// rstd [F] kept for the backward. running (optional): mean [F], var [F], moved by momentum 0.1 towards the batch mean and the
// UNBIASED variance, as torch's training-mode BatchNorm1d moves them. grid F / 32. With a QDrop, Y is multiplied by the site's m.
template <class... MaybeDrop>
__global__ __launch_bounds__(1024) void pg_bn_kernel(const float *__restrict__ X, int F, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                      float *__restrict__ Y, float *__restrict__ stat, float *__restrict__ running, int n,
                                                      MaybeDrop... drop)
{
    __shared__ float red[kBnGroups][32];
    const int f = threadIdx.x & 31, grp = threadIdx.x >> 5, feat = (int)blockIdx.x * 32 + f;
    const float *x = X + feat;
    float a[kBnParts];
#pragma unroll
    for (int u = 0; u < kBnParts; ++u) a[u] = 0.0f;
    bn_rows(grp, n, [&](int u, int row) { a[u] += x[(size_t)row * F]; });
    const float mean = bn_block_sum(a, red, grp, f) / (float)n;
#pragma unroll
    for (int u = 0; u < kBnParts; ++u) a[u] = 0.0f;
    bn_rows(grp, n, [&](int u, int row) {
        const float d = x[(size_t)row * F] - mean;
        a[u] += d * d;
    });
    const float ss = bn_block_sum(a, red, grp, f);
    const float rstd = 1.0f / sqrtf(ss / (float)n + kBnEps), ga = gamma[feat], be = beta[feat];
    for (int i = grp; i < n; i += kBnGroups) {
        float y = (x[(size_t)i * F] - mean) * rstd * ga + be;
        if constexpr (sizeof...(MaybeDrop) != 0) y *= qdrop_mult(drop..., (uint32_t)(i * F + feat));
        Y[(size_t)i * F + feat] = y;
    }
    if (grp == 0) {
        stat[feat] = mean;
        stat[F + feat] = rstd;
        if (running) {
            running[feat] = (1.0f - kMomentum) * running[feat] + kMomentum * mean;
            running[F + feat] = (1.0f - kMomentum) * running[F + feat] + kMomentum * (ss / (float)(n - 1));
        }
    }
}

// The backward of pg_bn_kernel, in place: D [n][F] holds d loss / d Y and leaves as d loss / d H, where X = relu(H) is the
// BatchNorm's input (zero where X <= 0; a NaN X passes the gradient, as torch's ReLU backward does). dgamma [F] = sum dy xhat, dbeta [F] = sum dy with xhat = (X - mean) rstd from stat.
// With a QDrop, D holds d loss / d (Y m), the dropped output: every dy is first multiplied by the regenerated m.
template <class... MaybeDrop>
__global__ __launch_bounds__(1024) void pg_bn_bwd_kernel(float *__restrict__ D, const float *__restrict__ X, int F, const float *__restrict__ gamma,
                                                          const float *__restrict__ stat, float *__restrict__ dgamma, float *__restrict__ dbeta, int n,
                                                          MaybeDrop... drop)
{
    __shared__ float red[kBnGroups][32];
    const int f = threadIdx.x & 31, grp = threadIdx.x >> 5, feat = (int)blockIdx.x * 32 + f;
    const float *x = X + feat;
    float *d = D + feat;
    const float mean = stat[feat], rstd = stat[F + feat];
    float a[kBnParts], b[kBnParts];
#pragma unroll
    for (int u = 0; u < kBnParts; ++u) a[u] = b[u] = 0.0f;
    bn_rows(grp, n, [&](int u, int row) {
        float dy = d[(size_t)row * F];
        if constexpr (sizeof...(MaybeDrop) != 0) dy *= qdrop_mult(drop..., (uint32_t)(row * F + feat));
        a[u] += dy;
        b[u] += dy * ((x[(size_t)row * F] - mean) * rstd);
    });
    const float db = bn_block_sum(a, red, grp, f), dg = bn_block_sum(b, red, grp, f);
    const float scale = gamma[feat] * rstd, mb = db / (float)n, mg = dg / (float)n;
    for (int i = grp; i < n; i += kBnGroups) {
        const float xv = x[(size_t)i * F];
        float dy = d[(size_t)i * F];
        if constexpr (sizeof...(MaybeDrop) != 0) dy *= qdrop_mult(drop..., (uint32_t)(i * F + feat));
        const float v = scale * (dy - mb - (xv - mean) * rstd * mg);
        d[(size_t)i * F] = xv <= 0.0f ? 0.0f : v;
    }
    if (grp == 0) {
        dgamma[feat] = dg;
        dbeta[feat] = db;
    }
}

// ------------------------------------------------------------------------------------------------------------ heads --
// z[j] = fc4.bias[j] + fc4.weight[j] . h over K = 64: four partial sums (k & 3) of fused multiply-adds, combined pairwise
template <int O>
__device__ inline void fc4_row(const float *__restrict__ h, const float *__restrict__ W, float (&hv)[kH3], float (&z)[O])
{
#pragma unroll
    for (int k = 0; k < kH3; k += 4) {
        const f4 v = load_f4(h + k);
        hv[k] = v[0], hv[k + 1] = v[1], hv[k + 2] = v[2], hv[k + 3] = v[3];
    }
#pragma unroll
    for (int j = 0; j < O; ++j) {
        float a[4] = {W[O * kH3 + j], 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < kH3; k += 4)
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = fmaf(W[j * kH3 + k + u], hv[k + u], a[u]);
        z[j] = (a[0] + a[1]) + (a[2] + a[3]);
    }
}

// d3[k] = 0 where h[k] <= 0, else sum_j dz[j] fc4.weight[j][k] (a NaN h[k] passes it, as torch's ReLU backward does)
template <int O>
__device__ inline void fc4_row_dx(const float (&dz)[O], const float *__restrict__ W, const float (&hv)[kH3], float *__restrict__ d3)
{
#pragma unroll
    for (int k = 0; k < kH3; k += 4) {
        f4 v;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float s = dz[0] * W[k + u];
#pragma unroll
            for (int j = 1; j < O; ++j) s = fmaf(dz[j], W[j * kH3 + k + u], s);
            v[u] = hv[k + u] <= 0.0f ? 0.0f : s;
        }
        *reinterpret_cast<f4 *>(d3 + k) = v;
    }
}

// The actor's head, a thread a row: p = softmax(fc4 h3) to probs. With `actions` (the loss asked for):
//   q = p / sum(p); l = log(clamp(q, eps, 1 - eps)), eps = 2^-23 (Categorical(probs=p) in f32); ratio = exp(l[a] - old);
//   term = min(ratio A, clamp(ratio, 1 - clip, 1 + clip) A); ent = -sum l q; loss share = -term / n - ent_coef ent / n
// and its derivative: minimum splits a tie's gradient in halves, clamp passes it on [lo, hi] (edges included), a binding clamp of q
// passes none; back through the renormalisation and the softmax to dz [row][4] and through fc4 to d3 [row][64].
__global__ __launch_bounds__(64) void pg_actor_head_kernel(const float *__restrict__ h3, const float *__restrict__ W, float4 *__restrict__ probs,
                                                            const long long *__restrict__ actions, const float *__restrict__ old_log_probs,
                                                            const float *__restrict__ adv, float clip, float ent_coef, float *__restrict__ term,
                                                            float *__restrict__ ent, float4 *__restrict__ dz_out, float *__restrict__ d3, int n)
{
    const int i = (int)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    float hv[kH3], z[4];
    fc4_row<4>(h3 + (size_t)i * kH3, W, hv, z);
    const float4 p4 = softmax4(f4{z[0], z[1], z[2], z[3]});
    probs[i] = p4;
    if (!actions) return;
    const float p[4] = {p4.x, p4.y, p4.z, p4.w};
    float dz[4];
    ppo_actor_row(p, (int)(actions[i] & 3), old_log_probs[i], adv[i], clip, ent_coef, 1.0f / (float)n, term[i], ent[i], dz);
    dz_out[i] = make_float4(dz[0], dz[1], dz[2], dz[3]);
    fc4_row_dx<4>(dz, W, hv, d3 + (size_t)i * kH3);
}

// The critic's head: v = fc4 h3 to values. With `returns`: term = (v - returns)^2, dz = value_coef . 2 (v - returns) / n.
__global__ __launch_bounds__(64) void pg_critic_head_kernel(const float *__restrict__ h3, const float *__restrict__ W, float *__restrict__ values,
                                                             const float *__restrict__ returns, float value_coef, float *__restrict__ term,
                                                             float *__restrict__ dz_out, float *__restrict__ d3, int n)
{
    const int i = (int)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    float hv[kH3], z[1];
    fc4_row<1>(h3 + (size_t)i * kH3, W, hv, z);
    values[i] = z[0];
    if (!returns) return;
    const float dz[1] = {ppo_critic_row(z[0], returns[i], value_coef, n, term[i])};
    dz_out[i] = dz[0];
    fc4_row_dx<1>(dz, W, hv, d3 + (size_t)i * kH3);
}

// (the rows' terms to the four loss parts: block_sums and pg_loss_kernel, g2048_ppo_head.h)

// ------------------------------------------------------------------------------------------------------- advantages --
// ppo_agent.py:368-373 in one block of 256: thread t keeps its rows t, t + 256, .. (at most 16) in registers. The mean and the
// unbiased variance are the block's fixed-order sums (block_sums' order), the variance of the deviations from the mean.
__global__ __launch_bounds__(256) void pg_advantages_kernel(const float *__restrict__ values, const float *__restrict__ next_values,
                                                             const float *__restrict__ rewards, const float *__restrict__ dones, float gamma,
                                                             float *__restrict__ returns_out, float *__restrict__ adv_out, int n)
{
    __shared__ float red[256];
    constexpr int kRows = G2048_PPO_BATCH_MAX / 256;
    const int t = threadIdx.x;
    float adv[kRows], v = 0.0f;
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
        const int i = t + 256 * u;
        adv[u] = 0.0f;
        if (i < n) {
            const float ret = rewards[i] + gamma * next_values[i] * (1.0f - dones[i]);
            returns_out[i] = ret;
            adv[u] = ret - values[i];
            v += adv[u];
        }
    }
    if (n > 1) {
        red[t] = v;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (t < s) red[t] += red[t + s];
            __syncthreads();
        }
        const float mean = red[0] / (float)n;
        __syncthreads();
        v = 0.0f;
#pragma unroll
        for (int u = 0; u < kRows; ++u)
            if (t + 256 * u < n) {
                adv[u] -= mean;
                v += adv[u] * adv[u];
            }
        red[t] = v;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (t < s) red[t] += red[t + s];
            __syncthreads();
        }
        const float denom = sqrtf(red[0] / (float)(n - 1)) + 1e-8f;
#pragma unroll
        for (int u = 0; u < kRows; ++u) adv[u] /= denom;
    }
#pragma unroll
    for (int u = 0; u < kRows; ++u)
        if (t + 256 * u < n) adv_out[t + 256 * u] = adv[u];
}

// ------------------------------------------------------------------------------------------------------------- host --
struct Net {
    const float *P;        // plain parameters
    float *running;        // or null
    float *G;              // gradient buffer, or null (forward only)
    float *ws;             // this network's workspace
    int n_out;
    bool dropout;          // p > 0: drop[s] is site s's
    QDrop drop[2];
};

// what the dropout entry points add to a network: p, and with p > 0 the two sites' launch scalars
Net with_dropout(Net net, uint64_t seed, uint64_t call_index, int w, double p)
{
    net.dropout = p > 0.0;
    if (net.dropout)
        for (int s = 0; s < 2; ++s) net.drop[s] = drop_site(seed, call_index, w, s, p);
    return net;
}

// the training-mode forward up to relu(fc3 ..), the activations kept in net.ws. b1 / b2 (BatchNorm's outputs, dropped where the
// network has dropout) are what fc2 / fc3 and the backward's dW products read; without BatchNorm and dropout they are h1 / h2
void launch_trunk(const Net &net, const float *states, int n, hipStream_t s)
{
    const NetWorkspace w((size_t)n);
    const unsigned tiles = (unsigned)(w.np / 16);
    const bool bn = n > 1, own = bn || net.dropout;
    float *h1 = net.ws + w.h1(), *b1 = own ? net.ws + w.b1() : h1, *h2 = net.ws + w.h2(), *b2 = own ? net.ws + w.b2() : h2, *h3 = net.ws + w.h3(),
          *stat = net.ws + w.stat();
    const auto norm = [&](const float *h, int F, const float *gamma, const float *beta, float *b, float *st, float *running, const QDrop &drop) {
        if (bn && net.dropout)
            hipLaunchKernelGGL(pg_bn_kernel<QDrop>, dim3(F / 32), dim3(1024), 0, s, h, F, gamma, beta, b, st, running, n, drop);
        else if (bn)
            hipLaunchKernelGGL(pg_bn_kernel<>, dim3(F / 32), dim3(1024), 0, s, h, F, gamma, beta, b, st, running, n);
        else if (net.dropout)
            hipLaunchKernelGGL(pg_drop_kernel, dim3(blocks_for((size_t)n * F, 256)), dim3(256), 0, s, h, b, drop, (uint32_t)(n * F));
    };
    hipLaunchKernelGGL(pg_fc1_kernel, dim3(kH1 / 64, tiles), dim3(256), 0, s, states, net.P + kFc1W, net.P + kFc1B, h1, n);
    norm(h1, kH1, net.P + kBn1W, net.P + kBn1B, b1, stat, net.running ? net.running + kRun1 : nullptr, net.drop[0]);
    hipLaunchKernelGGL((qb_linear_kernel<true, true>), dim3(kH2 / 64, tiles), dim3(256), 0, s, static_cast<const float *>(b1), kH1, net.P + kFc2W,
                       net.P + kFc2B, h2, kH2, n);
    norm(h2, kH2, net.P + kBn2W, net.P + kBn2B, b2, stat + 2 * kH1, net.running ? net.running + kRun2 : nullptr, net.drop[1]);
    hipLaunchKernelGGL((qb_linear_kernel<true, true>), dim3(kH3 / 64, tiles), dim3(256), 0, s, static_cast<const float *>(b2), kH2, net.P + kFc3W,
                       net.P + kFc3B, h3, kH3, n);
}

// from dz [n][n_out] and d3 [n][64] (the head's) to every gradient of the network
int launch_backward(const Net &net, const float *states, int n, hipStream_t s, const char *entry)
{
    const NetWorkspace w((size_t)n);
    const unsigned tiles = (unsigned)(w.np / 16);
    const bool bn = n > 1, own = bn || net.dropout;
    const float *P = net.P, *none = nullptr;
    float *G = net.G;
    const float *h1 = net.ws + w.h1(), *b1 = own ? net.ws + w.b1() : h1, *h2 = net.ws + w.h2(), *b2 = own ? net.ws + w.b2() : h2, *h3 = net.ws + w.h3(),
                *stat = net.ws + w.stat(), *dz = net.ws + w.dz();
    float *d3 = net.ws + w.d3(), *d2 = net.ws + w.d2(), *d1 = net.ws + w.d1();
    const int O = net.n_out;
    const auto dx = [&](const float *dY, int M, const float *W, int K, const float *mask, float *dX) {
        hipLaunchKernelGGL(qg_dx_kernel, dim3((unsigned)(K + 63) / 64, tiles), dim3(256), 0, s, dY, M, W, K, none, mask, dX, n);
    };
    const auto dw = [&](const float *dY, int ldy, int M, const float *X, int K, float *dW, float *db) {
        hipLaunchKernelGGL(qg_dw_kernel, dim3((unsigned)(K + 63) / 64, (unsigned)(M + 15) / 16), dim3(256), 0, s, dY, ldy, M, X, K, dW, db, n);
    };
    // d [n][F] = d loss / d b (the BatchNorm's, dropped, output) to d loss / d (fc's output before its ReLU), in place
    const auto norm_bwd = [&](float *d, const float *h, int F, const float *gamma, const float *st, float *dgamma, float *dbeta, const QDrop &drop) {
        if (bn && net.dropout)
            hipLaunchKernelGGL(pg_bn_bwd_kernel<QDrop>, dim3(F / 32), dim3(1024), 0, s, d, h, F, gamma, st, dgamma, dbeta, n, drop);
        else if (bn)
            hipLaunchKernelGGL(pg_bn_bwd_kernel<>, dim3(F / 32), dim3(1024), 0, s, d, h, F, gamma, st, dgamma, dbeta, n);
        else if (net.dropout)
            hipLaunchKernelGGL(pg_drop_bwd_kernel, dim3(blocks_for((size_t)n * F, 256)), dim3(256), 0, s, d, h, drop, (uint32_t)(n * F));
    };
    dw(dz, O, O, h3, kH3, G + kFc4W, G + kFc4W + O * kH3);
    dw(d3, kH3, kH3, b2, kH2, G + kFc3W, G + kFc3B);
    dx(d3, kH3, P + kFc3W, kH2, own ? none : h2, d2);
    norm_bwd(d2, h2, kH2, P + kBn2W, stat + 2 * kH1, G + kBn2W, G + kBn2B, net.drop[1]);
    dw(d2, kH2, kH2, b1, kH1, G + kFc2W, G + kFc2B);
    dx(d2, kH2, P + kFc2W, kH1, own ? none : h1, d1);
    norm_bwd(d1, h1, kH1, P + kBn1W, stat, G + kBn1W, G + kBn1B, net.drop[0]);
    dw(d1, kH1, kH1, states, kIn, G + kFc1W, G + kFc1B);
    if (!bn) {                                       // the reference's forward skips both BatchNorms for one row: no gradient
        hipError_t e = hipMemsetAsync(G + kBn1W, 0, 2 * kH1 * sizeof(float), s);
        if (e == hipSuccess) e = hipMemsetAsync(G + kBn2W, 0, 2 * kH2 * sizeof(float), s);
        if (e != hipSuccess) return fail(G2048_ERR_HIP, "%s: hipMemsetAsync: %s", entry, hipGetErrorString(e));
    }
    return G2048_OK;
}


// g2048_ppo_forward_train and g2048_ppo_forward_train_dropout (`entry`: whose messages); the first is net 0, p 0
int forward_train(const char *entry, const float *states, const float *plain, float *running_or_null, int n_out, int net_index, double p,
                  uint64_t seed, uint64_t call_index, float *out, size_t n, void *workspace, void *stream)
{
    if (n == 0) return G2048_OK;
    if (!states || !plain || !out || !workspace) return fail(G2048_ERR_ARG, "%s: null pointer", entry);
    if (!aligned(states, 16) || !aligned(plain, 16) || !aligned(workspace, 16) || !aligned(running_or_null, 4) ||
        !aligned(out, n_out == 4 ? 16 : 4))
        return fail(G2048_ERR_ARG, "%s: misaligned pointer (states, plain weights, workspace, probabilities: 16 bytes; the rest: 4)", entry);
    if (n_out != 4 && n_out != 1) return fail(G2048_ERR_ARG, "%s: n_out must be 4 (actor) or 1 (critic)", entry);
    if (net_index != 0 && net_index != 1) return fail(G2048_ERR_ARG, "%s: net must be 0 (the actor's masks) or 1 (the critic's)", entry);
    if (!good_qdrop(p)) return fail(G2048_ERR_ARG, "%s: the dropout probability must be finite, 0 <= p < 1", entry);
    if (n > G2048_PPO_BATCH_MAX)
        return fail(G2048_ERR_ARG, "%s: n must not exceed G2048_PPO_BATCH_MAX = %d (the batch statistics are the whole batch's; a larger "
                                   "batch is not truncated)", entry, G2048_PPO_BATCH_MAX);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int ni = (int)n;
    const Net net = with_dropout(Net{plain, running_or_null, nullptr, static_cast<float *>(workspace), n_out, false, {}}, seed, call_index,
                                 net_index, p);
    const float *h3 = net.ws + NetWorkspace(n).h3();
    launch_trunk(net, states, ni, s);
    if (n_out == 4)
        hipLaunchKernelGGL(pg_actor_head_kernel, dim3(blocks_for(n, 64)), dim3(64), 0, s, h3, plain + kFc4W, reinterpret_cast<float4 *>(out),
                           static_cast<const long long *>(nullptr), static_cast<const float *>(nullptr), static_cast<const float *>(nullptr), 0.0f,
                           0.0f, static_cast<float *>(nullptr), static_cast<float *>(nullptr), static_cast<float4 *>(nullptr),
                           static_cast<float *>(nullptr), ni);
    else
        hipLaunchKernelGGL(pg_critic_head_kernel, dim3(blocks_for(n, 64)), dim3(64), 0, s, h3, plain + kFc4W, out, static_cast<const float *>(nullptr),
                           0.0f, static_cast<float *>(nullptr), static_cast<float *>(nullptr), static_cast<float *>(nullptr), ni);
    return check_launch(entry);
}

// g2048_ppo_loss_grad and g2048_ppo_loss_grad_dropout; the first is p 0 for both networks
int loss_grad(const char *entry, const float *states, const int64_t *actions, const float *old_log_probs, const float *advantages,
              const float *returns, const float *plain_actor, const float *plain_critic, float *running_actor_or_null,
              float *running_critic_or_null, float clip_epsilon, float value_coef, float entropy_coef, double p_actor, double p_critic,
              uint64_t seed, uint64_t call_index, size_t n, float *grad_actor_out, float *grad_critic_out, float *loss_out, void *workspace,
              void *stream)
{
    if (n == 0) return G2048_OK;
    if (!states || !actions || !old_log_probs || !advantages || !returns || !plain_actor || !plain_critic || !grad_actor_out ||
        !grad_critic_out || !loss_out || !workspace)
        return fail(G2048_ERR_ARG, "%s: null pointer", entry);
    if (!aligned(states, 16) || !aligned(plain_actor, 16) || !aligned(plain_critic, 16) || !aligned(grad_actor_out, 16) ||
        !aligned(grad_critic_out, 16) || !aligned(workspace, 16) || !aligned(actions, 8) || !aligned(old_log_probs, 4) ||
        !aligned(advantages, 4) || !aligned(returns, 4) || !aligned(running_actor_or_null, 4) || !aligned(running_critic_or_null, 4) ||
        !aligned(loss_out, 4))
        return fail(G2048_ERR_ARG, "%s: misaligned pointer (states, plain weights, gradients, workspace: 16 bytes; actions: 8; the rest: 4)",
                    entry);
    if (!good_coef(clip_epsilon) || !good_coef(value_coef) || !good_coef(entropy_coef))
        return fail(G2048_ERR_ARG, "%s: clip_epsilon, value_coef and entropy_coef must be finite and not negative", entry);
    if (!good_qdrop(p_actor) || !good_qdrop(p_critic))
        return fail(G2048_ERR_ARG, "%s: the dropout probabilities must be finite, 0 <= p < 1", entry);
    if (n > G2048_PPO_BATCH_MAX)
        return fail(G2048_ERR_ARG, "%s: n must not exceed G2048_PPO_BATCH_MAX = %d (the batch statistics are the whole batch's; a larger "
                                   "batch is not truncated)", entry, G2048_PPO_BATCH_MAX);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int ni = (int)n;
    const NetWorkspace w(n);
    float *base = static_cast<float *>(workspace), *terms = base + 2 * w.floats();
    const Net actor = with_dropout(Net{plain_actor, running_actor_or_null, grad_actor_out, base, 4, false, {}}, seed, call_index, 0, p_actor);
    const Net critic = with_dropout(Net{plain_critic, running_critic_or_null, grad_critic_out, base + w.floats(), 1, false, {}}, seed, call_index,
                                    1, p_critic);
    launch_trunk(actor, states, ni, s);
    launch_trunk(critic, states, ni, s);
    hipLaunchKernelGGL(pg_actor_head_kernel, dim3(blocks_for(n, 64)), dim3(64), 0, s, static_cast<const float *>(actor.ws + w.h3()),
                       plain_actor + kFc4W, reinterpret_cast<float4 *>(actor.ws + w.out()), reinterpret_cast<const long long *>(actions),
                       old_log_probs, advantages, clip_epsilon, entropy_coef, terms, terms + 2 * w.np, reinterpret_cast<float4 *>(actor.ws + w.dz()),
                       actor.ws + w.d3(), ni);
    hipLaunchKernelGGL(pg_critic_head_kernel, dim3(blocks_for(n, 64)), dim3(64), 0, s, static_cast<const float *>(critic.ws + w.h3()),
                       plain_critic + kFc4W, critic.ws + w.out(), returns, value_coef, terms + w.np, critic.ws + w.dz(), critic.ws + w.d3(), ni);
    hipLaunchKernelGGL(pg_loss_kernel, dim3(1), dim3(256), 0, s, static_cast<const float *>(terms), w.np, value_coef, entropy_coef, loss_out, ni);
    int rc = launch_backward(actor, states, ni, s, entry);
    if (rc == G2048_OK) rc = launch_backward(critic, states, ni, s, entry);
    return rc == G2048_OK ? check_launch(entry) : rc;
}

}  // namespace

extern "C" {

size_t g2048_ppo_train_workspace(size_t n)
{
    if (n == 0 || n > G2048_PPO_BATCH_MAX) return 0;
    return workspace_floats(n) * sizeof(float);
}

int g2048_ppo_forward_train(const float *states, const float *plain, float *running_or_null, int n_out, float *out, size_t n, void *workspace,
                            void *stream)
{
    return forward_train("g2048_ppo_forward_train", states, plain, running_or_null, n_out, 0, 0.0, 0, 0, out, n, workspace, stream);
}

int g2048_ppo_forward_train_dropout(const float *states, const float *plain, float *running_or_null, int n_out, int net, double p, uint64_t seed,
                                    uint64_t call_index, float *out, size_t n, void *workspace, void *stream)
{
    return forward_train("g2048_ppo_forward_train_dropout", states, plain, running_or_null, n_out, net, p, seed, call_index, out, n, workspace,
                         stream);
}

int g2048_ppo_dropout_mask(uint64_t seed, uint64_t call_index, int net, int site, double p, uint8_t *keep_out, size_t n, void *stream)
{
    if (n == 0) return G2048_OK;
    if (!keep_out) return fail(G2048_ERR_ARG, "g2048_ppo_dropout_mask: null pointer");
    if ((net != 0 && net != 1) || (site != 0 && site != 1))
        return fail(G2048_ERR_ARG, "g2048_ppo_dropout_mask: net must be 0 (actor) or 1 (critic), site 0 (after bn1, 256 features) or 1 (after "
                                   "bn2, 128)");
    if (!good_qdrop(p)) return fail(G2048_ERR_ARG, "g2048_ppo_dropout_mask: the dropout probability must be finite, 0 <= p < 1");
    if (n > G2048_PPO_BATCH_MAX) return fail(G2048_ERR_ARG, "g2048_ppo_dropout_mask: n must not exceed G2048_PPO_BATCH_MAX = %d", G2048_PPO_BATCH_MAX);
    const uint32_t count = (uint32_t)n * (uint32_t)(site == 0 ? kH1 : kH2);
    hipLaunchKernelGGL(pg_drop_mask_kernel, dim3(blocks_for(count, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), keep_out,
                       drop_site(seed, call_index, net, site, p), count);
    return check_launch("g2048_ppo_dropout_mask");
}

int g2048_ppo_advantages(const float *values, const float *next_values, const float *rewards, const float *dones, float gamma,
                         float *returns_out, float *adv_out, size_t n, void *stream)
{
    if (n == 0) return G2048_OK;
    if (!values || !next_values || !rewards || !dones || !returns_out || !adv_out) return fail(G2048_ERR_ARG, "g2048_ppo_advantages: null pointer");
    if (!aligned(values, 4) || !aligned(next_values, 4) || !aligned(rewards, 4) || !aligned(dones, 4) || !aligned(returns_out, 4) ||
        !aligned(adv_out, 4))
        return fail(G2048_ERR_ARG, "g2048_ppo_advantages: misaligned pointer (4 bytes)");
    if (!std::isfinite(gamma)) return fail(G2048_ERR_ARG, "g2048_ppo_advantages: gamma must be finite");
    if (n > G2048_PPO_BATCH_MAX)
        return fail(G2048_ERR_ARG, "g2048_ppo_advantages: n must not exceed G2048_PPO_BATCH_MAX = %d (one block normalises the whole batch; "
                                   "a larger batch is not truncated)", G2048_PPO_BATCH_MAX);
    hipLaunchKernelGGL(pg_advantages_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), values, next_values, rewards, dones, gamma,
                       returns_out, adv_out, (int)n);
    return check_launch("g2048_ppo_advantages");
}

int g2048_ppo_loss_grad(const float *states, const int64_t *actions, const float *old_log_probs, const float *advantages, const float *returns,
                        const float *plain_actor, const float *plain_critic, float *running_actor_or_null, float *running_critic_or_null,
                        float clip_epsilon, float value_coef, float entropy_coef, size_t n, float *grad_actor_out, float *grad_critic_out,
                        float *loss_out, void *workspace, void *stream)
{
    return loss_grad("g2048_ppo_loss_grad", states, actions, old_log_probs, advantages, returns, plain_actor, plain_critic, running_actor_or_null,
                     running_critic_or_null, clip_epsilon, value_coef, entropy_coef, 0.0, 0.0, 0, 0, n, grad_actor_out, grad_critic_out, loss_out,
                     workspace, stream);
}

int g2048_ppo_loss_grad_dropout(const float *states, const int64_t *actions, const float *old_log_probs, const float *advantages,
                                const float *returns, const float *plain_actor, const float *plain_critic, float *running_actor_or_null,
                                float *running_critic_or_null, float clip_epsilon, float value_coef, float entropy_coef, double p_actor,
                                double p_critic, uint64_t seed, uint64_t call_index, size_t n, float *grad_actor_out, float *grad_critic_out,
                                float *loss_out, void *workspace, void *stream)
{
    return loss_grad("g2048_ppo_loss_grad_dropout", states, actions, old_log_probs, advantages, returns, plain_actor, plain_critic,
                     running_actor_or_null, running_critic_or_null, clip_epsilon, value_coef, entropy_coef, p_actor, p_critic, seed, call_index, n,
                     grad_actor_out, grad_critic_out, loss_out, workspace, stream);
}

}  // extern "C"
