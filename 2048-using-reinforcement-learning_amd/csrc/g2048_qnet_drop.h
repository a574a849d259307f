// g2048_qnet_drop.h -- the dropout kit of the training passes (DESIGN.md "RNG"): one dropout site of one launch (QDrop), the four
// sites of an encoder layer (DropSites), the launch that picks a kernel's instantiation with or without a QDrop (launch_site), the
// two elementwise kernels (keep bits for the tests, x m for sites 1 and 3 of the backward), and the host side the *_dropout_mask
// entry points and the p4 check share. Used by the Q-network's passes (domain kDomQnetDropout; g2048_qnet_batch_fwd.h,
// g2048_qnet_grad_bwd.h, g2048_grad_products.h; the entry points are csrc/g2048_qnet_train.hip's), the transformer policy's (domain
// kDomTpolicyDropout; g2048_tpolicy_grad_pass.h, csrc/g2048_tpolicy_train.hip) and the PPO networks' (domain kDomDropout;
// g2048_ppo_grad.hip). Element e of the launch with 32-bit stream id t in the library call with index c draws
// h = rng_draw(k0, k1, (t << 32) | e, 0), (k0, k1) = rng_keys(seed, the network's domain, c), and is kept iff h >= T = floor(p 2^32).
// The id's high word is the launch's, so it is folded into k1h on the host and the lane hashes 32 bits (rng_draw_lo). An encoder's
// stream id is 4 L + s for site s (0 the attention probabilities, 1 dropout1, 2 the hidden layer's dropout, 3 dropout2) of layer L;
// the PPO networks' is 2 net + site. Device and host code, per translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "g2048_board.h"             // rng_draw_lo, the per-element draw
#include "g2048_host.h"
#include "g2048_rng.h"

namespace {

using namespace g2048;

struct QDrop {
    uint32_t k0, k1h, T;
    float scale;           // (float)(1 / (1 - p))
    QDrop() = default;
    QDrop(uint32_t domain, uint64_t seed, uint64_t call_index, uint32_t stream, double p)
        : T((uint32_t)std::floor(p * 4294967296.0)), scale((float)(1.0 / (1.0 - p)))
    {
        const Keys k = rng_keys(seed, domain, call_index);
        k0 = k.k0;
        k1h = k.k1 + rng_hi_term((uint64_t)stream << 32);
    }
};

__device__ inline bool qdrop_keep(const QDrop &d, uint32_t e) { return rng_draw_lo(d.k0, d.k1h, e, 0) >= d.T; }
// the multiplier: a product, not a select, so that a NaN or an infinity in a dropped position becomes NaN as in torch
__device__ inline float qdrop_mult(const QDrop &d, uint32_t e) { return qdrop_keep(d, e) ? d.scale : 0.0f; }

// domain: kDomQnetDropout or kDomTpolicyDropout (g2048_rng.h), the network's own
inline QDrop qdrop_site(uint32_t domain, uint64_t seed, uint64_t call_index, int layer, int site, double p)
{
    return QDrop(domain, seed, call_index, (uint32_t)(4 * layer + site), p);
}

inline bool good_qdrop(double p) { return p >= 0.0 && p < 1.0; }      // a NaN fails both

// the four sites of one encoder layer of one call: at(s) is site s's QDrop where p4[s] > 0, else null. p4 null (an eval-mode pass):
// every site is off.
struct DropSites {
    QDrop d[4];
    bool on[4] = {false, false, false, false};
    DropSites(uint32_t domain, uint64_t seed, uint64_t call_index, int layer, const double *p4)
    {
        for (int s = 0; p4 && s < 4; ++s)
            if ((on[s] = p4[s] > 0.0)) d[s] = qdrop_site(domain, seed, call_index, layer, s, p4[s]);
    }
    const QDrop *at(int s) const { return on[s] ? &d[s] : nullptr; }
};

// One launch of a kernel that is a template on a trailing `MaybeDrop...` pack. `kernel` is a generic lambda that names it:
// [](auto... d) { return some_kernel<decltype(d)...>; }. With a live site (kDrop and d not null) the launch is the QDrop instantiation
// with *d as its last argument, else the instantiation without one: the eval-mode kernel. With kDrop false the QDrop instantiation
// is never named, so the code object does not hold it.
template <bool kDrop, class Kernel, class... Args>
void launch_site(const QDrop *d, Kernel kernel, dim3 grid, dim3 block, hipStream_t s, Args... args)
{
    if constexpr (kDrop) {
        if (d) {
            hipLaunchKernelGGL(kernel(*d), grid, block, 0, s, args..., *d);
            return;
        }
    }
    hipLaunchKernelGGL(kernel(), grid, block, 0, s, args...);
}

// The two elementwise kernels are templates so that only the library that launches them holds them.
// Y[i] = X[i] m_i over the rows x width elements of site 1 or 3 (element row width + feature = i)
template <class Drop>
__global__ __launch_bounds__(256) void qt_scale_kernel(const float *__restrict__ X, float *__restrict__ Y, Drop drop, uint32_t count)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < count) Y[i] = X[i] * qdrop_mult(drop, i);
}

// keep[i] = the keep bit of element first + i of a site, i < count
template <class Drop>
__global__ __launch_bounds__(256) void qt_mask_kernel(uint8_t *__restrict__ keep, Drop drop, uint32_t first, uint32_t count)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < count) keep[i] = qdrop_keep(drop, first + i) ? 1 : 0;
}

inline int check_p(const char *entry, const double *p4)
{
    if (!p4) return fail(G2048_ERR_ARG, "%s: null pointer", entry);
    for (int s = 0; s < 4; ++s)
        if (!good_qdrop(p4[s])) return fail(G2048_ERR_ARG, "%s: p[%d] must be finite, 0 <= p < 1", entry, s);
    return G2048_OK;
}

// What the encoders' two *_dropout_mask entry points do: rows first_row .. first_row + rows of the site's height x width matrix of
// keep bits. limit, limit_name: the network's batch limit and the macro that names it. Both networks' matrices hold at most 2^31
// elements (the callers say why), so 32 bits hold every index. A template so that only a library that calls it holds the kernel.
template <class Drop = QDrop>
int dropout_mask(const char *entry, uint32_t domain, size_t limit, const char *limit_name, uint64_t seed, uint64_t call_index, int layer,
                        int site, double p, size_t n, int dim_ff, size_t height, size_t width, size_t first_row, size_t rows, uint8_t *keep_out,
                        void *stream)
{
    if (n == 0 || rows == 0) return G2048_OK;
    if (!keep_out) return fail(G2048_ERR_ARG, "%s: null pointer", entry);
    if (n > limit) return fail(G2048_ERR_ARG, "%s: n must not exceed %s = %zu", entry, limit_name, limit);
    if (!good_encoder_shape(dim_ff, 1)) return fail(G2048_ERR_ARG, "%s: dim_ff must be a multiple of 32 (32 .. 65536)", entry);
    if (layer < 0 || layer >= 64) return fail(G2048_ERR_ARG, "%s: layer must be 0 .. 63", entry);
    if (site < 0 || site > 3) return fail(G2048_ERR_ARG, "%s: site must be 0 .. 3", entry);
    if (!good_qdrop(p)) return fail(G2048_ERR_ARG, "%s: p must be finite, 0 <= p < 1", entry);
    if (first_row > height || rows > height - first_row)
        return fail(G2048_ERR_ARG, "%s: rows %zu .. %zu lie past the site's matrix of %zu rows", entry, first_row, first_row + rows, height);
    hipLaunchKernelGGL(qt_mask_kernel<Drop>, dim3(blocks_for(rows * width, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), keep_out,
                       Drop(domain, seed, call_index, (uint32_t)(4 * layer + site), p), (uint32_t)(first_row * width), (uint32_t)(rows * width));
    return check_launch(entry);
}

}  // namespace
