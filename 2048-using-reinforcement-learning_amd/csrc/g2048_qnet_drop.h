// g2048_qnet_drop.h -- one dropout site of one launch of an encoder network's training passes (DESIGN.md "RNG"): the Q-network's
// (domain kDomQnetDropout; csrc/g2048_qnet_train.hip launches them, the kernels that apply them are the shared ones of
// g2048_qnet_batch_fwd.h, g2048_grad_products.h and g2048_qnet_grad_bwd.h, instantiated with a QDrop as their trailing argument) and
// the transformer policy's (domain kDomTpolicyDropout; csrc/g2048_tpolicy_train.hip, g2048_tpolicy_grad_pass.h). Element e of site s
// (0 the attention probabilities, 1 dropout1, 2 the hidden layer's dropout, 3 dropout2) of encoder layer L in the library call with
// index c draws h = rng_draw(k0, k1, ((4 L + s) << 32) | e, 0), (k0, k1) = rng_keys(seed, the network's domain, c), and is kept iff
// h >= T = floor(p_s 2^32). The id's high word is the launch's, so it is folded into k1h on the host and the lane hashes 32 bits
// (rng_draw_lo), as drop_site / drop_keep of g2048_ppo_grad.hip do for the PPO networks. Device and host code, per translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "g2048_board.h"             // rng_draw_lo, the per-element draw
#include "g2048_rng.h"

namespace {

using namespace g2048;

struct QDrop {
    uint32_t k0, k1h, T;
    float scale;           // (float)(1 / (1 - p))
};

__device__ inline bool qdrop_keep(const QDrop &d, uint32_t e) { return rng_draw_lo(d.k0, d.k1h, e, 0) >= d.T; }
// the multiplier: a product, not a select, so that a NaN or an infinity in a dropped position becomes NaN as in torch
__device__ inline float qdrop_mult(const QDrop &d, uint32_t e) { return qdrop_keep(d, e) ? d.scale : 0.0f; }

// domain: kDomQnetDropout or kDomTpolicyDropout (g2048_rng.h), the network's own
inline QDrop qdrop_site(uint32_t domain, uint64_t seed, uint64_t call_index, int layer, int site, double p)
{
    const Keys k = rng_keys(seed, domain, call_index);
    return QDrop{k.k0, k.k1 + rng_hi_term((uint64_t)(4 * layer + site) << 32), (uint32_t)std::floor(p * 4294967296.0), (float)(1.0 / (1.0 - p))};
}

inline bool good_qdrop(double p) { return p >= 0.0 && p < 1.0; }      // a NaN fails both

}  // namespace
