// g2048_ppo_head.h -- the head arithmetic of PPOAgent.update()'s loss (agents/ppo_agent.py:378-400), shared by the two passes that
// differentiate it: g2048_ppo_grad.hip (the MLP actor and critic) and g2048_tpolicy_grad.hip (the transformer policy's two heads,
// libg2048_tlearn_hip.so). One row's clipped-surrogate and entropy terms with their derivative back to the logits, the critic's
// squared error, and the fixed-order reduction of the rows' terms into the four loss parts. Device code, included by those two
// files and nothing else; every kernel is per translation unit. What it does at its edges (Categorical's clamp, a tie of min / clamp,
// a NaN advantage) is what tests/test_gpu_ppo_update_edges.py pins.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// torch.clamp and torch.min: a NaN operand gives NaN, where fminf / fmaxf return the operand that is none. Plain comparisons; for
// finite operands (lo <= hi) the values are fminf(fmaxf(x, lo), hi) and fminf(a, b).
__device__ inline float clamp_nan(float x, float lo, float hi) { return x < lo ? lo : x > hi ? hi : x; }
__device__ inline float min_nan(float a, float b) { return (a < b || a != a) ? a : b; }

// One row of the actor's loss from its softmax p:
//   q = p / sum(p); l = log(clamp(q, eps, 1 - eps)), eps = 2^-23 (Categorical(probs=p) in f32); ratio = exp(l[a] - old);
//   term = min(ratio A, clamp(ratio, 1 - clip, 1 + clip) A); ent = -sum l q; loss share = -term / n - ent_coef ent / n
// and its derivative: minimum splits a tie's gradient in halves, clamp passes it on [lo, hi] (edges included), a binding clamp of q
// passes none; back through the renormalisation and the softmax to dz, d loss / d logits.
__device__ inline void ppo_actor_row(const float (&p)[4], int a, float old_log_prob, float A, float clip, float ent_coef, float inv_n,
                                     float &term, float &ent, float (&dz)[4])
{
    const float eps = 1.1920928955078125e-07f;
    const float s = ((p[0] + p[1]) + p[2]) + p[3];
    float q[4], l[4], e = 0.0f;
    bool open[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        q[j] = p[j] / s;
        open[j] = q[j] >= eps && q[j] <= 1.0f - eps;
        l[j] = logf(clamp_nan(q[j], eps, 1.0f - eps));
        e += l[j] * q[j];
    }
    const float ratio = expf(l[a] - old_log_prob), lo = 1.0f - clip, hi = 1.0f + clip;
    const float s1 = ratio * A, s2 = clamp_nan(ratio, lo, hi) * A;
    term = min_nan(s1, s2);
    ent = -e;
    const float g1 = s1 < s2 ? 1.0f : s1 == s2 ? 0.5f : 0.0f, g2 = s2 < s1 ? 1.0f : s1 == s2 ? 0.5f : 0.0f;
    const float dratio = -inv_n * (g1 * A + (ratio >= lo && ratio <= hi ? g2 * A : 0.0f));
    const float dla = dratio * ratio, ce = ent_coef * inv_n;
    float gq[4], gp[4], dot = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float dl = ce * q[j] + (j == a ? dla : 0.0f);                 // d loss / d l[j]: the entropy's l q, the taken action's ratio
        gq[j] = ce * l[j] + (open[j] ? dl / q[j] : 0.0f);
        dot += gq[j] * p[j];
    }
    float dot2 = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        gp[j] = gq[j] / s - dot / (s * s);
        dot2 += gp[j] * p[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) dz[j] = p[j] * (gp[j] - dot2);
}

// One row of the critic's loss: term = (v - returns)^2; returns d loss / d v = value_coef . 2 (v - returns) / n.
__device__ inline float ppo_critic_row(float v, float ret, float value_coef, int n, float &term)
{
    const float d = v - ret;
    term = d * d;
    return value_coef * (2.0f * d) / (float)n;
}

// One block's fixed-order sums: thread t adds its rows t, t + 256, .. in order, then a fixed tree over the 256 threads, for each
// of K arrays of n floats, `stride` apart; the sums are left in red[k][0].
template <int K>
__device__ inline void block_sums(const float *__restrict__ terms, size_t stride, int n, float (&red)[K][256])
{
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float v = 0.0f;
        for (int i = t; i < n; i += 256) v += terms[k * stride + i];
        red[k][t] = v;
    }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s)
#pragma unroll
            for (int k = 0; k < K; ++k) red[k][t] += red[k][t + s];
        __syncthreads();
    }
}

// terms: the actor's min(..) [n], the critic's squared errors, the entropies. out = {loss, actor_loss, value_loss, entropy}
__global__ __launch_bounds__(256) void pg_loss_kernel(const float *__restrict__ terms, size_t stride, float value_coef, float ent_coef,
                                                       float *__restrict__ out, int n)
{
    __shared__ float red[3][256];
    block_sums<3>(terms, stride, n, red);
    if (threadIdx.x == 0) {
        const float actor = -(red[0][0] / (float)n), value = red[1][0] / (float)n, entropy = red[2][0] / (float)n;
        out[0] = actor + value_coef * value - ent_coef * entropy;
        out[1] = actor;
        out[2] = value;
        out[3] = entropy;
    }
}

}  // namespace
