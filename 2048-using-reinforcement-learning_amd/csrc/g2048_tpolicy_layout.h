// g2048_tpolicy_layout.h -- the transformer policy's shapes and its PLAIN f32 parameter layout (g2048_tpolicy_pack's input;
// include/g2048.h), written down once for the three files that read it: g2048_tpolicy.hip (pack, forward, complete games),
// g2048_tpolicy_grad.hip (the loss and gradient pass, libg2048_tlearn_hip.so) and g2048_tpolicy_step.hip (clipping and Adam,
// libg2048_tstep_hip.so), and for g2048_tpolicy_forward.h, through which g2048_tpolicy_collect.hip reads it too. Constants only;
// per translation unit.
#pragma once

namespace {

constexpr int kD = 64, kHeads = 4, kTok = 16, kFc1 = 128, kFc2 = 64, kFlat = kTok * kD;

// emb.w emb.b | per layer: in_proj_weight in_proj_bias out_proj.weight out_proj.bias linear1.weight linear1.bias linear2.weight
// linear2.bias norm1.w norm1.b norm2.w norm2.b eps1 eps2 | fc1.w fc1.b fc2.w fc2.b actor.w actor.b critic.w critic.b
constexpr int kPlainEmb = 0, kPlainLayer0 = 2 * kD;
constexpr int kPlInW = 0, kPlInB = kPlInW + 3 * kD * kD, kPlOutW = kPlInB + 3 * kD, kPlOutB = kPlOutW + kD * kD, kPlW1 = kPlOutB + kD;
__host__ __device__ constexpr int pl_b1(int ff) { return kPlW1 + ff * kD; }
__host__ __device__ constexpr int pl_w2(int ff) { return pl_b1(ff) + ff; }
__host__ __device__ constexpr int pl_b2(int ff) { return pl_w2(ff) + kD * ff; }
__host__ __device__ constexpr int pl_norm(int ff) { return pl_b2(ff) + kD; }             // norm1.w norm1.b norm2.w norm2.b eps1 eps2
__host__ __device__ constexpr int pl_layer(int ff) { return pl_norm(ff) + 4 * kD + 2; }
constexpr int kPlFc1W = 0, kPlFc1B = kPlFc1W + kFc1 * kFlat, kPlFc2W = kPlFc1B + kFc1, kPlFc2B = kPlFc2W + kFc2 * kFc1,
              kPlActW = kPlFc2B + kFc2, kPlActB = kPlActW + 4 * kD, kPlCriW = kPlActB + 4, kPlCriB = kPlCriW + kD, kPlTail = kPlCriB + 1;

}  // namespace
