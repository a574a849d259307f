// Host-only program over the host side of csrc/g2048_step_common.h, what the three optimiser-step entry points build their
// scalars, their refusals and their workspaces from. No device and no HIP call; built with ASan + UBSan (Makefile). Prints one
// line per failed check and "step_common_host: N checks, 0 failed" at the end; the exit status is the number of failures.
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "g2048_step_common.h"
#include "g2048_tpolicy_layout.h"

using namespace g2048;

static int checks = 0, failed = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        ++checks;                                                          \
        if (!(cond)) {                                                     \
            ++failed;                                                      \
            printf("FAILED line %d: %s\n", __LINE__, #cond);               \
        }                                                                  \
    } while (0)

static bool says(const char *defect, const char *want) { return defect && want ? strcmp(defect, want) == 0 : defect == want; }

static const char *kNotNegative = "lr, beta1, beta2 and eps must be finite and not negative";
static const char *kNotNegativeDecay = "lr, beta1, beta2, eps and weight_decay must be finite and not negative";
static const char *kBelowOne = "beta1 and beta2 must be below 1";
static const char *kMaxNorm = "max_norm must be above 0 (+inf: no clipping)";

// the defect of (lr, beta1, beta2, eps, max_norm) with value `v` in place `at`, with and without a weight decay of 1e-4
static void one_defect(int at, float v, const char *want, const char *want_decay)
{
    float a[5] = {3e-4f, 0.9f, 0.999f, 1e-8f, 0.5f};
    a[at] = v;
    const float lr_eps[2] = {a[0], a[3]}, decay = 1e-4f;
    CHECK(says(adam_hyper_defect(lr_eps, 2, a[1], a[2], nullptr, a[4]), want));
    CHECK(says(adam_hyper_defect(lr_eps, 2, a[1], a[2], &decay, a[4]), want_decay));
}

static size_t tpolicy_floats(int ff, int layers) { return (size_t)kPlainLayer0 + (size_t)layers * (size_t)pl_layer(ff) + (size_t)kPlTail; }

int main()
{
    // decimal_of: the decimal the caller wrote, exactly the double that literal is
    CHECK(decimal_of(0.9f) == 0.9);
    CHECK(decimal_of(0.999f) == 0.999);
    CHECK(decimal_of(0.99f) == 0.99);
    CHECK(decimal_of(0.5f) == 0.5);
    CHECK(decimal_of(1e-8f) == 1e-8);
    CHECK(decimal_of(0.0f) == 0.0);
    const float third = 1.0f / 3.0f;                 // no short decimal: nine digits, within half an ulp of the float
    CHECK((float)decimal_of(third) == third);
    CHECK(fabs(decimal_of(third) - (double)third) <= 0.5 * (double)(nextafterf(third, 1.0f) - third));
    CHECK(decimal_of(third) != (double)third);
    const BetaScalars b = beta_scalars(0.9f, 0.999f);
    CHECK(b.beta1 == 0.9 && b.beta2 == 0.999);
    CHECK(b.update.one_minus_beta1 == (float)(1.0 - 0.9) && b.update.one_minus_beta2 == (float)0.001 && b.update.beta2 == 0.999f);
    CHECK(b.update.one_minus_beta2 != (float)(1.0 - (double)0.999f));      // what reading the float itself would give

    // the hyper-parameter check: one defect a call, the message of each
    const float nan = nanf(""), inf = INFINITY;
    one_defect(0, 3e-4f, nullptr, nullptr);
    one_defect(4, inf, nullptr, nullptr);            // no clipping
    one_defect(0, 0.0f, nullptr, nullptr);
    const float bad[4] = {nan, inf, -inf, -1e-3f};
    for (int at = 0; at < 4; ++at)
        for (float v : bad) one_defect(at, v, kNotNegative, kNotNegativeDecay);
    for (int at = 1; at <= 2; ++at)
        for (float v : {1.0f, 1.5f}) one_defect(at, v, kBelowOne, kBelowOne);
    for (float v : {nan, 0.0f, -0.5f, -inf}) one_defect(4, v, kMaxNorm, kMaxNorm);
    {
        const float lr_eps[4] = {3e-4f, 1e-3f, 1e-5f, 1e-8f}, four_bad[4] = {3e-4f, 1e-3f, 1e-5f, nan};
        CHECK(says(adam_hyper_defect(lr_eps, 4, 0.9f, 0.999f, nullptr, 0.5f), nullptr));
        CHECK(says(adam_hyper_defect(four_bad, 4, 0.9f, 0.999f, nullptr, 0.5f), kNotNegative));
        for (float v : bad) CHECK(says(adam_hyper_defect(lr_eps, 2, 0.9f, 0.999f, &v, 0.5f), kNotNegativeDecay));
        CHECK(says(adam_hyper_defect(four_bad, 4, 1.0f, 0.999f, nullptr, 0.0f), kNotNegative));      // reported in this order
        CHECK(says(adam_hyper_defect(lr_eps, 4, 1.0f, 0.999f, nullptr, 0.0f), kBelowOne));
    }

    // the chunks: a partial per 1,024 floats up to 1,024 partials, then per 2,048, ..
    CHECK(kStepMaxPartials == 1024 && kStepGroup == 1024);
    const struct { int ff, layers; size_t chunk, partials; } shapes[4] = {{32, 1, 1024, 158}, {96, 2, 1024, 194}, {2048, 2, 1024, 686},
                                                                          {4096, 2, 2048, 601}};
    for (const auto &s : shapes) {
        const size_t floats = tpolicy_floats(s.ff, s.layers);
        CHECK(step_chunk(floats) == s.chunk);
        CHECK(step_partials(floats) == s.partials);
        CHECK(step_partial_bytes(floats) == (s.partials * 8 + 15) / 16 * 16);
        CHECK((s.partials - 1) * s.chunk < floats && floats <= s.partials * s.chunk);
    }
    CHECK(tpolicy_floats(4096, 2) == 1230601);
    CHECK(step_chunk(1) == 1024 && step_partials(1) == 1 && step_partial_bytes(1) == 16);
    CHECK(step_partials(1024 * 1024) == 1024 && step_chunk(1024 * 1024) == 1024);
    CHECK(step_partials(1024 * 1024 + 1) == 513 && step_chunk(1024 * 1024 + 1) == 2048);
    for (size_t floats = 1; floats < (size_t)1 << 34; floats = floats * 3 + 1) {
        CHECK(step_partials(floats) <= kStepMaxPartials && step_chunk(floats) % kStepGroup == 0);
        CHECK(step_partials(floats) * step_chunk(floats) >= floats && (step_partials(floats) - 1) * step_chunk(floats) < floats);
    }

    // what both sides form: the clip coefficient (the reciprocal first) and the f64 bias corrections
    CHECK(clip_coefficient(0.1f, 0.3f) == 1.0f && clip_coefficient(0.0f, INFINITY) == 1.0f);
    CHECK(clip_coefficient(7.0f, 0.3f) == (1.0f / (7.0f + 1e-6f)) * 0.3f);
    const BiasCorrections bc = bias_corrections((double)3e-4f, 0.9, 0.999, 6.0);
    CHECK(bc.step_size == (float)((double)3e-4f / (1.0 - pow(0.9, 6.0))) && bc.bc2_sqrt == (float)sqrt(1.0 - pow(0.999, 6.0)));

    printf("step_common_host: %d checks, %d failed\n", checks, failed);
    return failed;
}
