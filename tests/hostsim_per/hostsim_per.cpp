// hostsim_per.cpp -- TEST HARNESS ONLY (lives under tests/, never shipped, never loaded by the product).
//
// Compiles csrc/g2048_per.h -- train_step's reward shaping, the priority rule and the ring's index arithmetic, exactly as the
// kernels of g2048_per.hip run them -- for the host CPU, with the portable stand-ins of tests/hostsim for the two gfx950
// builtins, so the `-m "not gpu"` suite can hold them against what the reference returned without a GPU.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../hostsim/hostsim_intrinsics.h"
#include "g2048_per.h"

using namespace g2048;

static Board ld(const uint8_t *p) { Board b; memcpy(b.w, p, 16); return b; }

extern "C" {

void hp_shape(const uint8_t *states, const uint8_t *next_states, const float *rewards, float *shaped, size_t n)
{
    for (size_t i = 0; i < n; ++i) shaped[i] = dqn_shaped_reward(ld(states + 16 * i), ld(next_states + 16 * i), rewards[i]);
}

void hp_priority(const float *td_errors, float *priorities, size_t n)
{
    for (size_t i = 0; i < n; ++i) priorities[i] = per_priority(td_errors[i]);
}

void hp_tile_values(const uint8_t *codes, float *values, size_t n)
{
    for (size_t i = 0; i < n; ++i) values[i] = per_tile_value(codes[i]);
}

size_t hp_slot(size_t head, size_t i, size_t capacity) { return per_slot(head, i, capacity); }

}  // extern "C"
