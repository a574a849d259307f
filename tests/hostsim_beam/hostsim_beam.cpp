// hostsim_beam.cpp -- TEST HARNESS ONLY (lives under tests/, never shipped, never loaded by the product).
//
// Compiles csrc/g2048_lookahead.h -- the hybrid agent's planned decision and the mapping from draws to candidate boards, exactly
// as the kernels of g2048_qnet.hip run them -- for the host CPU, with the portable stand-ins of tests/hostsim for the two gfx950
// builtins, so the `-m "not gpu"` suite can hold them against the reference's recorded decisions without a GPU.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../hostsim/hostsim_intrinsics.h"
#include "g2048_lookahead.h"
#include "g2048_rng.h"

using namespace g2048;

static Board ld(const uint8_t *p) { Board b; memcpy(b.w, p, 16); return b; }

extern "C" {

void hb_planned(const uint8_t *boards, uint32_t threshold, uint8_t *planned, size_t n)
{
    for (size_t i = 0; i < n; ++i) planned[i] = lookahead_planned(ld(boards + 16 * i), threshold) ? 1 : 0;
}

// the planned action of every board (whether or not the search would plan it); leaf_q: null, or float32 (n, 32, 4)
void hb_actions(const uint8_t *boards, uint32_t width, double gamma, const float *leaf_q, uint8_t *actions, size_t n)
{
    for (size_t i = 0; i < n; ++i) {
        LookaheadLocal s;
        actions[i] = (uint8_t)lookahead_action(ld(boards + 16 * i), width, gamma, leaf_q ? leaf_q + i * kLookaheadSlots * 4 : nullptr, s);
    }
}

// the candidate boards of every board from its draws h (n, 4, 3): succ (n, 32, 16), count (n, 4)
void hb_expand(const uint8_t *boards, const uint32_t *h, uint8_t *succ, uint8_t *count, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        for (uint32_t a = 0; a < 4; ++a)
            for (uint32_t j = 0; j < 8; ++j) {
                const uint32_t *ha = h + (i * 4 + a) * 3;
                uint32_t c;
                const Board o = lookahead_slot(ld(boards + 16 * i), a, j, ha[0], ha[1], ha[2], c);
                memcpy(succ + ((i * kLookaheadSlots) + 8 * a + j) * 16, o.w, 16);
                count[i * 4 + a] = (uint8_t)c;
            }
}

// draw `ctr` of (seed, SIMULATE, step_index, id): what g2048_qnet_beam_expand feeds lookahead_slot (ctr = 3 a + pick)
uint32_t hb_draw(uint64_t seed, uint64_t step_index, uint64_t id, uint32_t ctr)
{
    const Keys k = rng_keys(seed, DOM_SIMULATE, step_index);
    return rng_draw(k.k0, k.k1, id, ctr);
}

}  // extern "C"
