// hostsim_expectimax.cpp -- TEST HARNESS ONLY (lives under tests/, never shipped, never loaded by the product).
//
// Compiles csrc/g2048_expectimax.h -- the expectimax value function exactly as the kernels of g2048_expectimax.hip run it -- for
// the host CPU, with the portable stand-ins of tests/hostsim for the two gfx950 builtins, so the `-m "not gpu"` suite can hold
// it to tests/expectimax_ref.py without a GPU. hx_decide takes the four steps of the device's decide_wave in a plain loop:
// the root, every successor's term under its number (an array stands in for LDS), the four fixed-order sums, the pick.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../hostsim/hostsim_intrinsics.h"
#include "g2048_expectimax.h"

using namespace g2048;

template <int D>
static uint32_t decide(const Board &b, uint32_t mask, ExThr t, double values[4])
{
    const ExRoot r = ex_root(b, mask);
    double terms[kExMaxItems];
    // lane l of the wavefront takes l, l + 64: the same numbers in another order
    for (uint32_t lane = 0; lane < 64u; ++lane)
        for (uint32_t i = lane; i < r.items; i += 64u) terms[i] = ex_root_term<D>(r, i, t);
    for (uint32_t a = 0; a < 4u; ++a) values[a] = ex_root_chance(r, a, terms);
    return ex_pick(values[0], values[1], values[2], values[3]);
}

extern "C" {

// boards: n x 16 codes; mask_or_null: n bytes; actions: n bytes; values: n x 4 doubles. Returns 0, or -1 for a depth outside 1..3.
int hx_decide(const uint8_t *boards, const uint8_t *mask_or_null, int depth, uint32_t early_thr, uint32_t mid_thr, size_t n,
              uint8_t *actions, double *values)
{
    if (depth < 1 || depth > kExMaxDepth) return -1;
    const ExThr t{early_thr, mid_thr};
    for (size_t i = 0; i < n; ++i) {
        Board b;
        memcpy(b.w, boards + 16 * i, 16);
        const uint32_t mask = mask_or_null ? mask_or_null[i] : 15u;
        double *v = values + 4 * i;
        actions[i] = (uint8_t)(depth == 1 ? decide<1>(b, mask, t, v) : depth == 2 ? decide<2>(b, mask, t, v) : decide<3>(b, mask, t, v));
    }
    return 0;
}

// V(board, depth) for depth 0..2, the value a lane computes for its successor
double hx_value(const uint8_t *board, int depth, uint32_t early_thr, uint32_t mid_thr)
{
    Board b;
    memcpy(b.w, board, 16);
    const ExThr t{early_thr, mid_thr};
    return depth == 0 ? ex_value<0>(b, t) : depth == 1 ? ex_value<1>(b, t) : ex_value<2>(b, t);
}

}  // extern "C"
