// g2048_per.h -- the per-transition arithmetic of the hybrid agent's prioritized experience replay ("per"): the reward shaping
// of DQNAgent.train_step (agents/hybrid.py:971-1034) and the priority rule of its update (:1063-1064, :759-762). Uses only
// g2048_board.h; compiled for the device by g2048_per.hip and for the host by the tests' harness. The shaping mixes f32 and
// f64 exactly as the reference's NumPy scalars do: compile with -ffp-contract=off.
//
// The buffer. A ring of `capacity` slots in caller-owned arrays; the host tracks size (live entries) and head (physical slot of
// the oldest entry). Logical index i (0 = oldest, the reference's deque index) lives at physical slot (head + i) % capacity.
//
// push (:736-740). m transitions pushed in order all get the priority M = the maximum of the `size` live priorities before the
// call (1.0 for an empty buffer). That is exactly what m sequential calls of the reference's push give, not an approximation:
// the first of them appends M itself, so from then on the buffer holds an entry of priority M that is younger than everything
// an eviction can remove during the batch, no entry exceeds M, and every later max() is M again.
#pragma once
#include "g2048_board.h"

namespace g2048 {

// physical slot of logical index i (i < size <= capacity, head < capacity)
G2048_HD size_t per_slot(size_t head, size_t i, size_t capacity)
{
    const size_t p = head + i;
    return p >= capacity ? p - capacity : p;
}

// the float32 state value of a cell: the tile 2^code, 0 for an empty cell
G2048_HD float per_tile_value(uint32_t code) { return code ? (float)(1u << code) : 0.0f; }

// update_priorities(indices, td_errors + 1e-5) (:1063-1064, :759-762): the sum is float32 (a float32 tensor plus a Python
// scalar), and Python's max(priority, 1e-5) keeps its first argument unless the second is larger
G2048_HD float per_priority(float td_error)
{
    const float v = td_error + 1e-5f;
    return 1e-5f > v ? 1e-5f : v;
}

// sum of the tile values of every cell that equals its right or lower neighbour (:1012-1023); below 2^24, so the
// reference's float32 running sum holds the same integer
G2048_HD uint32_t per_merge_sum(const Board &b)
{
    uint32_t sum = 0u;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t x = b.w[r];
        const uint32_t h = eqnzflag(x, x >> 8);                      // lane c: cell (r, c) == cell (r, c + 1) != 0 (lane 3 never)
        const uint32_t v = r < 3 ? eqnzflag(x, b.w[(r + 1) & 3]) : 0u;   // lane c: cell (r, c) == cell (r + 1, c) != 0
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t tile = 1u << ((x >> (8 * c)) & 0xffu);
            if (h & (0x80u << (8 * c))) sum += tile;
            if (v & (0x80u << (8 * c))) sum += tile;
        }
    }
    return sum;
}

// One iteration of train_step's shaping loop (:974-1032) and its rounding to float32 (:1034). The dtypes are the reference's,
// under NumPy 2's promotion rules (Python scalars are weak):
//   :980        base * 0.1                        Python floats: f64
//   :983-985    + np.log2(max_tile) * 2.0          a float32 scalar times a Python float is float32, and a Python float plus a
//                                                  float32 scalar is float32: the sum is ROUNDED TO f32 and added in f32
//   :988-998    + (snake_score / 500) * 10.0       float32 x int64 is float64: f64 from here on (the score is a small integer)
//   :1001-1005  + np.log2(max_tile) * 5.0 / 2.0    float32 (exact), widened; needs max_tile > 64; (3,3) first, else (0,0)
//   :1008-1009  + empty_count * 0.5                int64 x Python float: f64
//   :1012-1025  + merge_bonus * 0.01               a float32 sum times a Python float: an f32 PRODUCT with 0.01f, widened
//   :1028-1029  + max_tile * 0.5                   float32 (exact), widened; needs a new maximum
// np.log2 of a float32 power of two is the exact integer for codes 1 .. 17, so everything works from the codes. An empty
// next board (max_tile == 0) skips the f32 step, as the reference does.
G2048_HD float dqn_shaped_reward(const Board &prev, const Board &next, float reward)
{
    const uint32_t mc = max_code(next);
    double s = (double)reward * 0.1;
    if (mc != 0u) s = (double)((float)s + (float)mc * 2.0f);
    // 16 - snake_pattern (:801-806), row by row, cell (r, c) in byte c
    uint32_t snake = dot4(next.w[0], 0x04030201u, 0u);
    snake = dot4(next.w[1], 0x05060708u, snake);
    snake = dot4(next.w[2], 0x0c0b0a09u, snake);
    snake = dot4(next.w[3], 0x0d0e0f10u, snake);
    s += ((double)snake / 500.0) * 10.0;
    if (mc > 6u) {
        if ((next.w[3] >> 24) == mc) s += (double)((float)mc * 5.0f);
        else if ((next.w[0] & 0xffu) == mc) s += (double)((float)mc * 2.0f);
    }
    s += (double)count_empty(next) * 0.5;
    s += (double)((float)per_merge_sum(next) * 0.01f);
    if (mc > max_code(prev)) s += (double)((float)(1u << mc) * 0.5f);
    return (float)s;
}

}  // namespace g2048
