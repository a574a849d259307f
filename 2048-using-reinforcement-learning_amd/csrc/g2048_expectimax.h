// g2048_expectimax.h -- the expectimax value function of g2048_expectimax.hip (include/g2048_search.h), per board and per
// root successor: everything a lane computes, and the fixed-order sum one lane takes afterwards. G2048_HD like g2048_board.h,
// so the tests compile this exact arithmetic for the host and hold it to a plain restatement of the definition.
//
// The function (f64, -ffp-contract=off; env moves, actions 0..3 as the env numbers them -- no rot180-DOWN quirk):
//   leaf(B)  = eval_full(B, phase_of(max code of B))                                    (the beam agent's _evaluate_state)
//   V(B, 0)  = leaf(B)
//   V(B, d)  = leaf(B) if no move is valid, else max over the valid actions a, ascending, of C(move(B, a), d)
//   C(M, d)  = (sum over the empty cells c of M, row-major, of 0.9 V(M + 2@c, d-1) + 0.1 V(M + 4@c, d-1)) / (double)#cells
// with the two products formed first, then added, then added to the running sum, which starts at 0.0.
//
// No recursion: ex_value<D> is a template, so depth D is D pairs of nested loops in one function body (action, then the
// 2 x #cells successors of the moved board), all state in registers; there is no call stack and no array indexed at run time.
// The two tiles of a cell are one loop of 2 x #cells trips, not two copies of the body: trip k places tile (k & 1) at empty cell
// k >> 1, the even trip parks its product, the odd one adds the pair to the sum.
//
// The root is cut differently, so that a wavefront can share it: ex_root() makes the four moves and numbers the
// (action, cell, tile) successors of the valid ones 0 .. items-1 (at most 4 x 15 x 2 = 120) without gaps; ex_root_term<D>(i) is
// successor i's product 0.9 / 0.1 x V(., D-1), which any lane may compute; ex_root_chance(a, terms) is C for action a from the
// terms in cell order, and ex_pick() the decision. The tests' host build runs the same four steps in a plain loop.
#pragma once
#include "g2048_board.h"

namespace g2048 {

constexpr int kExMaxDepth = 3;
constexpr uint32_t kExMaxItems = 128;            // >= 4 actions x 15 empty cells x 2 tiles

struct ExThr { uint32_t early, mid; };           // BeamSearchAgent's early_game_threshold / mid_game_threshold, tile values

G2048_HD double ex_leaf(const Board &b, ExThr t)
{
    const uint32_t mc = max_code(b);
    return eval_full_known(b, phase_of(mc, t.early, t.mid), count_empty(b), mc);
}

// 0x80 in the byte of the empty cell of row-major rank `rank` (0-based) of m, 0 elsewhere (rank >= #empty: all 0): ranks by a
// byte-wise prefix sum of the zero indicators, as simulate_sampled_successor takes them
G2048_HD void ex_cell_flag(const Board &m, uint32_t rank, uint32_t hit[4])
{
    const uint32_t ones = 0x01010101u;
    uint32_t z[4], p[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { z[r] = zflag(m.w[r]); p[r] = (z[r] >> 7) * ones; }
    const uint32_t o1 = p[0] >> 24, o2 = o1 + (p[1] >> 24), o3 = o2 + (p[2] >> 24);
    const uint32_t want = (rank + 1u) * ones;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t rk = p[r] + (r == 0 ? 0u : r == 1 ? o1 : r == 2 ? o2 : o3) * ones;      // 1-based rank of every empty cell, <= 16
        hit[r] = zflag(rk ^ want) & z[r];
    }
}

// successor k of the moved board m: tile 2 (k even) or 4 (k odd) at empty cell k >> 1
G2048_HD Board ex_successor(const Board &m, uint32_t k)
{
    uint32_t hit[4];
    ex_cell_flag(m, k >> 1, hit);
    const uint32_t sh = (k & 1u) ? 6u : 7u;          // 0x80 >> 7 = code 1 (tile 2), >> 6 = code 2 (tile 4)
    return Board{{m.w[0] | (hit[0] >> sh), m.w[1] | (hit[1] >> sh), m.w[2] | (hit[2] >> sh), m.w[3] | (hit[3] >> sh)}};
}

template <int D>
G2048_HD double ex_value(const Board &b, ExThr t);

// C(m, D), D >= 1; m has at least one empty cell (a valid move leaves one)
template <int D>
G2048_HD double ex_chance(const Board &m, ExThr t)
{
    const uint32_t e = count_empty(m);
    double acc = 0.0, p2 = 0.0;
#pragma unroll 1
    for (uint32_t k = 0; k < 2u * e; ++k) {
        const double v = ex_value<D - 1>(ex_successor(m, k), t);
        if (k & 1u) {
            const double p4 = 0.1 * v;
            acc += p2 + p4;
        } else {
            p2 = 0.9 * v;
        }
    }
    return acc / (double)e;
}

template <int D>
G2048_HD double ex_value(const Board &b, ExThr t)
{
    if constexpr (D == 0) {
        return ex_leaf(b, t);
    } else {
        const uint32_t mask = valid_mask_env(b);
        if (mask == 0u) return ex_leaf(b, t);
        double best = -__builtin_inf();
#pragma unroll 1
        for (uint32_t a = 0; a < 4u; ++a) {
            if (!((mask >> a) & 1u)) continue;
            uint32_t gain;
            const double c = ex_chance<D>(move_env(b, a, gain), t);
            if (c > best) best = c;
        }
        return best;
    }
}

// ---------------------------------------------------------------------------------------------------------------- root --
// (plain members, no arrays: the struct lives in registers across the successor loop)
struct ExRoot {
    Board m0, m1, m2, m3;              // move(b, a)
    uint32_t e0, e1, e2, e3;           // empty cells of the moved board; 0 for an action that is invalid or masked out
    uint32_t f1, f2, f3;               // the number of action a's first successor (action 0's is 0)
    uint32_t items;                    // successors in all, <= 120
    uint32_t mask;                     // the env's valid moves AND the caller's mask
};

G2048_HD uint32_t ex_sel(uint32_t a, uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3)
{
    return a == 0u ? x0 : a == 1u ? x1 : a == 2u ? x2 : x3;
}

G2048_HD ExRoot ex_root(const Board &b, uint32_t caller_mask)
{
    ExRoot r;
    r.mask = valid_mask_env(b) & caller_mask & 15u;
    uint32_t gain;
    r.m0 = move_env(b, 0u, gain);
    r.m1 = move_env(b, 1u, gain);
    r.m2 = move_env(b, 2u, gain);
    r.m3 = move_env(b, 3u, gain);
    r.e0 = (r.mask & 1u) ? count_empty(r.m0) : 0u;
    r.e1 = (r.mask & 2u) ? count_empty(r.m1) : 0u;
    r.e2 = (r.mask & 4u) ? count_empty(r.m2) : 0u;
    r.e3 = (r.mask & 8u) ? count_empty(r.m3) : 0u;
    r.f1 = 2u * r.e0;
    r.f2 = r.f1 + 2u * r.e1;
    r.f3 = r.f2 + 2u * r.e2;
    r.items = r.f3 + 2u * r.e3;
    return r;
}

// successor i < r.items: its action's moved board by selects (nothing is indexed at run time), then its product
template <int D>
G2048_HD double ex_root_term(const ExRoot &r, uint32_t i, ExThr t)
{
    // an action without successors shares its first number with the next one, so counting the firsts that are <= i skips it
    const uint32_t a = (i >= r.f1 ? 1u : 0u) + (i >= r.f2 ? 1u : 0u) + (i >= r.f3 ? 1u : 0u);
    const uint32_t k = i - ex_sel(a, 0u, r.f1, r.f2, r.f3);
    const Board m = {{ex_sel(a, r.m0.w[0], r.m1.w[0], r.m2.w[0], r.m3.w[0]), ex_sel(a, r.m0.w[1], r.m1.w[1], r.m2.w[1], r.m3.w[1]),
                      ex_sel(a, r.m0.w[2], r.m1.w[2], r.m2.w[2], r.m3.w[2]), ex_sel(a, r.m0.w[3], r.m1.w[3], r.m2.w[3], r.m3.w[3])}};
    const double v = ex_value<D - 1>(ex_successor(m, k), t);
    return (k & 1u) ? 0.1 * v : 0.9 * v;
}

// C(move(b, a), D) from the terms, in cell order; -inf for an action that is invalid or masked out
G2048_HD double ex_root_chance(const ExRoot &r, uint32_t a, const double *terms)
{
    const uint32_t e = ex_sel(a, r.e0, r.e1, r.e2, r.e3), f = ex_sel(a, 0u, r.f1, r.f2, r.f3);
    if (e == 0u) return -__builtin_inf();
    double acc = 0.0;
    for (uint32_t c = 0; c < e; ++c) acc += terms[f + 2u * c] + terms[f + 2u * c + 1u];
    return acc / (double)e;
}

// the largest of the four, ties to the lowest action; all -inf (no move left): 0
G2048_HD uint32_t ex_pick(double c0, double c1, double c2, double c3)
{
    uint32_t a = 0u;
    double best = c0;
    if (c1 > best) { best = c1; a = 1u; }
    if (c2 > best) { best = c2; a = 2u; }
    if (c3 > best) { best = c3; a = 3u; }
    return a;
}

}  // namespace g2048
