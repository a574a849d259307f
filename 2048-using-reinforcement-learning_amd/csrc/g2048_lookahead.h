// g2048_lookahead.h -- the hybrid agent's beam_search (agents/hybrid.py:814-907) as the reference actually runs it, one
// decision per board. Uses only g2048_board.h; compiled for the device by g2048_qnet.hip and for the host by the tests'
// harness. Everything is f64 in the reference's operation order: compile with -ffp-contract=off.
//
// What the reference's search is. Its loop ends after the first level at every search_depth: the early-exit test (:871) reads
// the fourth field of a beam entry as `done`, but that field is the probability 1 / len(transitions) > 0, so all(...) holds
// and the loop breaks after step 0. What is left is one ranking of the root's children:
//   planned    the search decides when the max tile is >= the threshold (:939) and at least 8 cells are filled (:821);
//              otherwise the action is the exploit action on the board's own Q.
//   candidates in the order a = 0, 1, 2, 3 (LEFT, UP, RIGHT, DOWN, all four directions true). M = move(B, a). M == B: one
//              candidate, reward -1.0, p = 1.0 (:606-607). Else with e = empty cells of M and k = min(3, e): 2k candidates, pick 0
//              with a 2, pick 0 with a 4, pick 1 with a 2, ...; reward = simulate_sampled_successor's (weighted 0.9 / 0.1: it
//              depends on M and the tile's value, not on the cell), p = 1.0 / (2k). (A changed board always has an empty cell,
//              so the `done` transition of :611-613 cannot occur.)
//   totals     search_depth >= 2: total = 0.0 + reward; step 0 is not the last step, so no network is consulted and the draws
//              do not matter. search_depth == 1: total = (0.0 + reward) + gamma * (double)v, v = the f32 maximum of the four
//              Q-values of the candidate's board (for an invalid move the board itself, :852-855).
//   beam       key = total * p; the first `width` candidates in descending key order, equal keys in candidate order (Python's
//              stable sort(reverse=True), :867-868).
//   action     the beam is walked in order and every action sums the keys of its members in that order (the first assigns, later
//              ones add, :883-890); the largest sum wins, equal sums go to the action whose first member stands earliest in the
//              beam (max over a dict in insertion order, :894).
// Finite leaf values are assumed. The slots of a board's candidates are numbered 8 a + j (j < 6): the layout of the candidate
// boards g2048_qnet_beam_expand writes and of the leaf Q-values g2048_qnet_beam_actions reads.
#pragma once
#include "g2048_board.h"

namespace g2048 {

constexpr uint32_t kLookaheadSlots = 32;             // 8 a + j
constexpr uint32_t kLookaheadCandidates = 24;        // at most 4 x 2 x 3

// The scratch of one decision: S gives `double &key(uint32_t i)` and `uint32_t &rank(uint32_t i)` for i < kLookaheadCandidates.
// The kernels keep it in LDS (a column per lane: every index below is uniform over the lanes that run it), the host in a struct.
struct LookaheadLocal {
    double k[kLookaheadCandidates];
    uint32_t r[kLookaheadCandidates];
    G2048_HD double &key(uint32_t i) { return k[i]; }
    G2048_HD uint32_t &rank(uint32_t i) { return r[i]; }
};

G2048_HD bool lookahead_planned(const Board &b, uint32_t threshold)
{
    const uint32_t mc = max_code(b);
    const bool reached = mc >= 32u || (mc ? (1u << mc) : 0u) >= threshold;
    return reached && count_empty(b) <= 8u;
}

// candidates of (b, a): 1 for a move that changes nothing, else 2 * min(3, empty cells of the moved board)
G2048_HD uint32_t lookahead_count(const Board &b, const Board &moved)
{
    if (same(moved, b)) return 1u;
    const uint32_t e = count_empty(moved);
    return 2u * (e < 3u ? e : 3u);
}

// Slot 8 a + j of board b's candidates, with the three draws of action a (pick i is simulate_sampled_successor's mapping of
// h_i): the board itself in slot 8 a for an invalid move, the empty board in an unused slot. count = lookahead_count.
G2048_HD Board lookahead_slot(const Board &b, uint32_t a, uint32_t j, uint32_t h0, uint32_t h1, uint32_t h2, uint32_t &count)
{
    uint32_t gain;
    const Board moved = move_env(b, a, gain);
    count = lookahead_count(b, moved);
    if (j >= count) return Board{{0u, 0u, 0u, 0u}};
    if (count == 1u) return moved;
    return simulate_sampled_successor(b, moved, j, count_empty(moved), h0, h1, h2).board;
}

G2048_HD float lookahead_leaf(const float *q4)
{
    float v = q4[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) v = q4[k] > v ? q4[k] : v;
    return v;
}

// The planned action of board b. leaf_q: null for search_depth >= 2; for search_depth == 1 the board's 32 x 4 Q-values, slot
// 8 a + j as g2048_qnet_forward gives them for lookahead_slot's boards.
template <class S>
G2048_HD uint32_t lookahead_action(const Board &b, uint32_t width, double gamma, const float *leaf_q, S &s)
{
    uint32_t n = 0u, s1 = 0u, s2 = 0u, s3 = 0u;      // candidates so far; where the actions 1, 2, 3 start
#pragma unroll 1
    for (uint32_t a = 0u; a < 4u; ++a) {
        s1 = a == 1u ? n : s1;
        s2 = a == 2u ? n : s2;
        s3 = a == 3u ? n : s3;
        uint32_t gain;
        const Board moved = move_env(b, a, gain);
        const uint32_t count = lookahead_count(b, moved);
        if (count == 1u) {
            double total = 0.0 + -1.0;
            if (leaf_q) total = total + gamma * (double)lookahead_leaf(leaf_q + 4u * (8u * a));
            s.key(n) = total * 1.0;
        } else {
            const uint32_t e = count_empty(moved);
            const double r2 = simulate_sampled_successor(b, moved, 0u, e, 0u, 0u, 0u).reward;
            const double r4 = simulate_sampled_successor(b, moved, 1u, e, 0u, 0u, 0u).reward;
            const double p = count == 2u ? 0.5 : count == 4u ? 0.25 : 1.0 / 6.0;
#pragma unroll 1
            for (uint32_t j = 0u; j < count; ++j) {
                double total = 0.0 + ((j & 1u) ? r4 : r2);
                if (leaf_q) total = total + gamma * (double)lookahead_leaf(leaf_q + 4u * (8u * a + j));
                s.key(n + j) = total * p;
            }
        }
        n += count;
    }
    // a candidate's place in the stable descending order, by counting
#pragma unroll 1
    for (uint32_t i = 0u; i < n; ++i) {
        const double ki = s.key(i);
        uint32_t r = 0u;
#pragma unroll 1
        for (uint32_t j = 0u; j < n; ++j) {
            const double kj = s.key(j);
            r += (kj > ki || (kj == ki && j < i)) ? 1u : 0u;
        }
        s.rank(i) = r;
    }
    // the beam in order: per action the sum of its members' keys and the place of its first member
    const uint32_t beam = width < n ? width : n;
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    uint32_t first[4] = {~0u, ~0u, ~0u, ~0u};
#pragma unroll 1
    for (uint32_t r = 0u; r < beam; ++r) {
#pragma unroll 1
        for (uint32_t i = 0u; i < n; ++i) {
            if (s.rank(i) != r) continue;
            const double k = s.key(i);
            const uint32_t a = (i >= s1 ? 1u : 0u) + (i >= s2 ? 1u : 0u) + (i >= s3 ? 1u : 0u);
#pragma unroll
            for (uint32_t c = 0u; c < 4u; ++c) {
                if (a != c) continue;
                sum[c] = first[c] == ~0u ? k : sum[c] + k;
                first[c] = first[c] == ~0u ? r : first[c];
            }
        }
    }
    uint32_t best = 4u;
    double best_sum = 0.0;
    uint32_t best_first = ~0u;
#pragma unroll
    for (uint32_t c = 0u; c < 4u; ++c) {
        if (first[c] == ~0u) continue;
        if (best == 4u || sum[c] > best_sum || (sum[c] == best_sum && first[c] < best_first)) {
            best = c; best_sum = sum[c]; best_first = first[c];
        }
    }
    return best;
}

}  // namespace g2048
