// san_main.cpp -- TEST HARNESS ONLY: a stand-alone program that runs the host build of csrc/g2048_expectimax.h (hostsim_expectimax.cpp)
// under ASan + UBSan over hand-made and pseudo-random boards at depths 1..3, and checks what needs no yardstick: the action is
// the first largest of the four values, an invalid action's value is -inf, a dead board gives action 0, and the values of depth
// d + 1 are built from V(., d) (hx_value). Prints "expectimax san ok" and a checksum; any finding of a sanitizer ends it non-zero.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

extern "C" int hx_decide(const uint8_t *boards, const uint8_t *mask_or_null, int depth, uint32_t early_thr, uint32_t mid_thr, size_t n,
                         uint8_t *actions, double *values);
extern "C" double hx_value(const uint8_t *board, int depth, uint32_t early_thr, uint32_t mid_thr);

static uint32_t rnd(uint32_t &s) { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; }

int main()
{
    enum { N = 40 };
    static uint8_t boards[N][16];
    uint32_t s = 0x2048u;
    // 0: dead (a checkerboard of 2 and 4); 1: empty; 2: one tile; 3: a full board with one merge; 4: code 15 and 16 present
    for (int c = 0; c < 16; ++c) boards[0][c] = (uint8_t)(1 + ((c + (c >> 2)) & 1));
    boards[2][5] = 1;
    for (int c = 0; c < 16; ++c) boards[3][c] = (uint8_t)(1 + ((c + (c >> 2)) & 1));
    boards[3][15] = boards[3][14];
    for (int c = 0; c < 16; ++c) boards[4][c] = (uint8_t)(c < 12 ? 0 : 13 + (c & 3));
    for (int i = 5; i < N; ++i)
        for (int c = 0; c < 16; ++c) boards[i][c] = (uint8_t)((rnd(s) % 100u) < (i < 20 ? 20u : 70u) ? 0u : 1u + rnd(s) % 11u);
    double sum = 0.0;
    int bad = 0;
    for (int depth = 1; depth <= 3; ++depth) {
        const int n = depth == 3 ? 12 : N;           // (the first twelve: the hand-made ones and seven crowded boards)
        uint8_t actions[N], masks[N];
        double values[N][4];
        for (int i = 0; i < n; ++i) masks[i] = (uint8_t)(i % 3 == 2 ? rnd(s) & 15u : 15u);
        if (hx_decide(&boards[0][0], masks, depth, 512u, 1024u, (size_t)n, actions, &values[0][0]) != 0) return 2;
        for (int i = 0; i < n; ++i) {
            int first = 0;
            for (int a = 1; a < 4; ++a) if (values[i][a] > values[i][first]) first = a;
            bad += actions[i] != first;
            for (int a = 0; a < 4; ++a) {
                bad += !((masks[i] >> a) & 1) && !(isinf(values[i][a]) && values[i][a] < 0);
                bad += isnan(values[i][a]);
                if (isfinite(values[i][a])) sum += values[i][a];
            }
        }
        bad += actions[0] != 0 || isfinite(values[0][0]) || isfinite(values[0][3]);
        sum += hx_value(boards[depth], depth - 1, 512u, 1024u);
    }
    bad += hx_decide(&boards[0][0], nullptr, 0, 512u, 1024u, 1, nullptr, nullptr) != -1;
    bad += hx_decide(&boards[0][0], nullptr, 4, 512u, 1024u, 1, nullptr, nullptr) != -1;
    printf("expectimax san %s: mismatches %d, checksum %.17g\n", bad ? "FAILED" : "ok", bad, sum);
    return bad ? 1 : 0;
}
