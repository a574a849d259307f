"""The CPU yardstick of the expectimax agent (include/g2048_search.h): the definition restated in plain Python floats (IEEE f64,
one rounding per operation) over the oracle's env move, valid-move mask and full evaluation. It includes nothing of the device
code: csrc/g2048_expectimax.h is held to THIS, by tests/test_expectimax_host.py on the CPU and tests/test_gpu_expectimax.py on the
device, with == on every f64.

    leaf(B)  = full_eval(B, phase of B's max tile)
    V(B, 0)  = leaf(B)
    V(B, d)  = leaf(B) if no move is valid, else max over the valid actions a, ascending, of C(move(B, a), d)
    C(M, d)  = acc / e: acc = 0.0; for each empty cell c, row-major: acc += 0.9 * V(M + 2@c, d-1) + 0.1 * V(M + 4@c, d-1)

Boards here are tuples of 16 tile VALUES (0 = empty), the oracle's single-board form; decide() takes codes and returns codes' rows.
Values are memoised per call of decide(): the same board recurs under different move orders."""
import numpy as np

from oracle import oracle as O

NEG_INF = float("-inf")


class Search:
    def __init__(self, early_thr=512, mid_thr=1024):
        self.early, self.mid = int(early_thr), int(mid_thr)
        self.memo = {}

    def leaf(self, b):
        top = max(b)
        return O.full_eval(b, 0 if top < self.early else 1 if top < self.mid else 2)

    def value(self, b, d):
        if d == 0:
            return self.leaf(b)
        key = (b, d)
        if key not in self.memo:
            mask = O.env_valid_mask(b)
            if mask == 0:
                v = self.leaf(b)
            else:
                v = None
                for a in range(4):
                    if (mask >> a) & 1:
                        c = self.chance(tuple(int(x) for x in O.env_move(b, a)[0]), d)
                        if v is None or c > v:
                            v = c
            self.memo[key] = v
        return self.memo[key]

    def chance(self, m, d):
        cells = [c for c in range(16) if m[c] == 0]
        acc = 0.0
        for c in cells:
            two = 0.9 * self.value(m[:c] + (2,) + m[c + 1:], d - 1)
            four = 0.1 * self.value(m[:c] + (4,) + m[c + 1:], d - 1)
            acc += two + four
        return acc / float(len(cells))

    def decide(self, b, depth, mask=15):
        """(action, [C(move(b, a), depth) or -inf] * 4) for one board of tile values."""
        allowed = O.env_valid_mask(b) & int(mask) & 15
        values = [self.chance(tuple(int(x) for x in O.env_move(b, a)[0]), depth) if (allowed >> a) & 1 else NEG_INF for a in range(4)]
        action = 0
        for a in range(1, 4):
            if values[a] > values[action]:
                action = a
        return action, values


def decide(codes, depth, mask=None, early_thr=512, mid_thr=1024):
    """codes: uint8 (n, 16) log2 codes. Returns (actions uint8 (n,), values float64 (n, 4))."""
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1, 16)
    tiles = O.unpack(codes)
    actions = np.zeros(len(codes), np.uint8)
    values = np.zeros((len(codes), 4), np.float64)
    for i, row in enumerate(tiles):
        s = Search(early_thr, mid_thr)
        actions[i], values[i] = s.decide(tuple(int(x) for x in row), depth, 15 if mask is None else int(mask[i]))
    return actions, values


# ---- the boards the CPU and the GPU tests share ------------------------------------------------------------------------------------
def _checker():
    return [1 + ((c + (c >> 2)) & 1) for c in range(16)]


DEAD = _checker()                                                   # 2 and 4 alternating: no move
ONE_MOVE = _checker()[:12] + [0, 0, 0, 0]                           # three full rows without a pair over an empty one: DOWN alone
ONE_MERGE = _checker()[:14] + [3, 3]                                # full, one pair in the last row: LEFT and RIGHT, one empty cell after
CODE_15 = [15, 14, 13, 12, 5, 6, 7, 8, 3, 2, 1, 0, 0, 0, 1, 0]      # a 32768 tile
TIE = [1, 1, 1, 1, 4, 4, 4, 4, 4, 4, 4, 4, 1, 1, 1, 1]              # LEFT's and RIGHT's children are mirror images and tie to the bit
HAND = {"dead": DEAD, "one_move": ONE_MOVE, "tie": TIE, "one_merge": ONE_MERGE, "code_15": CODE_15}
RAGGED = 257                                                        # the GPU test's n = 1, 63, 64, 65, 257 are prefixes of these
_CACHE = {}


def _crowded(count, most_empty, seed):
    """The first `count` synthetic boards with 1 .. most_empty empty cells."""
    b = O.synth_boards(4096, seed=seed, p_empty=0.15)
    empty = (b == 0).sum(axis=1)
    return b[(empty >= 1) & (empty <= most_empty)][:count]


def boards_for(depth):
    """What the issue sets per depth, then the hand-made boards: 64 synthetic boards at depth 1, 16 with at most 6 empty cells at
    depth 2, 4 with at most 3 at depth 3."""
    first = {1: lambda: O.synth_boards(64, seed=0xE1), 2: lambda: _crowded(16, 6, 0xE2), 3: lambda: _crowded(4, 3, 0xE3)}[depth]()
    assert len(first) == {1: 64, 2: 16, 3: 4}[depth]
    return np.concatenate([first, np.array(list(HAND.values()), np.uint8)])


def reference(depth, which="cases"):
    """(boards, actions, values) of boards_for(depth), or with which="ragged" of RAGGED synthetic boards (depth 1 only): computed
    once per process and shared by every test that asks; the arrays are read-only."""
    key = (depth, which)
    if key not in _CACHE:
        boards = boards_for(depth) if which == "cases" else O.synth_boards(RAGGED, seed=0xE4)
        out = (boards,) + decide(boards, depth)
        for a in out:
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]
