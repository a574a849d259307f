"""The hybrid agent's beam_search (agents/hybrid.py:814-907) restated in plain Python / NumPy, in the project's own words: the
yardstick of csrc/g2048_lookahead.h and of the kernels that use it. Boards are 16 uint8 log2 codes, row-major.

The reference's loop leaves after its first level (its early-exit test at :871 reads a beam entry's probability as `done`), so a
decision is one ranking of the root's children:

  planned(B)   max tile >= threshold and at least 8 filled cells; otherwise the exploit action on the board's own Q decides.
  candidates   for a = 0, 1, 2, 3 (LEFT, UP, RIGHT, DOWN): M = move(B, a). M == B: one candidate, reward -1.0, p = 1.0. Else, with
               e empty cells in M and k = min(3, e): 2k candidates -- pick 0 with a 2, pick 0 with a 4, pick 1 with a 2, ... -- of
               reward ((tile + bonus) + (e - 1) * 0.1) * (0.9 for a 2, 0.1 for a 4), bonus = the new max tile if it rose, and
               p = 1.0 / (2k). The reward does not depend on the picked cell.
  total        search_depth >= 2: 0.0 + reward. search_depth == 1: (0.0 + reward) + gamma * float(v), v = the float32 maximum of
               the candidate board's four Q-values (slot 8 a + j of `leaf`).
  beam         key = total * p; the first `width` candidates by descending key, equal keys in candidate order.
  action       per action the keys of its beam members summed in beam order; the largest sum, ties to the action whose first
               member stands earliest in the beam.
"""
import numpy as np

SLOTS = 32          # slot 8 a + j


def slide_left(row):
    """One row of codes slid and merged to the left (each tile merges at most once)."""
    tiles = [int(c) for c in row if c]
    out, i = [], 0
    while i < len(tiles):
        if i + 1 < len(tiles) and tiles[i] == tiles[i + 1]:
            out.append(tiles[i] + 1)
            i += 2
        else:
            out.append(tiles[i])
            i += 1
    return out + [0] * (4 - len(out))


def move(board, action):
    """The board after action 0 LEFT, 1 UP, 2 RIGHT, 3 DOWN (no spawn)."""
    g = np.asarray(board, dtype=np.int64).reshape(4, 4)
    if action in (1, 3):
        g = g.T
    if action in (2, 3):
        g = g[:, ::-1]
    g = np.array([slide_left(r) for r in g], dtype=np.int64)
    if action in (2, 3):
        g = g[:, ::-1]
    if action in (1, 3):
        g = g.T
    return g.reshape(16)


def tile(code):
    return (1 << int(code)) if code else 0


def planned(board, threshold=64):
    b = np.asarray(board)
    return tile(b.max()) >= threshold and int((b > 0).sum()) >= 8


def counts(board):
    """Candidates per action: 1 for a move that changes nothing, else 2 * min(3, empty cells of the moved board)."""
    b = np.asarray(board, dtype=np.int64)
    out = []
    for a in range(4):
        m = move(b, a)
        out.append(1 if np.array_equal(m, b) else 2 * min(3, int((m == 0).sum())))
    return out


def candidates(board):
    """[(action, reward, p)] in candidate order."""
    b = np.asarray(board, dtype=np.int64)
    old_max = tile(b.max())
    out = []
    for a in range(4):
        m = move(b, a)
        if np.array_equal(m, b):
            out.append((a, -1.0, 1.0))
            continue
        e = int((m == 0).sum())
        k = min(3, e)
        for j in range(2 * k):
            t = 4 if j & 1 else 2
            new_max = max(tile(m.max()), t)
            bonus = new_max if new_max > old_max else 0
            reward = (float(t + bonus) + (e - 1) * 0.1) * (0.1 if j & 1 else 0.9)
            out.append((a, reward, 1.0 / (2 * k)))
    return out


def action(board, width, search_depth=30, gamma=0.99, leaf=None):
    """The planned action. leaf: for search_depth == 1, float32 (32,) -- the maximum Q of the candidate board in slot 8 a + j."""
    keyed, j, last = [], 0, -1
    for a, reward, p in candidates(board):
        j = j + 1 if a == last else 0
        last = a
        total = 0.0 + reward
        if search_depth == 1:
            total = total + gamma * float(np.float32(leaf[8 * a + j]))
        keyed.append((total * p, a))
    order = sorted(range(len(keyed)), key=lambda i: (-keyed[i][0], i))[:width]
    sums, first = {}, {}
    for place, i in enumerate(order):
        key, a = keyed[i]
        if a in sums:
            sums[a] += key
        else:
            sums[a], first[a] = key, place
    return min(sums, key=lambda a: (-sums[a], first[a]))


def expand(board, h):
    """The candidate boards of one board from its draws h (4, 3): (succ uint8 (32,16), count (4,)). Pick i of action a is the
    ((h[a][i] >> 16) * (e - i)) >> 16-th empty cell of the moved board, row-major, among those not picked before."""
    b = np.asarray(board, dtype=np.int64)
    succ = np.zeros((SLOTS, 16), np.uint8)
    cnt = counts(b)
    for a in range(4):
        m = move(b, a)
        if cnt[a] == 1:
            succ[8 * a] = m
            continue
        empty = [c for c in range(16) if m[c] == 0]
        for i in range(cnt[a] // 2):
            cell = empty.pop(((int(h[a][i]) >> 16) * len(empty)) >> 16)
            for t in (0, 1):
                s = m.copy()
                s[cell] = 1 + t
                succ[8 * a + 2 * i + t] = s
    return succ, np.array(cnt, np.uint8)


def exploit(q, board):
    """The exploit action of select_action: Q of an invalid move replaced by -1e9, argmax with ties to the lowest index."""
    b = np.asarray(board, dtype=np.int64)
    q = np.asarray(q, dtype=np.float32).copy()
    for a in range(4):
        if np.array_equal(move(b, a), b):
            q[a] = np.float32(-1e9)
    return int(np.argmax(q))
