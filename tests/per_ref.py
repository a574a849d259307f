"""NumPy restatement of the hybrid agent's prioritized replay (agents/hybrid.py:730-765) and of train_step's reward shaping
(:971-1034), with every dtype spelled out. tests/test_per_host.py holds it to tests/golden/per.npz (what the reference's own
classes returned) with ==; the GPU tests use it as the reference of the entry points in csrc/g2048_per.hip.

Boards are uint8 log2 codes (n, 16), row-major; the reference's states are the float32 tile values 2 ** code (0 = empty).
"""
import numpy as np

f32, f64 = np.float32, np.float64
DOM_REPLAY = 10                       # the RNG domain of the sample draws (csrc/g2048_board.h)

# 16 - snake_pattern (:801-806), row-major
SNAKE_POSITION = np.array([1, 2, 3, 4, 8, 7, 6, 5, 9, 10, 11, 12, 16, 15, 14, 13], dtype=np.int64)


def tiles_f32(codes):
    c = np.asarray(codes, dtype=np.int64)
    return np.where(c > 0, 1 << c, 0).astype(f32)


def shaped_reward(state, next_state, reward):
    """One iteration of the loop :974-1032, then the rounding of :1034. state / next_state: 16 codes; reward: float32."""
    b = np.asarray(next_state, dtype=np.int64).reshape(4, 4)
    mc = int(b.max())
    s = f64(f32(reward)) * f64(0.1)                                   # :980 Python floats
    if mc > 0:
        s = f32(s) + f32(mc) * f32(2.0)                               # :985 float32 + float32 (the Python float is weak)
    snake = int((b.reshape(16) * SNAKE_POSITION).sum())               # :988-995 exact small integer
    s = f64(s) + (f64(snake) / f64(500.0)) * f64(10.0)                # :998 float64 from here on
    if mc > 6:                                                        # :1001 max_tile > 64
        if b[3, 3] == mc:
            s = s + f64(f32(mc) * f32(5.0))
        elif b[0, 0] == mc:
            s = s + f64(f32(mc) * f32(2.0))
    s = s + f64(int((b == 0).sum())) * f64(0.5)                       # :1008-1009
    merge = 0                                                         # :1012-1023 a float32 sum of tile values: exact
    for r in range(4):
        for c in range(4):
            if b[r, c] > 0:
                if c < 3 and b[r, c] == b[r, c + 1]:
                    merge += 1 << int(b[r, c])
                if r < 3 and b[r, c] == b[r + 1, c]:
                    merge += 1 << int(b[r, c])
    assert merge < 1 << 24
    s = s + f64(f32(merge) * f32(0.01))                               # :1025 a float32 product
    if mc > int(np.asarray(state).max()):                             # :1028-1029
        s = s + f64(f32(1 << mc) * f32(0.5))
    return f32(s)                                                     # :1034


def shaped_rewards(states, next_states, rewards):
    return np.array([shaped_reward(s, n, r) for s, n, r in zip(states, next_states, rewards)], dtype=f32).reshape(-1)


def priority_of(td_errors):
    """update_priorities(indices, td_errors + 1e-5) (:1063-1064, :762): float32 sum, then max(priority, 1e-5) stored as float32."""
    v = np.asarray(td_errors, dtype=f32) + f32(1e-5)
    return np.where(f32(1e-5) > v, f32(1e-5), v).astype(f32)


def probs_of(priorities, alpha):
    """:746-748 float32 throughout (NumPy's own float32 sum)."""
    p = np.asarray(priorities, dtype=f32) ** f32(alpha)
    return (p / p.sum()).astype(f32)


def cdf_of(probs):
    """np.random.choice(p=probs): the float64 running sum in order, divided by its last element."""
    cdf = np.cumsum(np.asarray(probs).astype(f64))
    return cdf / cdf[-1]


def search(cdf, u):
    return np.searchsorted(cdf, np.asarray(u, dtype=f64), side="right").astype(np.int64)


def weights_of(probs, indices, size, beta):
    """:754-755 float32 throughout."""
    w = (f32(size) * np.asarray(probs, dtype=f32)[indices]) ** f32(-beta)
    return (w / w.max()).astype(f32)


def probs_f64(priorities, alpha):
    p = np.asarray(priorities).astype(f64) ** f64(alpha)
    return p / p.sum()


def weights_f64(probs64, indices, size, beta):
    w = (f64(size) * probs64[indices]) ** f64(-beta)
    return w / w.max()


def near_cdf(cdf, u, eps):
    """True for the draws within eps of an entry of cdf: the ones a comparison of two evaluations of the cdf may leave out."""
    u = np.asarray(u, dtype=f64)
    k = np.clip(np.searchsorted(cdf, u), 0, len(cdf) - 1)
    d = np.abs(cdf[k] - u)
    d = np.minimum(d, np.abs(cdf[np.maximum(k - 1, 0)] - u))
    return d <= eps


class Buffer:
    """PrioritizedReplayBuffer on arrays, in logical (deque) order. Transitions are rows of (state codes, action, float32 reward,
    next state codes, done)."""

    def __init__(self, capacity, alpha):
        self.capacity, self.alpha = int(capacity), alpha
        self.states = np.zeros((0, 16), np.uint8)
        self.next_states = np.zeros((0, 16), np.uint8)
        self.actions = np.zeros(0, np.uint8)
        self.rewards = np.zeros(0, f32)
        self.dones = np.zeros(0, np.uint8)
        self.priorities = np.zeros(0, f32)

    def __len__(self):
        return len(self.priorities)

    def push(self, states, actions, rewards, next_states, dones):
        m = len(actions)
        top = self.priorities.max() if len(self) else f32(1.0)        # :738, the same for the whole batch (csrc/g2048_per.h)
        keep = slice(max(0, len(self) + m - self.capacity), None)

        def cat(old, new, dtype):
            return np.concatenate([old, np.asarray(new, dtype=dtype)])[keep]
        self.states = cat(self.states, states, np.uint8)
        self.next_states = cat(self.next_states, next_states, np.uint8)
        self.actions = cat(self.actions, actions, np.uint8)
        self.rewards = cat(self.rewards, np.asarray(rewards).astype(f32), f32)
        self.dones = cat(self.dones, dones, np.uint8)
        self.priorities = cat(self.priorities, np.full(m, top, f32), f32)

    def sample(self, u, beta):
        probs = probs_of(self.priorities, self.alpha)
        indices = search(cdf_of(probs), u)
        return indices, probs, weights_of(probs, indices, len(self), beta)

    def update_priorities(self, indices, td_errors):
        for i, v in zip(np.asarray(indices, dtype=np.int64), priority_of(td_errors)):     # in order: the last duplicate wins
            if 0 <= i < len(self):
                self.priorities[i] = v


# ------------------------------------------------------------------------------------- the scripted runs of tests/golden/per.npz --
PUSH, SAMPLE, UPDATE = 0, 1, 2


def script(golden, r):
    """The ops of run r of the fixture, in order: dicts with kind, k (the op's number), and for a push the pool rows `rows`, for a
    sample batch / beta / u / idx / probs / w / perr / werr and the sampled transitions s*, for an update uidx / td; prio = the
    priorities in deque order after the op."""
    cursor = sum(int(golden["r%d_arg" % q][golden["r%d_kind" % q] == PUSH].sum()) for q in range(r))
    for k, (kind, arg, beta) in enumerate(zip(golden["r%d_kind" % r], golden["r%d_arg" % r], golden["r%d_beta" % r])):
        get = lambda name: golden["r%d_%s_%d" % (r, name, k)]          # noqa: E731
        op = dict(kind=int(kind), k=k, prio=get("prio"))
        if kind == PUSH:
            op["rows"] = slice(cursor, cursor + int(arg))
            cursor += int(arg)
        elif kind == SAMPLE:
            op.update(batch=int(arg), beta=float(beta), **{n: get(n) for n in ("u", "idx", "probs", "w", "perr", "werr", "sstate", "snext",
                                                                               "saction", "sreward", "sdone")})
        else:
            op.update(uidx=get("uidx"), td=get("td"))
        yield op
