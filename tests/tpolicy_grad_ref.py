"""What the CPU and the GPU tests of the transformer policy's loss and gradient pass share: stock-torch modules of the reference's
layout (RefSpelling of tests/test_tpolicy_host.py, eval mode), the inputs' recipe, the module's own autograd through the lines of
PPOAgent.update()'s loss (agents/ppo_agent.py:378-400) on its two heads -- the yardstick in float64, the tolerance's measure in
float32 -- and the conditions the inputs must meet for the comparison to mean something. Tensors are numbered in the plain layout's
order, which is the module's parameter order.

The tolerance is tests/ppo_update_ref.py's: per case and tensor max|got - f64| / max|f64| <= F32_FACTOR x the worst such ratio of
stock CPU float32 autograd over the case's gradient tensors; loss parts, probs and value are held to the same bound relative to
their own maxima.

The recipe: actions (5 i + 1) % 4, old_log_probs = the float64 module's own log-probabilities + noise x N(0, 1), advantages of both
signs that correlate with the board, returns around the module's own value. A case is kept only if the clipped branch is the
minimum on 10 % .. 90 % of its rows (clipped_share; N = 1 and N = 2 are excused) and no gradient tensor is zero: a zeroed policy
gradient cannot pass. Its values reach VALUE_FLOOR (N > 2), so that an error relative to max|value| is no cancellation
artefact. Where a case misses the band its noise scale or seed is changed, never the band."""
import copy
import functools

import numpy as np
import torch

from qnet_grad_ref import F32_FACTOR, plain_slices, ratios  # noqa: F401  (re-exported)
from test_tpolicy_host import RefSpelling

CLIP, VALUE_COEF, ENTROPY_COEF = 0.3, 0.4, 0.05          # PPOAgent's own settings
BAND = (0.10, 0.90)
WEIGHT_SEED = 29
# The weight seed per (dim_ff, layers) where the default's critic head nearly cancels: under seed 29 the (32, 2) module's values stay
# below 0.3 while the products that make them up do not, and stock float32's OWN value error is then 4 .. 10 x its gradient error
# (measured on the CPU, one to sixteen threads): no float32 pass can meet a bound that is relative to max|value| there. Of the
# seeds 29 .. 44, 39 keeps max|value| above 1 at every size used here, float32's own value error at or below 1.2 x its gradient
# error, and its yardstick below 1e-5 at N = 1,024 (under seed 34 a ReLU input of the float32 module changes sign there).
WEIGHT_SEEDS = {(32, 2): 39}
VALUE_FLOOR = 0.5                                        # max|value| of a case with N > 2: the value head does not cancel
ROW_CHUNK = 512 // 16                                    # boards per chunk of the row-split weight gradient (kRowChunk rows)
# (N, dim_ff, layers): the 16-row tile edge, more than one block, the reference's shape, the row-split's chunk edge, the limit
GPU_CASES = ((1, 32, 1), (2, 32, 2), (15, 64, 2), (16, 64, 2), (17, 96, 2), (33, 160, 1), (64, 2048, 2),
             (ROW_CHUNK - 1, 32, 2), (ROW_CHUNK, 32, 2), (ROW_CHUNK + 1, 32, 2), (1024, 32, 2))
HOST_CASES = ((1, 32, 1), (17, 96, 2), (33, 2048, 2))
# A ReLU input within rounding of zero has one sign in float64 and maybe the other in float32: the unit's gradient is then on in one
# and off in the other, and a bias gradient moves by a whole row's share (1e-3 of max|g| at N = 1,024, in stock float32 as on the
# device). So every ReLU input of a case (linear1 of every layer, fc1, fc2; float64) keeps RELU_MARGIN x the largest of its layer:
# about ten times the float32 rounding of such a product. A case has 16 N dim_ff layers of them: the large cases repeat a few
# distinct boards (boards[i % distinct], as tests/ppo_update_ref.py does above 300 rows), their rows still differing in action,
# old log-probability, advantage and return, and take the first board seed from N on, in steps of 1,000, that keeps the margin.
RELU_MARGIN = 2e-6
# per case: (board seed, noise scale, distinct boards); the default is (N, 0.5, N). tests/test_tpolicy_grad_host.py asserts the
# conditions for every case.
TUNED = {(64, 2048, 2): (1064, 0.5, 8), (33, 2048, 2): (9033, 0.5, 8), (1024, 32, 2): (1024, 0.5, 64)}


def stock_module(dim_ff, layers, seed=None):
    """A float32 RefSpelling in eval mode: torch's default init, the two heads x 8 (default init gives near-uniform probabilities
    for every board), LayerNorm weights and biases perturbed (their defaults 1 and 0 hide a swapped or dropped term)."""
    seed = WEIGHT_SEEDS.get((dim_ff, layers), WEIGHT_SEED) if seed is None else seed
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        model = RefSpelling(dim_ff, layers)
        gen = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            model.actor.weight.mul_(8.0)
            model.critic.weight.mul_(8.0)
            for lay in model.transformer_encoder.layers:
                for norm in (lay.norm1, lay.norm2):
                    norm.weight.copy_(1 + 0.3 * torch.randn(64, generator=gen))
                    norm.bias.copy_(0.2 * torch.randn(64, generator=gen))
    return model.eval()


def boards_of(n, seed, distinct=None):
    """uint8 (n,16) random boards, codes 0..11, a third of the cells empty; with distinct < n, boards[i % distinct]."""
    distinct = n if distinct is None else min(n, distinct)
    rng = np.random.default_rng(1000 + seed)
    b = rng.integers(0, 12, size=(distinct, 16)).astype(np.uint8)
    b[rng.random((distinct, 16)) < 0.35] = 0
    return np.ascontiguousarray(b[np.arange(n) % distinct])


def relu_margin(model64, boards):
    """min over the ReLU inputs' layers (linear1 of every encoder layer, fc1, fc2) of min|z| / max|z|, from the float64 module."""
    seen, hooks = [], []
    mods = [lay.linear1 for lay in model64.transformer_encoder.layers] + [model64.fc1, model64.fc2]
    for m in mods:
        hooks.append(m.register_forward_hook(lambda _m, _i, out: seen.append(float(out.detach().abs().min() / out.detach().abs().max()))))
    try:
        with torch.enable_grad():            # (with gradients enabled the encoder layer takes the path that calls linear1)
            model64(torch.from_numpy(np.unique(boards, axis=0)).double() / 15)
    finally:
        for h in hooks:
            h.remove()
    assert len(seen) == len(mods)
    return min(seen)


def find_board_seed(model64, n, distinct, limit=400):
    for k in range(limit):
        if relu_margin(model64, boards_of(n, n + 1000 * k, distinct)) >= RELU_MARGIN:
            return n + 1000 * k
    raise RuntimeError("no board seed keeps the ReLU margin at n = %d" % n)


def stock_loss_grad(model, boards, actions, old_log_probs, advantages, returns, clip=CLIP, value_coef=VALUE_COEF,
                    entropy_coef=ENTROPY_COEF):
    """ppo_agent.py:378-400 up to backward() on the stock module (eval mode) in its own dtype, the two heads taking the places of
    the actor and the critic. Everything as float64 NumPy: dict(losses (loss, actor_loss, value_loss, entropy), probs, value,
    grads [per parameter, flattened], log_probs, clipped: per row, is the clipped branch the minimum)."""
    dtype = next(model.parameters()).dtype
    x = torch.from_numpy(np.asarray(boards)).to(dtype) / 15
    a = torch.from_numpy(np.asarray(actions))
    old, adv, ret = (torch.from_numpy(np.asarray(t)).to(dtype) for t in (old_log_probs, advantages, returns))
    model.zero_grad()
    probs, value = model(x)
    dist = torch.distributions.Categorical(probs=probs)
    new_log_probs = dist.log_prob(a)
    entropy = dist.entropy().mean()
    ratio = torch.exp(new_log_probs - old)
    s1, s2 = ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv
    actor_loss = -torch.min(s1, s2).mean()
    value_loss = ((value[:, 0] - ret) ** 2).mean()
    loss = actor_loss + value_coef * value_loss - entropy_coef * entropy
    loss.backward()
    f64 = lambda t: t.detach().numpy().astype(np.float64)       # noqa: E731
    grads = [f64(p.grad).reshape(-1) for p in model.parameters()]
    model.zero_grad()
    return dict(losses=np.array([float(t.detach()) for t in (loss, actor_loss, value_loss, entropy)]), probs=f64(probs), value=f64(value),
                grads=grads, log_probs=f64(new_log_probs), clipped=f64(s2) < f64(s1))


def recipe(model64, boards, seed, noise):
    """(actions int64, old_log_probs, advantages, returns float32) of the boards."""
    n = len(boards)
    i = np.arange(n, dtype=np.int64)
    actions = (5 * i + 1) % 4
    zero = np.zeros(n, dtype=np.float32)
    own = stock_loss_grad(model64, boards, actions, zero, zero, zero)
    rng = np.random.default_rng(77 + seed)
    old = own["log_probs"] + noise * rng.standard_normal(n)
    adv = ((13 * i) % 17 - 8) / 4.0 + 2.0 * boards[:, 0].astype(np.float64) / 15.0 + (0.25 if n < 3 else 0.0)
    ret = own["value"][:, 0] + 0.5 + boards.astype(np.float64).sum(1) / 120.0 + ((7 * i) % 11 - 5) / 5.0
    return actions, old.astype(np.float32), adv.astype(np.float32), ret.astype(np.float32)


class Case:
    """One (N, dim_ff, layers): the float32 and float64 modules, the inputs, the float64 yardstick, stock float32's own error and
    the bound."""

    def __init__(self, n, dim_ff, layers, model32=None, boards=None):
        self.n, self.dim_ff, self.layers = n, dim_ff, layers
        seed, noise, distinct = TUNED.get((n, dim_ff, layers), (n, 0.5, n))
        self.model32 = model32 if model32 is not None else stock_module(dim_ff, layers)
        self.model64 = copy.deepcopy(self.model32).double()
        self.boards = boards_of(n, seed, distinct) if boards is None else boards
        self.actions, self.old, self.adv, self.ret = recipe(self.model64, self.boards, seed, noise)
        self.args = (self.boards, self.actions, self.old, self.adv, self.ret)
        self.want = stock_loss_grad(self.model64, *self.args)
        self.f32 = stock_loss_grad(self.model32, *self.args)
        self.yardstick = float(ratios(self.f32["grads"], self.want["grads"]).max())
        self.bound = F32_FACTOR * self.yardstick
        self.clipped_share = float(self.want["clipped"].mean())

    def conditions(self):
        """Asserted, not assumed: the clipped branch binds on 10 .. 90 % of the rows (N > 2), advantages of both signs (N > 1), no
        gradient tensor is zero, and stock float32 is off by something."""
        if self.n > 2:
            assert BAND[0] <= self.clipped_share <= BAND[1], "clipped share %.2f at %s" % (self.clipped_share, (self.n, self.dim_ff, self.layers))
        if self.n > 1:
            assert (self.adv > 0).any() and (self.adv < 0).any()
        assert relu_margin(self.model64, self.boards) >= RELU_MARGIN, "a ReLU input is within rounding of zero"
        if self.n > 2:
            assert np.abs(self.want["value"]).max() >= VALUE_FLOOR, "the value head cancels: max|value| %.3g" % np.abs(self.want["value"]).max()
        assert all(np.abs(g).max() > 0 for g in self.want["grads"]), "a gradient tensor of the float64 module is zero"
        assert 0 < self.yardstick < 1e-4, self.yardstick


@functools.lru_cache(maxsize=None)
def case(n, dim_ff, layers):
    return Case(n, dim_ff, layers)


def rel(got, want):
    """max|got - want| / max|want| of one tensor."""
    return float(ratios([np.asarray(got, np.float64)], [np.asarray(want, np.float64)])[0])


def split(parsed, flat):
    """A flat gradient in the plain layout as (per-tensor float64 arrays, the LayerNorm-eps slots' values)."""
    slices, eps, total = plain_slices(parsed)
    g = np.asarray(flat, np.float64)
    assert g.shape == (total,)
    return [g[o:o + k] for o, k in slices], g[eps]


# ---- the golden fixture (tests/golden/tpolicy_grad.npz): the recipe weights of tests/tpolicy_weights.py, 32 boards of policy.npz
GOLDEN_ROWS, GOLDEN_STRIDE, GOLDEN_FULL = 32, 97, 4096


def golden_positions(numel):
    """The flat indices of a gradient tensor the fixture stores: all of them up to 4,096 elements, else every 97th."""
    return np.arange(numel) if numel <= GOLDEN_FULL else np.arange(0, numel, GOLDEN_STRIDE)
