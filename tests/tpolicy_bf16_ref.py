"""What the CPU and the GPU tests of the transformer policy's bf16 gradient pass (include/g2048_tbf16.h) share: the cases with their
own board seeds, the rounded oracle (g2048.tpolicy.loss_grad_reference(ff_bf16=True)) in float64 and in float32, the two measures
the bound is made of, and the conditions every case must meet.

Two measures, both max|a - b| / max|b| of the worst gradient tensor of a case:
    intrinsic cost  the rounded float64 function against the UNROUNDED float64 function: what bf16 feed-forward products cost;
    flip noise      the rounded function in float32 against itself in float64: a value that differs by a float32 ulp between two
                    implementations sometimes rounds to the other bf16 neighbour, which cannot be predicted per element.
The device is held to CAP x the case's intrinsic cost against the rounded float64 oracle. CAP = 0.25: a wrong operand, a dropped
mask or a second rounding moves the result by about the intrinsic cost itself, four times the cap; flip noise, the only thing a
correct implementation differs by, is asserted here to stay a factor F32_FACTOR = 8 below the cap for every case. Both sides of
that reasoning are measured on the CPU and neither on the device.

Rounding moves the ReLU inputs, so tests/tpolicy_grad_ref.py's board seeds do not carry over: a case takes the first board seed
from N on, in steps of 1,000, at which the ROUNDED float64 function keeps RELU_MARGIN on every ReLU input (linear1 of every layer
after its rounded product, fc1, fc2), Case.conditions' rules hold and 8 x flip noise fits under the cap (SEEDS). The large cases
repeat a few distinct boards as there. Cases with dropout take the masks of (dropout seed, INDEX) and their own seeds."""
import copy
import functools

import numpy as np
import torch

import tpolicy_dropout_ref as D
import tpolicy_grad_ref as R

CAP = 0.25                                    # of the case's intrinsic cost; never above 0.5
INDEX = D.INDEX
P4, SITE2 = D.P4, (0.0, 0.0, 0.1, 0.0)
# (N, dim_ff, layers): tests/tpolicy_grad_ref.py's shapes
SHAPES = R.GPU_CASES
# (N, dim_ff, layers, p4 or None): board seed, distinct boards, dropout seed
SEEDS = {
    (15, 64, 2, None): (1015, 15, 0),            # board seed 15: margin 3.7e-7
    (16, 64, 2, None): (1016, 16, 0),            # board seed 16: a head ReLU changes sign in float32, flip noise 0.009
    (64, 2048, 2, None): (7064, 8, 0),           # board seeds 64 .. 6064: margins 2.8e-7 .. 1.3e-6
    (1024, 32, 2, None): (1024, 64, 0),
    (17, 96, 2, P4): (17, 17, 2),                # dropout seeds 0, 1: margins 7.8e-8, 1.9e-6
    (33, 160, 1, P4): (33, 33, 1),               # dropout seed 0: margin 1.97e-6
}
DROPOUT_CASES = ((17, 96, 2, P4), (33, 160, 1, P4), (17, 96, 2, SITE2), (33, 160, 1, SITE2))
ALL_CASES = tuple(s + (None,) for s in SHAPES) + DROPOUT_CASES
HOST_CASES = ((1, 32, 1, None), (17, 96, 2, None), (33, 160, 1, P4))
DISTINCT = {(64, 2048, 2): 8, (1024, 32, 2): 64}


def case_id(case):
    n, ff, layers, p4 = case
    return "n%d-ff%d-L%d%s" % (n, ff, layers, "" if p4 is None else "-p" + "_".join("%g" % p for p in p4))


def parsed_of(model):
    from g2048 import tpolicy
    return tpolicy.parse(model)


def reference(model32, args, dtype, ff_bf16, multipliers=None):
    """loss_grad_reference on the case's inputs as tests/tpolicy_grad_ref.stock_loss_grad returns it: float64 NumPy, grads per tensor."""
    from g2048 import tpolicy
    boards, actions, old, adv, ret = (torch.from_numpy(np.ascontiguousarray(x)) for x in args)
    p = parsed_of(model32)
    losses, probs, value, flat = tpolicy.loss_grad_reference(p, boards, actions, old, adv, ret, R.CLIP, R.VALUE_COEF, R.ENTROPY_COEF, dtype=dtype,
                                                             multipliers=multipliers, ff_bf16=ff_bf16)
    f64 = lambda t: t.detach().numpy().astype(np.float64)       # noqa: E731
    grads, eps = R.split(p, f64(flat))
    assert np.all(eps == 0)
    return dict(losses=f64(losses), probs=f64(probs), value=f64(value), grads=grads)


@torch.no_grad()
def relu_inputs(model32, boards, multipliers=None, dtype=torch.float64):
    """What the ROUNDED function feeds its ReLUs, per layer as flat float64 arrays: linear1 of every encoder layer (rnd(x1) rnd(W1)^T
    + b1), fc1, fc2. The forward of g2048.tpolicy.loss_grad_reference(ff_bf16=True) with the products' results kept."""
    from g2048 import _encoder_net as E
    from g2048 import tpolicy as T
    p, seen = parsed_of(model32), []
    w = E.weight_caster(dtype, None)

    def feed_forward(x, w1, b1, w2, b2, m2):
        z = T.rnd(x) @ T.rnd(w1).T + b1
        seen.append(z)
        return T.rnd(m2(torch.relu(z))) @ T.rnd(w2).T + b2

    x = torch.from_numpy(np.ascontiguousarray(boards)).to(dtype) / 15
    x = x.reshape(-1, T.TOKENS, 1) * w(p.embedding.weight).reshape(1, 1, -1) + w(p.embedding.bias)
    n = x.shape[0]
    for i, lay in enumerate(p.layers):
        a = lay.self_attn
        mult = None if multipliers is None else (lambda site, shape, dt, i=i: multipliers(i, site, shape, dt))
        qkv = x @ w(a.in_proj_weight).T + w(a.in_proj_bias)
        q, k, v = (t.reshape(n, T.TOKENS, T.N_HEAD, -1).transpose(1, 2) for t in qkv.split(T.D_MODEL, -1))
        s = torch.softmax((q @ k.transpose(-1, -2)) / 4, -1)
        if mult is not None:
            s = s * mult(0, tuple(s.shape), s.dtype)
        x = E.post_norm_tail(lay, x, (s @ v).transpose(1, 2).reshape(n, T.TOKENS, T.D_MODEL), w, mult, feed_forward)
    z1 = x.reshape(n, -1) @ w(p.fc1.weight).T + w(p.fc1.bias)
    z2 = torch.relu(z1) @ w(p.fc2.weight).T + w(p.fc2.bias)
    return [z.numpy().astype(np.float64).reshape(-1) for z in seen + [z1, z2]]


def relu_margin(model32, boards, multipliers=None):
    return min(float(np.abs(z).min() / np.abs(z).max()) for z in relu_inputs(model32, boards, multipliers))


def worst(a, b):
    """The worst gradient tensor's max|a - b| / max|b|."""
    return float(R.ratios(a["grads"], b["grads"]).max())


def others(a, b):
    """The same measure of the loss parts, probs and value."""
    return {k: R.rel(a[k], b[k]) for k in ("losses", "probs", "value")}


class Case:
    """One (N, dim_ff, layers, p4): the module, the inputs, the rounded oracle in float64 (want) and float32, the unrounded float64
    function, the two measures and the cap."""

    def __init__(self, case, board_seed=None, dropout_seed=None):
        self.case = case
        n, ff, layers, p4 = case
        self.n, self.dim_ff, self.layers, self.p4 = n, ff, layers, p4
        tuned = SEEDS.get(case, (n, DISTINCT.get((n, ff, layers), n), 0))
        self.board_seed = tuned[0] if board_seed is None else board_seed
        self.distinct = tuned[1]
        self.seed = tuned[2] if dropout_seed is None else dropout_seed          # the dropout seed
        self.index = INDEX
        self.model32 = R.stock_module(ff, layers)
        model64 = copy.deepcopy(self.model32).double()
        self.boards = R.boards_of(n, self.board_seed, self.distinct)
        self.actions, self.old, self.adv, self.ret = R.recipe(model64, self.boards, self.board_seed, 0.5)
        self.args = (self.boards, self.actions, self.old, self.adv, self.ret)
        self.multipliers = None if p4 is None else D.multipliers_of(self.seed, self.index, p4, n, ff)
        self.want = reference(self.model32, self.args, torch.float64, True, self.multipliers)
        self.unrounded = reference(self.model32, self.args, torch.float64, False, self.multipliers)
        self.rounded32 = reference(self.model32, self.args, torch.float32, True, self.multipliers)
        self.intrinsic = worst(self.want, self.unrounded)
        self.flip = max(worst(self.rounded32, self.want), *others(self.rounded32, self.want).values())
        self.cap = CAP * self.intrinsic
        self.clipped_share = self._clipped_share()

    def _clipped_share(self):
        """The share of rows on which the clipped branch is the minimum, on the rounded oracle's probabilities."""
        eps = float(np.finfo(np.float32).eps)
        qn = self.want["probs"] / self.want["probs"].sum(1, keepdims=True)
        logp = np.log(np.clip(qn, eps, 1 - eps))[np.arange(self.n), self.actions]
        ratio, adv = np.exp(logp - self.old.astype(np.float64)), self.adv.astype(np.float64)
        return float((np.clip(ratio, 1 - R.CLIP, 1 + R.CLIP) * adv < ratio * adv).mean())

    def failed(self):
        """The conditions the case misses, as text (empty: none)."""
        out = []
        if self.n > 2 and not R.BAND[0] <= self.clipped_share <= R.BAND[1]:
            out.append("clipped share %.2f" % self.clipped_share)
        if self.n > 1 and not ((self.adv > 0).any() and (self.adv < 0).any()):
            out.append("advantages of one sign")
        if self.n > 2 and np.abs(self.want["value"]).max() < R.VALUE_FLOOR:
            out.append("the value head cancels: max|value| %.3g" % np.abs(self.want["value"]).max())
        if not all(np.abs(g).max() > 0 for g in self.want["grads"]):
            out.append("a gradient tensor of the rounded float64 function is zero")
        self.relu_margin = relu_margin(self.model32, self.boards, self.multipliers)
        if self.relu_margin < R.RELU_MARGIN:
            out.append("a ReLU input of the rounded function is within rounding of zero (margin %.3g)" % self.relu_margin)
        if not self.intrinsic > 0:
            out.append("rounding changes nothing")
        if not R.F32_FACTOR * self.flip <= self.cap:
            out.append("8 x flip noise %.3g exceeds the cap %.3g" % (R.F32_FACTOR * self.flip, self.cap))
        return out

    def conditions(self):
        missed = self.failed()
        assert not missed, "%s, board seed %d, dropout seed %d: %s" % (case_id(self.case), self.board_seed, self.seed, "; ".join(missed))


@functools.lru_cache(maxsize=None)
def case(c):
    return Case(c)


def find_seeds(c, limit=40):
    """(board seed, distinct boards, dropout seed) of the first board seed from N on, in steps of 1,000, that meets the conditions:
    how SEEDS was made."""
    n = c[0]
    for k in range(limit):
        got = Case(c, board_seed=n + 1000 * k)
        if not got.failed():
            return got.board_seed, got.distinct, got.seed
    raise RuntimeError("no board seed meets the conditions at %s" % (c,))


# ------------------------------------------------------------------------------------------------------- the products --
def rnd64(a):
    """rnd of a float array (any dtype), as float64 NumPy."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()


def bf16_spacing(v):
    """The distance between the bf16 neighbours of |v| (normal range)."""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 1e-30))) - 7)


def ties(shape, rng):
    """float32 values on bf16 ties and just either side of them: (1 + (2 k + 1) 2^-8) 2^e, and the float32 neighbours of each.
    Round to nearest even takes a tie to the even bf16 mantissa and the neighbours to opposite sides; truncation takes all three
    down."""
    k = rng.integers(0, 64, size=shape)
    e = rng.integers(-3, 4, size=shape)
    side = rng.integers(-1, 2, size=shape)                     # -1, 0, +1 float32 ulps from the tie
    sign = rng.choice([-1.0, 1.0], size=shape)
    tie = ((1.0 + (2 * k + 1) * 2.0 ** -8) * 2.0 ** e).astype(np.float32)
    moved = (tie.view(np.int32) + side.astype(np.int32)).view(np.float32)
    return (sign * moved).astype(np.float32)
