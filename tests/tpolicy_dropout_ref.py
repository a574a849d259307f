"""What the CPU and the GPU tests of the transformer policy's training-mode dropout share (tests/test_tpolicy_dropout_host.py,
tests/test_gpu_tpolicy_dropout.py).

The mask rule, restated in NumPy uint32 from its specification (include/g2048_ttrain.h), not imported from the library: for the
library call with index c, (k0, k1) = rng_keys(seed, 13, c); element e of site s of encoder layer L draws
h = rng_draw(k0, k1, ((4 L + s) << 32) | e, 0) and is kept iff h >= T = floor(p_s 2^32); a kept element is multiplied by
1 / (1 - p_s), a dropped one by 0. For n boards of 16 tokens: site 0, the attention probabilities, e = ((board 4 + head) 16 + query)
16 + key, matrix (64 n, 16); sites 1 and 3, dropout1 / dropout2, e = token 64 + feature, (16 n, 64); site 2, the hidden layer's
dropout, e = token dim_ff + feature, (16 n, dim_ff). The hash itself (splitmix64, rng_keys, rng_draw) is the restatement
tests/ppo_dropout_ref.py already holds.

The yardstick: the STOCK module in .train() mode, fed those masks by replacing torch.nn.functional.dropout and
torch.nn.functional.scaled_dot_product_attention for the duration of a call (feeding()). The training-mode layer calls them in the
order SDPA (n, 4, 16, 16), dropout (n, 16, 64), (n, 16, dim_ff), (n, 16, 64) per layer, which is the order of the sites; every call
asserts its shape and the probability torch passes. tpolicy_grad_ref.stock_loss_grad on such a module in float64 (scale
1 / (1 - p) in double) is the reference, the same module in float32 (the float scale) the tolerance's measure: per tensor
max|got - f64| / max|f64| <= 8 x the float32 run's worst such ratio over the gradient tensors of the same case (F32_FACTOR), and
that ratio itself must lie in (0, FAIR_F32]. The inputs are tpolicy_grad_ref's cases (boards, actions, old log-probabilities,
advantages, returns); their conditions are asserted again UNDER THE MASKS (Case.conditions). The dropout seed of a case is the
first from 0 upwards that meets them (SEEDS names the cases whose seed is not 0); the host test checks every case.
"""
import copy
import functools

import numpy as np
import torch

import encoder_dropout_ref as E
import tpolicy_grad_ref as R

DOMAIN = 13
HIGH_INDEX = (1 << 32) + 7            # a call index above 2^32
FAIR_F32 = 1e-5                       # above this stock float32 is no yardstick
P4 = (0.1, 0.1, 0.1, 0.1)
HALF = (0.5, 0.5, 0.5, 0.5)
UNEQUAL = (0.3, 0.0, 0.2, 0.1)        # a site with p = 0 next to live ones, no two sites alike
INDEX = 7
# (N, dim_ff, layers, p4, call index): the loss-and-gradient cases
LOSS_CASES = tuple((n, ff, l, P4, INDEX) for n, ff, l in R.GPU_CASES) + ((17, 96, 2, HALF, INDEX), (17, 96, 2, UNEQUAL, HIGH_INDEX))
SEEDS = {(33, 160, 1, P4, INDEX): 1}  # case -> dropout seed, where the first seed that meets the conditions is not 0 (here: the ReLU margin)
UPDATE_N, UPDATE_SHAPE, UPDATE_EPOCHS, UPDATE_LR, GAMMA = 48, (96, 2), 2, 1e-4, 0.995


def case_id(case):
    n, ff, l, p4, index = case
    return "n%d-ff%d-L%d-p%s%s" % (n, ff, l, "_".join("%g" % p for p in p4) if len(set(p4)) > 1 else "%g" % p4[0], "-hi" if index >= 1 << 32 else "")


# ------------------------------------------------------------------------------------------------------ the mask rule --
def site_shape(site, n, dim_ff):
    return (64 * n, 16) if site == 0 else (16 * n, dim_ff if site == 2 else 64)


ENCODER = E.Encoder(DOMAIN, site_shape, lambda n: (n, 4, 16, 16), lambda n, width: (n, 16, width),
                    lambda model: model.transformer_encoder.layers)
# the mask rule and the stock module, masked (encoder_dropout_ref.py)
keep_mask, multiplier, feeding, training_copy, dims = (ENCODER.keep_mask, ENCODER.multiplier, ENCODER.feeding, ENCODER.training_copy,
                                                       ENCODER.dims)


def multipliers_of(seed, call_index, p4, n, dim_ff):
    """The callable g2048.tpolicy.loss_grad_reference takes as `multipliers`."""
    return lambda layer, site, shape, dtype: multiplier(seed, call_index, layer, site, p4[site], n, dim_ff, dtype).reshape(shape)


def masked_loss_grad(model, p4, seed, call_index, boards, actions, old, adv, ret):
    """tpolicy_grad_ref.stock_loss_grad of the training-mode module (training_copy) under the masks of (seed, call_index)."""
    dim_ff, layers = dims(model)
    with feeding(seed, call_index, p4, len(boards), dim_ff) as calls:
        out = R.stock_loss_grad(model, boards, actions, old, adv, ret)
    assert calls[0] == 4 * layers
    return out


@torch.no_grad()
def masked_forward(model, p4, seed, call_index, boards):
    """(probs (n,4), value (n,1)) float64 NumPy of the training-mode module under the masks of (seed, call_index)."""
    dim_ff, layers = dims(model)
    dtype = next(model.parameters()).dtype
    with feeding(seed, call_index, p4, len(boards), dim_ff) as calls:
        probs, value = model(torch.from_numpy(np.asarray(boards)).to(dtype) / 15)
    assert calls[0] == 4 * layers
    return probs.numpy().astype(np.float64), value.numpy().astype(np.float64)


def relu_inputs_masked(model, p4, seed, call_index, boards):
    """What the training-mode module under the masks feeds its ReLUs (linear1 of every encoder layer, fc1, fc2), over ALL the
    boards (a mask belongs to a position, so a repeated board is another input): the hooks see the masked layers' outputs."""
    seen, hooks = [], []
    mods = [lay.linear1 for lay in model.transformer_encoder.layers] + [model.fc1, model.fc2]
    for m in mods:
        hooks.append(m.register_forward_hook(lambda _m, _i, out: seen.append(out.detach().numpy().astype(np.float64).reshape(-1))))
    try:
        masked_forward(model, p4, seed, call_index, boards)
    finally:
        for h in hooks:
            h.remove()
    assert len(seen) == len(mods)
    return seen


def relu_margin_masked(model, p4, seed, call_index, boards):
    """tpolicy_grad_ref.relu_margin of the training-mode float64 module under the masks."""
    return min(float(np.abs(z).min() / np.abs(z).max()) for z in relu_inputs_masked(model, p4, seed, call_index, boards))


# The ReLU margin under the masks. tpolicy_grad_ref keeps every ReLU input RELU_MARGIN x its layer's largest away from zero, and
# reaches that at the large shapes by repeating a few boards. Under dropout a repeated board at another position is another input,
# so a case has 16 N dim_ff layers + 192 N distinct ReLU inputs: 1.2e6 at (1024, 32, 2), 4.2e6 at (64, 2048, 2). Their density at
# zero is about 1 per unit of the layer's largest, so about 2 K RELU_MARGIN of K inputs lie inside the margin: below one only up
# to K of about 2^18, and five and seventeen of them at those two shapes whatever the seed (dropout seeds 0 .. 39 all miss there,
# their margins 2e-8 .. 1.5e-6). So the margin itself is asserted for the cases of at most RELU_MARGIN_INPUTS inputs, and for every
# case what the margin is there to protect: the float32 masked module takes the same side of every ReLU as the float64 one, so its
# deviation -- the yardstick -- is rounding and not a unit that is on in one and off in the other.
RELU_MARGIN_INPUTS = 1 << 18


# ------------------------------------------------------------------------------------------------------------ the cases --
class Case:
    """One loss-and-gradient case: tpolicy_grad_ref's case of the shape for the modules and the inputs, the masked float64 module
    for the reference, the masked float32 module for the bound."""

    def __init__(self, case, seed=None):
        self.case = case
        n, ff, layers, p4, index = case
        self.n, self.dim_ff, self.layers, self.p4, self.index = n, ff, layers, p4, index
        self.seed = SEEDS.get(case, 0) if seed is None else seed
        base = R.case(n, ff, layers)
        self.model32, self.boards, self.args = base.model32, base.boards, base.args
        self.adv = base.adv
        self.train64, self.train32 = training_copy(base.model32, p4, torch.float64), training_copy(base.model32, p4, torch.float32)
        self.want = masked_loss_grad(self.train64, p4, self.seed, index, *self.args)
        self.f32 = masked_loss_grad(self.train32, p4, self.seed, index, *self.args)
        self.yardstick = float(R.ratios(self.f32["grads"], self.want["grads"]).max())
        self.bound = R.F32_FACTOR * self.yardstick
        self.clipped_share = float(self.want["clipped"].mean())
        self.max_value = float(np.abs(self.want["value"]).max())

    def failed(self):
        """The conditions the case misses under the masks, as text (empty: none)."""
        out = []
        if self.n > 2 and not R.BAND[0] <= self.clipped_share <= R.BAND[1]:
            out.append("clipped share %.2f" % self.clipped_share)
        if self.n > 2 and self.max_value < R.VALUE_FLOOR:
            out.append("the value head cancels: max|value| %.3g" % self.max_value)
        if not all(np.abs(g).max() > 0 for g in self.want["grads"]):
            out.append("a gradient tensor of the float64 module is zero")
        if not 0 < self.yardstick <= FAIR_F32:
            out.append("the float32 yardstick is %.3g" % self.yardstick)
        z64 = relu_inputs_masked(self.train64, self.p4, self.seed, self.index, self.boards)
        z32 = relu_inputs_masked(self.train32, self.p4, self.seed, self.index, self.boards)
        self.relu_inputs = sum(z.size for z in z64)
        self.relu_margin = min(float(np.abs(z).min() / np.abs(z).max()) for z in z64)
        if self.relu_inputs <= RELU_MARGIN_INPUTS and self.relu_margin < R.RELU_MARGIN:
            out.append("a ReLU input is within rounding of zero (margin %.3g)" % self.relu_margin)
        if not all(np.array_equal(a > 0, b > 0) for a, b in zip(z64, z32)):
            out.append("a ReLU is on in one of the float64 and the float32 masked modules and off in the other")
        return out

    def conditions(self):
        missed = self.failed()
        assert not missed, "%s, dropout seed %d: %s" % (case_id(self.case), self.seed, "; ".join(missed))


@functools.lru_cache(maxsize=None)
def loss_case(case):
    return Case(case)


def first_seed(case, limit=16):
    """The first dropout seed from 0 upwards under which the case meets its conditions."""
    for seed in range(limit):
        if not Case(case, seed).failed():
            return seed
    raise RuntimeError("no dropout seed below %d meets the conditions of %s" % (limit, case_id(case)))


@torch.no_grad()
def plain_loss_grad(c, dtype=torch.float64):
    """The case through g2048.tpolicy.loss_grad_reference with the restated masks: plain torch ops, no module called."""
    from g2048 import tpolicy
    parsed = tpolicy.parse(copy.deepcopy(c.model32).to(dtype).eval())
    boards, actions, old, adv, ret = (torch.from_numpy(np.asarray(t)) for t in c.args)
    losses, probs, value, flat = tpolicy.loss_grad_reference(parsed, boards, actions, old, adv, ret, dtype=dtype,
                                                             multipliers=multipliers_of(c.seed, c.index, c.p4, c.n, c.dim_ff))
    grads, eps = R.split(parsed, flat.numpy())
    return dict(losses=losses.numpy().astype(np.float64), probs=probs.numpy().astype(np.float64), value=value.numpy().astype(np.float64),
                grads=grads, eps=eps)


# ------------------------------------------------------------------------------------------------------ one closed update --
def update_inputs():
    """(boards, actions, old_log_probs, rewards, next_boards, dones) of the closed update: N = 48 boards at (96, 2), the boards
    rolled by one as their successors, by tests/test_gpu_tpolicy_step.py's recipe."""
    base = R.case(UPDATE_N, *UPDATE_SHAPE)
    i = np.arange(base.n)
    rewards = (base.ret * 0.5 + (i % 3)).astype(np.float32)
    dones = (i % 5 == 0).astype(np.float32)
    return base, (base.boards, base.actions, base.old, rewards, np.roll(base.boards, 1, axis=0), dones)


def flat_params(model, dtype):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).to(dtype)


@torch.no_grad()
def load_flat(model, flat):
    o = 0
    for p in model.parameters():
        p.copy_(flat[o:o + p.numel()].view(p.shape))
        o += p.numel()


@functools.lru_cache(maxsize=None)
def closed_update(dtype, seed=0):
    """update(epochs=UPDATE_EPOCHS) on the masked stock module in dtype: the advantage block with call indices 0 (boards) and 1
    (next boards), then per epoch the loss and gradients (indices 2, 3, ..) and clipping + Adam by tests/tpolicy_step_ref.py's
    restatement over the parameters (the eps slots are not parameters). Returns (returns, advantages, per epoch a dict of float64
    NumPy: losses, probs, value, grads, and after the step params, exp_avg, exp_avg_sq (the parameters' order, no eps slots), norm)."""
    import ppo_step_ref as S
    import ppo_update_ref as P
    base, (boards, actions, old, rewards, nxt, dones) = update_inputs()
    model = training_copy(base.model32, P4, dtype)
    v = masked_forward(model, P4, seed, 0, boards)[1]
    nv = masked_forward(model, P4, seed, 1, nxt)[1]
    returns, adv = P.advantage_lines(dtype, v, nv, rewards, dones, GAMMA)
    m = s = torch.zeros_like(flat_params(model, dtype))
    steps = []
    for e in range(UPDATE_EPOCHS):
        out = masked_loss_grad(model, P4, seed, 2 + e, boards, actions, old, adv.astype(np.float32), returns.astype(np.float32))
        g = torch.from_numpy(np.concatenate(out["grads"])).to(dtype)
        p, _, m, s, norm = S.adam_step_reference(flat_params(model, dtype), g, m, s, UPDATE_LR, e + 1, dtype=dtype)
        load_flat(model, p)
        steps.append(dict(out, params=p.numpy().astype(np.float64), exp_avg=m.numpy().astype(np.float64), exp_avg_sq=s.numpy().astype(np.float64),
                          norm=float(norm)))
    return returns, adv, steps
