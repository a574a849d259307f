"""What the CPU and the GPU tests of the PPO update's loss and gradient pass share: the stock modules (RefLayout of
tests/test_policy_host.py with dropout p = 0, in training mode, the BatchNorm affine parameters perturbed), the inputs' recipe,
the stock modules' own autograd through agents/ppo_agent.py:378-400 (the yardstick in float64, the tolerance's measure in
float32) and the conditions the inputs must meet for the comparison to mean something. Tensors are numbered actor first, then
critic, each in named_parameters() order, which is the plain layout's order.

The tolerance follows tests/qnet_grad_ref.py: per case and tensor max|got - f64| / max|f64| <= F32_FACTOR x the worst such ratio
of stock CPU float32 autograd over the case's 24 gradient tensors."""
import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F

from qnet_grad_ref import F32_FACTOR, ratios  # noqa: F401  (re-exported)
from test_policy_host import RefLayout

CLIP, VALUE_COEF, ENTROPY_COEF = 0.3, 0.4, 0.05          # PPOAgent's own settings
RELU_MARGIN = 1e-5
DISTINCT_ABOVE, DISTINCT = 300, 64                       # n > 300: 64 distinct boards repeated
F32_EPS = float(torch.finfo(torch.float32).eps)          # 2^-23: what Categorical clamps float32 probabilities to
GPU_SIZES = (1, 2, 3, 15, 16, 17, 127, 128, 129, 256, 257, 1025, 4095, 4096)
# the board seed per n: the first for which every ReLU input keeps RELU_MARGIN (find_seed; tests/test_ppo_update_host.py checks them)
SEEDS = {1: 0, 2: 0, 3: 0, 15: 1, 16: 0, 17: 0, 32: 0, 127: 6, 128: 135, 129: 16, 256: 3360, 257: 5031, 1025: 2, 4095: 28, 4096: 2}
WEIGHT_SEED = 23


def make_modules(seed=WEIGHT_SEED):
    """(actor, critic) float32 RefLayout modules in training mode, dropout p = 0, BatchNorm weight and bias perturbed."""
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        nets = RefLayout(4), RefLayout(1)
        gen = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for net in nets:
                net.dropout.p = 0.0
                for bn in (net.bn1, net.bn2):
                    bn.weight.copy_(1 + 0.3 * torch.randn(bn.num_features, generator=gen))
                    bn.bias.copy_(0.2 * torch.randn(bn.num_features, generator=gen))
                    bn.running_mean.copy_(0.3 * torch.randn(bn.num_features, generator=gen))
                    bn.running_var.copy_(torch.rand(bn.num_features, generator=gen) * 1.5 + 0.25)
                net.train()
    return nets


def states_of(n, seed):
    """float32 (n,16) observations codes / 15 of random boards; for n > 300 rows of 64 distinct boards, boards[i % 64]."""
    distinct = n if n <= DISTINCT_ABOVE else DISTINCT
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 12, size=(distinct, 16))
    codes[rng.random((distinct, 16)) < 0.35] = 0
    return (codes.astype(np.float32) / np.float32(15.0))[np.arange(n) % distinct]


def relu_inputs(net64, x64):
    """[z1, z2, z3]: the inputs of the three ReLUs of the float64 module's training-mode forward (running statistics untouched)."""
    out, h = [], x64
    with torch.no_grad():
        for fc, bn in ((net64.fc1, net64.bn1), (net64.fc2, net64.bn2), (net64.fc3, None)):
            z = fc(h)
            out.append(z)
            h = torch.relu(z)
            if bn is not None and h.shape[0] > 1:
                h = F.batch_norm(h, None, None, bn.weight, bn.bias, True, 0.1, bn.eps)
    return out


def relu_margin(nets64, x64):
    """min over both networks and the three layers of min|z| / max|z|."""
    return min(float(z.abs().min() / z.abs().max()) for net in nets64 for z in relu_inputs(net, x64))


def find_seed(n, nets64, start=0, limit=200000):
    for seed in range(start, start + limit):
        if relu_margin(nets64, torch.from_numpy(states_of(n, seed)).double()) >= RELU_MARGIN:
            return seed
    raise RuntimeError("no board seed in %d .. %d keeps the ReLU margin at n = %d" % (start, start + limit, n))


def categorical_parts(probs, actions, eps=None):
    """(log_prob(actions), entropy per row) of torch.distributions.Categorical(probs=probs); with eps, the same evaluated by hand
    with that clamp (float64 with float32's eps: the yardstick of a case in which the clamp binds)."""
    if eps is None:
        dist = torch.distributions.Categorical(probs=probs)
        return dist.log_prob(actions), dist.entropy()
    q = probs / probs.sum(-1, keepdim=True)
    logits = torch.log(torch.clamp(q, min=eps, max=1 - eps))
    return logits.gather(-1, actions.unsqueeze(-1)).squeeze(-1), -(logits * q).sum(-1)


def stock_update(nets, x, actions, old_log_probs, advantages, returns, calls=1, eps=None):
    """ppo_agent.py:378-400 up to backward() on deep copies of the stock modules in their own dtype, the forwards made `calls`
    times (the running statistics move each time; the gradients are the last call's). Everything as float64 NumPy: dict(losses
    (loss, actor_loss, value_loss, entropy), probs, values, grads [24], running [8], log_probs)."""
    actor, critic = (copy.deepcopy(net) for net in nets)
    dtype = actor.fc1.weight.dtype
    xs, a = torch.from_numpy(x).to(dtype), torch.from_numpy(actions)
    old, adv, ret = (torch.from_numpy(np.asarray(t)).to(dtype) for t in (old_log_probs, advantages, returns))
    for _ in range(calls):
        new_probs = actor(xs)
        new_log_probs, entropies = categorical_parts(new_probs, a, eps)
        entropy = entropies.mean()
        value_pred = critic(xs).squeeze()
        if value_pred.dim() == 0:
            value_pred = value_pred.unsqueeze(0)
        ratio = torch.exp(new_log_probs - old)
        clipped_ratio = torch.clamp(ratio, 1 - CLIP, 1 + CLIP)
        actor_loss = -torch.min(ratio * adv, clipped_ratio * adv).mean()
        value_loss = F.mse_loss(value_pred, ret)
        loss = actor_loss + VALUE_COEF * value_loss - ENTROPY_COEF * entropy
    loss.backward()
    f64 = lambda t: t.detach().numpy().astype(np.float64)       # noqa: E731
    # one row: the forward skips both BatchNorms, autograd leaves their .grad None; the device writes zeros
    grads = [f64(p.grad).reshape(-1) if p.grad is not None else np.zeros(p.numel()) for net in (actor, critic) for p in net.parameters()]
    running = [f64(t) for net in (actor, critic) for t in (net.bn1.running_mean, net.bn1.running_var, net.bn2.running_mean, net.bn2.running_var)]
    return dict(losses=np.array([float(t.detach()) for t in (loss, actor_loss, value_loss, entropy)]), probs=f64(new_probs),
                values=f64(value_pred), grads=grads, running=running, log_probs=f64(new_log_probs), ratio=f64(ratio))


def recipe(nets64, x, actions=None, eps=None):
    """(actions int64, old_log_probs, advantages, returns float32) of the rows of x: every action present, the ratios on both
    clip branches, advantages and returns that correlate with the input (input-independent periodic offsets make the critic's
    gradients cancel)."""
    n = len(x)
    i = np.arange(n, dtype=np.int64)
    if actions is None:
        actions = (5 * i + 1) % 4
    zero = np.zeros(n, dtype=np.float32)
    own = stock_update(nets64, x, actions, zero, zero, zero, eps=eps)
    old = own["log_probs"] + ((37 * i + 11) % 101 - 50) / 100.0
    adv = ((13 * i) % 17 - 8) / 4.0 + 2.0 * x[:, 0].astype(np.float64)
    ret = own["values"] + 0.5 + x.astype(np.float64).sum(1) / 8.0 + ((7 * i) % 11 - 5) / 5.0
    return actions, old.astype(np.float32), adv.astype(np.float32), ret.astype(np.float32)


class Case:
    """One n: the float32 and float64 modules, the inputs, the float64 yardstick, stock float32's own error and the bound."""

    def __init__(self, n, seed, nets32=None, x=None, actions=None, eps=None):
        self.n, self.seed = n, seed
        self.nets32 = nets32 if nets32 is not None else make_modules()
        self.nets64 = tuple(copy.deepcopy(net).double() for net in self.nets32)
        self.x = states_of(n, seed) if x is None else x
        self.actions, self.old, self.adv, self.ret = recipe(self.nets64, self.x, actions, eps)
        self.args = (self.x, self.actions, self.old, self.adv, self.ret)
        self.want = stock_update(self.nets64, *self.args, eps=eps)
        self.f32 = stock_update(self.nets32, *self.args)
        self.yardstick = float(ratios(self.f32["grads"], self.want["grads"]).max())
        self.bound = F32_FACTOR * self.yardstick

    def want_after(self, calls):
        return stock_update(self.nets64, *self.args, calls=calls)


@functools.lru_cache(maxsize=None)
def case(n):
    return Case(n, SEEDS[n])


CLAMP_N, CLAMP_ACTION, CLAMP_BIAS = 32, 2, -30.0


@functools.lru_cache(maxsize=None)
def clamp_case():
    """The case in which Categorical's clamp binds: the actor's fc4.bias puts one action's probability below 1e-9 on every row,
    and the even rows take that action (the odd rows action 1 or 3). float64 clamps at 2^-52, so the float64 yardstick is the
    by-hand Categorical with float32's eps; the old log-probs are around ITS log-probs (log(2^-23) on the even rows), so the
    ratios span both clip branches here too."""
    nets = make_modules()
    with torch.no_grad():
        nets[0].fc4.bias[CLAMP_ACTION] = CLAMP_BIAS
    i = np.arange(CLAMP_N, dtype=np.int64)
    actions = np.where(i % 2 == 0, CLAMP_ACTION, 1 + 2 * ((i // 2) % 2))
    return Case(CLAMP_N, SEEDS[CLAMP_N], nets32=nets, actions=actions, eps=F32_EPS)


def rel(got, want):
    """max|got - want| / max|want| of one tensor."""
    return float(ratios([got], [np.asarray(want, np.float64)])[0])
