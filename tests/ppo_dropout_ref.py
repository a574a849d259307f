"""What the CPU and the GPU tests of the PPO update's dropout share (tests/test_ppo_dropout_host.py, tests/test_gpu_ppo_dropout.py).

The mask rule, restated in NumPy uint32 from its specification (include/g2048.h, "Dropout"), not imported from the library: for the
library call with index c, (k0, k1) = rng_keys(seed, 11, c); element (row, feature) of site s (0 after bn1, F = 256; 1 after bn2,
F = 128) of network w (0 actor, 1 critic) draws h = rng_draw(k0, k1, ((2 w + s) << 32) | (row F + feature), 0) and is kept iff
h >= T = floor(p 2^32); a kept element is multiplied by 1 / (1 - p), a dropped one by 0.

The stock modules with those masks: MaskedLayout is RefLayout (tests/test_policy_host.py) whose two nn.Dropout calls are the explicit
products h * keep * scale, the masks those of the call indices the module is given, one per forward. masked_modules() makes them
from ppo_update_ref.make_modules(), so ppo_update_ref.stock_update / stock_loop run on them unchanged: float64 with scale =
1 / (1 - p) in double is the yardstick, float32 with the float scale on stock CPU torch the measure. The tolerance is
ppo_update_ref.Case's: per tensor max|got - f64| / max|f64| <= F32_FACTOR x the float32 run's worst such ratio over the 24 gradient
tensors. The inputs' condition is ppo_update_ref's too, relu_margin >= RELU_MARGIN, evaluated WITH the masks applied (they decide
what fc2 and fc3 see). The dropout seed is fixed; the board seed per case is the first that find_seed accepts (SEEDS, LOOP_SEED;
tests/test_ppo_dropout_host.py re-checks the tables)."""
import copy
import functools
import math

import numpy as np
import torch

import ppo_update_ref as R
from test_policy_host import RefLayout

DOMAIN = 11
DROPOUT_SEED = 0x2048D0
WIDTH = (256, 128)                                       # features of site 0 and site 1
M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------------ the mask rule --
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def rng_keys(seed, domain, index):
    a = splitmix64((seed ^ (domain * 0xD1B54A32D192ED03)) & M64)
    b = splitmix64(a ^ splitmix64((index + 0x2048204820482048) & M64))
    return b & 0xFFFFFFFF, b >> 32


def rng_draws(k0, k1, hi, lo, ctr=0):
    """rng_draw(k0, k1, (hi << 32) | lo, ctr) for a uint32 array lo."""
    u = np.uint32
    with np.errstate(over="ignore"):
        h = np.asarray(lo, dtype=u) ^ u(k0)
        h ^= h >> u(16); h *= u(0x85EBCA6B); h ^= h >> u(13); h *= u(0xC2B2AE35); h ^= h >> u(16)        # noqa: E702
        h += u((k1 + hi * 0x9E3779B1 + ctr * 0x85EBCA77) & 0xFFFFFFFF)
        h ^= h >> u(16); h *= u(0x7FEB352D); h ^= h >> u(15); h *= u(0x846CA68B); h ^= h >> u(16)        # noqa: E702
    return h


def threshold(p):
    """T = floor(p 2^32), formed in double; below 2^32 because p < 1."""
    return int(math.floor(float(p) * 4294967296.0))


def scale64(p):
    return 1.0 / (1.0 - float(p))


def scale32(p):
    return np.float32(scale64(p))


@functools.lru_cache(maxsize=256)
def keep_mask(seed, call_index, net, site, p, n):
    """bool (n, F): which elements of site `site` of network `net` the call keeps."""
    k0, k1 = rng_keys(seed, DOMAIN, call_index)
    F = WIDTH[site]
    keep = rng_draws(k0, k1, 2 * net + site, np.arange(n * F, dtype=np.uint32)) >= np.uint32(threshold(p))
    return keep.reshape(n, F)


def pair(p):
    return (float(p[0]), float(p[1])) if isinstance(p, (tuple, list)) else (float(p), float(p))


# ------------------------------------------------------------------------------------------ the stock modules, masked --
MARGINS = []                 # every MaskedLayout forward with `record` set appends its ReLU margin (the run's own weights)


class MaskedLayout(RefLayout):
    """RefLayout with its dropout written out: forward k multiplies by the masks of call index self.indices[k]. Made by
    masked_modules(); the attributes are plain Python, so parameters(), state_dict() and deepcopy are RefLayout's."""

    def multipliers(self, n, dtype):
        index = self.indices[self.calls]
        self.calls += 1
        scale = scale64(self.p) if dtype == torch.float64 else float(scale32(self.p))
        return [torch.from_numpy(keep_mask(self.seed, index, self.w, s, self.p, n)).to(dtype) * scale for s in (0, 1)]

    def forward(self, x):
        single = x.dim() == 1
        if single:
            x = x.unsqueeze(0)
        m1, m2 = self.multipliers(x.shape[0], x.dtype)
        z1 = self.fc1(x)
        x = self.relu(z1)
        if x.shape[0] > 1:
            x = self.bn1(x)
        z2 = self.fc2(x * m1)
        x = self.relu(z2)
        if x.shape[0] > 1:
            x = self.bn2(x)
        z3 = self.fc3(x * m2)
        x = self.fc4(self.relu(z3))
        if self.record:
            MARGINS.append(min(float(z.detach().abs().min() / z.detach().abs().max()) for z in (z1, z2, z3)))
        if self.softmax is not None:
            x = self.softmax(x)
        return x.squeeze(0) if single else x


def masked_modules(nets, p, indices, seed=DROPOUT_SEED, record=False):
    """Deep copies of (actor, critic) as MaskedLayout: p a probability or an (actor, critic) pair; indices = (the actor's call
    indices, the critic's), one per forward each will make, or one list for both."""
    if not isinstance(indices[0], (tuple, list)):
        indices = (indices, indices)
    out = []
    for w, (net, pw, idx) in enumerate(zip(nets, pair(p), indices)):
        m = copy.deepcopy(net)
        m.__class__ = MaskedLayout
        m.p, m.w, m.seed, m.indices, m.calls, m.record = pw, w, seed, tuple(idx), 0, record
        out.append(m)
    return tuple(out)


def masked_forward(nets, x, p, index, seed=DROPOUT_SEED):
    """(probs, values, ReLU margin) of one training-mode forward of both modules with the masks of call `index`; the modules'
    running statistics are left alone (deep copies)."""
    actor, critic = masked_modules(nets, p, [index], seed, record=True)
    del MARGINS[:]
    xs = torch.from_numpy(np.asarray(x)).to(actor.fc1.weight.dtype)
    with torch.no_grad():
        probs, values = actor(xs), critic(xs)
    return probs.numpy().astype(np.float64), values.numpy().astype(np.float64).reshape(-1), min(MARGINS)


def relu_margin_masked(nets64, x, p, index, seed=DROPOUT_SEED):
    return masked_forward(nets64, x, p, index, seed)[2]


def near_zero_count(nets64, x, p, index, seed=DROPOUT_SEED):
    """How many ReLU inputs of the masked float64 forward of both modules lie within RELU_MARGIN of zero, relative to their layer's
    largest: the rows on which a float32 rounding can flip a ReLU."""
    count = 0
    for net in masked_modules(nets64, p, [index], seed):
        xs = torch.from_numpy(np.asarray(x)).double()
        m1, m2 = net.multipliers(len(x), torch.float64)
        with torch.no_grad():
            z1 = net.fc1(xs)
            h = torch.relu(z1)
            z2 = net.fc2((torch.nn.functional.batch_norm(h, None, None, net.bn1.weight, net.bn1.bias, True, 0.1, net.bn1.eps) if len(x) > 1 else h) * m1)
            h = torch.relu(z2)
            z3 = net.fc3((torch.nn.functional.batch_norm(h, None, None, net.bn2.weight, net.bn2.bias, True, 0.1, net.bn2.eps) if len(x) > 1 else h) * m2)
        count += sum(int((z.abs() < R.RELU_MARGIN * z.abs().max()).sum()) for z in (z1, z2, z3))
    return count


def states_of(n, seed):
    """ppo_update_ref.states_of without its repetition above 300 rows: with dropout every row is distinct after the first site."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 12, size=(n, 16))
    codes[rng.random((n, 16)) < 0.35] = 0
    return codes.astype(np.float32) / np.float32(15.0)


def find_seed(n, p, nets64=None, index=0, start=0, limit=200000):
    """The first board seed at which every ReLU input of both masked float64 modules keeps RELU_MARGIN."""
    nets64 = nets64 or tuple(copy.deepcopy(net).double() for net in R.make_modules())
    for seed in range(start, start + limit):
        if relu_margin_masked(nets64, states_of(n, seed), p, index) >= R.RELU_MARGIN:
            return seed
    raise RuntimeError("no board seed in %d .. %d keeps the ReLU margin at n = %d, p = %r" % (start, start + limit, n, p))


P = 0.2                                                  # the reference's nn.Dropout(0.2)
GRAD_SIZES = (1, 2, 3, 16, 17, 33, 129, 225, 257)        # every edge of the touched kernels (tests/test_gpu_ppo_dropout.py)
EXTRA_P = (0.5, (0.1, 0.3), 1e-12)                       # at n = 17
LARGE_SIZES = (1025, 4096)                               # no gradient comparison: LARGE_NEAR_ZERO
# (n, p) -> board seed, call index 0: find_seed's first (tests/test_ppo_dropout_host.py re-checks the margin)
SEEDS = {(1, 0.2): 0, (2, 0.2): 0, (3, 0.2): 0, (16, 0.2): 0, (17, 0.2): 0, (33, 0.2): 1, (129, 0.2): 3, (225, 0.2): 3553, (257, 0.2): 40055,
         (17, 0.5): 0, (17, (0.1, 0.3)): 1, (17, 1e-12): 0}
# near_zero_count at the large sizes with board seed LARGE_SEED: ReLU inputs a float32 rounding can flip, so no gradient bound holds
LARGE_SEED = 0
LARGE_NEAR_ZERO = {1025: 43, 4096: 162}


class Case:
    """ppo_update_ref.Case with the masks of one call: the float32 and float64 masked modules, the inputs, the float64 yardstick,
    stock float32's own error and the bound."""

    def __init__(self, n, p, seed, index=0):
        self.n, self.p, self.seed, self.index = n, p, seed, index
        self.coefs = (R.CLIP, R.VALUE_COEF, R.ENTROPY_COEF)
        self.nets32 = R.make_modules()
        self.plain64 = tuple(copy.deepcopy(net).double() for net in self.nets32)
        self.masked32 = masked_modules(self.nets32, p, [index])
        self.masked64 = masked_modules(self.plain64, p, [index])
        self.x = states_of(n, seed)
        self.actions, self.old, self.adv, self.ret = R.recipe(self.masked64, self.x)
        self.args = (self.x, self.actions, self.old, self.adv, self.ret)
        self.want = R.stock_update(self.masked64, *self.args)
        self.f32 = R.stock_update(self.masked32, *self.args)
        self.yardstick = float(R.ratios(self.f32["grads"], self.want["grads"]).max())
        self.bound = R.F32_FACTOR * self.yardstick


@functools.lru_cache(maxsize=None)
def case(n, p=P):
    return Case(n, p, SEEDS[(n, p)])


class LargeCase(Case):
    """A size at which no board seed keeps the ReLU margin (LARGE_NEAR_ZERO): the gradients are no yardstick there. The yardstick
    is the float32 masked modules' worst error on what is continuous in the ReLU inputs (probabilities, values, loss parts, running
    statistics), at least the 8 float32 roundings of ppo_update_ref.ADV_FLOOR."""

    def __init__(self, n):
        super().__init__(n, P, LARGE_SEED)
        cont = lambda r: [r["probs"], r["values"], r["losses"]] + r["running"]      # noqa: E731
        self.yardstick = max(float(R.ratios(cont(self.f32), cont(self.want)).max()), R.ADV_FLOOR)
        self.bound = R.F32_FACTOR * self.yardstick


@functools.lru_cache(maxsize=None)
def large_case(n):
    return LargeCase(n)


# ---------------------------------------------------------------------------------------------------- a whole update --
LOOP_ADV_INDICES, LOOP_EPOCH_INDICES = (0, 1), (2, 3, 4)        # update(epochs=3) from dropout_index 0
LOOP_SEED = 165                                                  # the first seed find_loop_seed accepts


def stock_loop_masked(nets, inputs, actions, old, p=P, record=False):
    """ppo_update_ref.stock_loop on the masked modules: the critic's two forwards of the advantages block draw call indices 0 and
    1, the epochs 2, 3, 4 for both networks. With record, also 'margins': every forward's ReLU margin under the run's weights."""
    masked = masked_modules(nets, p, (LOOP_EPOCH_INDICES, LOOP_ADV_INDICES + LOOP_EPOCH_INDICES), record=record)
    del MARGINS[:]
    out = R.stock_loop(masked, inputs, actions, old)
    out["margins"] = list(MARGINS)
    return out


def loop_recipe(nets64, x, p=P):
    return R.recipe(masked_modules(nets64, p, [LOOP_EPOCH_INDICES[0]]), x)[:2]


def loop_margins_hold(nets64, seed, p=P):
    inputs = R.loop_inputs(seed)
    actions, old = loop_recipe(nets64, inputs[0], p)
    margins = stock_loop_masked(nets64, inputs, actions, old, p, record=True)["margins"]
    return len(margins) == 2 + 2 * R.LOOP_EPOCHS and min(margins) >= R.RELU_MARGIN


def find_loop_seed(nets64=None, start=0, limit=20000):
    nets64 = nets64 or tuple(copy.deepcopy(net).double() for net in R.make_modules())
    for seed in range(start, start + limit):
        if loop_margins_hold(nets64, seed):
            return seed
    raise RuntimeError("no board seed in %d .. %d keeps the ReLU margin through the masked epochs" % (start, start + limit))


class LoopCase:
    """ppo_update_ref.LoopCase with dropout p = 0.2 in both networks."""

    def __init__(self, seed):
        self.seed = seed
        self.nets32 = R.make_modules()
        self.nets64 = tuple(copy.deepcopy(net).double() for net in self.nets32)
        self.inputs = R.loop_inputs(seed)
        self.x = self.inputs[0]
        self.actions, self.old = loop_recipe(self.nets64, self.x)
        self.want = stock_loop_masked(self.nets64, self.inputs, self.actions, self.old, record=True)
        self.f32 = stock_loop_masked(self.nets32, self.inputs, self.actions, self.old)
        self.yardstick = float(R.ratios(self.f32["epochs"][0]["grads"], self.want["epochs"][0]["grads"]).max())
        self.bound = R.F32_FACTOR * self.yardstick
        self.adv_bound = R.advantage_bound((self.f32["adv"]["returns"], self.f32["adv"]["advantages"]),
                                           (self.want["adv"]["returns"], self.want["adv"]["advantages"]))


@functools.lru_cache(maxsize=None)
def loop_case():
    return LoopCase(LOOP_SEED)


if __name__ == "__main__":               # the scans that made SEEDS, LOOP_SEED and LARGE_NEAR_ZERO
    for key in [(n, P) for n in GRAD_SIZES] + [(17, p) for p in EXTRA_P]:
        print("SEEDS[%r] = %d" % (key, find_seed(*key)), flush=True)
    print("LOOP_SEED = %d" % find_loop_seed(), flush=True)
    nets64 = tuple(copy.deepcopy(net).double() for net in R.make_modules())
    for n in LARGE_SIZES:
        print("LARGE_NEAR_ZERO[%d] = %d" % (n, near_zero_count(nets64, states_of(n, LARGE_SEED), P, 0)), flush=True)
