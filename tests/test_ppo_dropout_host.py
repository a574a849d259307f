"""CPU-side checks of the PPO update's dropout (g2048_ppo_*_dropout, DevicePPOLearner(dropout=...)): the NumPy restatement of the
mask rule against the oracle's RNG, the masks' statistics, the threshold at the edges of p, the committed seed tables, the masked
stock modules against stock torch with F.dropout replaced by the same mask, the C-ABI's argument validation and the learner's
`dropout` argument. The kernels themselves are checked on the GPU (tests/test_gpu_ppo_dropout.py)."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import ppo_dropout_ref as D
import ppo_update_ref as R
from oracle import oracle as O
from test_policy_host import RefLayout

CALLS = (0, 7, (1 << 32) + 5)


def test_restatement_is_the_specified_rule():
    """rng_keys and rng_draw of the helper equal the oracle's with domain 11 on ids of both networks and both sites at three call
    indices (one above 2^32), low words from the first rows, the last row of the largest batch and random ones."""
    rng = np.random.default_rng(5)
    checked = 0
    for c in CALLS:
        keys = D.rng_keys(D.DROPOUT_SEED, D.DOMAIN, c)
        assert keys == O.rng_keys(D.DROPOUT_SEED, 11, c)
        for w in (0, 1):
            for s in (0, 1):
                F = D.WIDTH[s]
                lo = np.concatenate([np.arange(8), [F - 1, F, 4095 * F, 4096 * F - 1], rng.integers(0, 4096 * F, 16)]).astype(np.uint32)
                got = D.rng_draws(keys[0], keys[1], 2 * w + s, lo)
                want = [O.rng_draw(keys[0], keys[1], ((2 * w + s) << 32) | int(i), 0) for i in lo]
                assert got.tolist() == want, (c, w, s)
                checked += len(lo)
    assert checked >= 300


def masks_at(p, n, call=0):
    return {(w, s): D.keep_mask(D.DROPOUT_SEED, call, w, s, p, n) for w in (0, 1) for s in (0, 1)}


def test_dropped_share():
    """p = 0.2, n = 4,096: the dropped share of each (network, site) mask within 5 binomial standard deviations of T / 2^32."""
    q = D.threshold(0.2) / 2.0 ** 32
    for (w, s), keep in masks_at(0.2, 4096).items():
        sd = math.sqrt(q * (1 - q) / keep.size)
        share = 1.0 - keep.mean()
        print("network %d site %d: dropped share %.5f (T / 2^32 = %.5f, 5 sd = %.5f)" % (w, s, share, q, 5 * sd))
        assert abs(share - q) <= 5 * sd


def test_masks_of_different_network_site_or_call_are_independent():
    """Two masks agree on a share within 5 standard deviations of p^2 + (1 - p)^2 (the smaller site's element count)."""
    p, n = 0.2, 4096
    q = D.threshold(p) / 2.0 ** 32
    agree = q * q + (1 - q) * (1 - q)
    a, b = masks_at(p, n, 0), masks_at(p, n, 1)
    pairs = [("network", a[0, 0], a[1, 0]), ("network, site 1", a[0, 1], a[1, 1]), ("site", a[0, 0][:, :128], a[0, 1]),
             ("call index", a[0, 0], b[0, 0]), ("call index, critic site 1", a[1, 1], b[1, 1])]
    far = D.keep_mask(D.DROPOUT_SEED, 1 << 32, 0, 0, p, n)
    pairs.append(("call index 2^32 against 0", a[0, 0], far))
    other = D.keep_mask(D.DROPOUT_SEED + 1, 0, 0, 0, p, n)
    pairs.append(("seed", a[0, 0], other))
    for what, x, y in pairs:
        sd = math.sqrt(agree * (1 - agree) / x.size)
        share = float((x == y).mean())
        print("%s: agreement %.5f (expected %.5f, 5 sd = %.5f)" % (what, share, agree, 5 * sd))
        assert abs(share - agree) <= 5 * sd, what


def test_threshold_at_the_edges():
    assert D.threshold(0.0) == 0 and D.keep_mask(D.DROPOUT_SEED, 0, 0, 0, 0.0, 64).all() and D.scale32(0.0) == 1.0 and D.scale64(0.0) == 1.0
    assert D.threshold(1e-12) == 0 and D.keep_mask(D.DROPOUT_SEED, 0, 1, 1, 1e-12, 64).all() and D.scale32(1e-12) == np.float32(1.0)
    top = 1.0 - 2.0 ** -33
    assert top < 1.0 and D.threshold(top) == 2 ** 32 - 1
    assert D.threshold(0.2) == 858993459 and D.threshold(0.5) == 2 ** 31
    assert D.scale32(0.2) == np.float32(1.25) and D.scale32(0.5) == np.float32(2.0)


@pytest.mark.parametrize("key", sorted(D.SEEDS, key=str), ids=str)
def test_seed_table_meets_the_margin(key):
    """Per case of the GPU test: the committed board seed keeps every ReLU input of the MASKED float64 modules at RELU_MARGIN (the
    three seeds before it, where there are any, do not: it is the scan's), and stock float32's own error is a fair float32's."""
    n, p = key
    nets64 = tuple(copy.deepcopy(net).double() for net in R.make_modules())
    seed = D.SEEDS[key]
    margin = D.relu_margin_masked(nets64, D.states_of(n, seed), p, 0)
    c = D.case(n, p)
    print("n = %d, p = %r: seed %d, masked ReLU margin %.3g, float32 yardstick %.3g" % (n, p, seed, margin, c.yardstick))
    assert margin >= R.RELU_MARGIN
    assert D.find_seed(n, p, nets64, start=max(0, seed - 3), limit=4) == seed
    # BatchNorm over two or three rows divides by a variance near eps, more so with a quarter of its inputs zeroed: float32's own
    # error is larger there. A mask, scale or index error moves a gradient by tenths of its maximum, far above 8 x either limit
    assert 0 < c.yardstick <= (1e-3 if n in (2, 3) else 1e-5)
    assert np.isfinite(c.want["losses"]).all() and all(np.isfinite(g).all() for g in c.want["grads"])
    if p != 1e-12:                      # the masks reach the function: it is not the one without dropout
        plain = R.stock_update(c.plain64, *c.args)
        assert R.ratios(plain["grads"], c.want["grads"]).max() > 1e-2


def test_loop_seed_meets_the_margin_in_every_epoch():
    c = D.loop_case()
    print("closed loop: seed %d, margins %s, yardstick %.3g" % (c.seed, " ".join("%.3g" % m for m in c.want["margins"]), c.yardstick))
    assert len(c.want["margins"]) == 2 + 2 * R.LOOP_EPOCHS and min(c.want["margins"]) >= R.RELU_MARGIN
    assert D.find_loop_seed(c.nets64, start=max(0, c.seed - 2), limit=3) == c.seed
    assert 0 < c.yardstick <= 1e-5
    assert c.want["tracked"] == [3, 3, 5, 5]


def test_large_sizes_have_relu_inputs_near_zero():
    """Why the GPU test compares no gradients at n = 1,025 and 4,096: the committed count of ReLU inputs within RELU_MARGIN of zero
    is not 0 there (a float32 rounding can flip such a ReLU, and one flip moves a gradient by far more than the bound)."""
    nets64 = tuple(copy.deepcopy(net).double() for net in R.make_modules())
    for n in D.LARGE_SIZES:
        count = D.near_zero_count(nets64, D.states_of(n, D.LARGE_SEED), D.P, 0)
        print("n = %d: %d ReLU inputs within %.0e of zero" % (n, count, R.RELU_MARGIN))
        assert count == D.LARGE_NEAR_ZERO[n] and count > 0


@pytest.mark.parametrize("p", [0.2, 0.5, (0.1, 0.3)], ids=str)
def test_masked_modules_are_stock_modules_under_the_same_mask(p, monkeypatch):
    """The masked modules equal the stock modules (nn.Dropout live, training mode) with F.dropout replaced by torch's own formula on
    the restated keep bits, input * (keep / (1 - p)): losses, outputs, all 24 gradients and the running statistics bit for bit in
    float32. So the float scale the library uses, float32(1 / (1 - p)), is the one torch's division gives."""
    n = 17
    c = D.case(n, p)
    state = dict(w=0)

    def same_mask_dropout(x, p=0.5, training=True, inplace=False):
        assert training and not inplace
        keep = D.keep_mask(D.DROPOUT_SEED, 0, state["w"], D.WIDTH.index(x.shape[1]), p, x.shape[0])
        return x * torch.from_numpy(keep).to(x.dtype).div_(1 - p)

    class Stock(RefLayout):
        def forward(self, x):
            state["w"] = self.w
            return super().forward(x)

    stock = []
    for w, (net, pw) in enumerate(zip(c.nets32, D.pair(p))):
        m = copy.deepcopy(net)
        m.__class__, m.w, m.dropout = Stock, w, nn.Dropout(pw)
        stock.append(m.train())
    monkeypatch.setattr(torch.nn.functional, "dropout", same_mask_dropout)
    got = R.stock_update(tuple(stock), *c.args)
    want = R.stock_update(D.masked_modules(c.nets32, p, [0]), *c.args)
    for key in ("losses", "probs", "values"):
        assert np.array_equal(got[key], want[key]), key
    for k, (a, b) in enumerate(zip(got["grads"] + got["running"], want["grads"] + want["running"])):
        assert np.array_equal(a, b), k


def test_dropout_entry_points_validate_without_device():
    """The three new entry points reject a bad p, net or site and null and misaligned pointers before any device call (status -1, a
    message that names them); n == 0 is G2048_OK. The existing entry points' checks are tests/test_ppo_update_host.py's."""
    from g2048 import _lib
    L = _lib.lib()
    buf = (C.c_uint8 * 4096)()
    base = (C.addressof(buf) + 15) & ~15
    f, d = C.c_float, C.c_double
    bad_p = (-0.1, 1.0, 1.5, float("nan"), float("inf"), -float("inf"))

    def fwd(states=base, plain=base, running=None, n_out=4, net=0, p=0.2, out=base, n=8, workspace=base):
        return L.g2048_ppo_forward_train_dropout(states, plain, running, n_out, net, d(p), 1, 2, out, n, workspace, None)
    assert fwd(n=0) == 0 and fwd(n=0, p=2.0) == 0
    for name in ("states", "plain", "out", "workspace"):
        assert fwd(**{name: None}) == -1 and b"g2048_ppo_forward_train_dropout: null pointer" in L.g2048_last_error(), name
        assert fwd(**{name: base + 4}) == -1 and b"misaligned" in L.g2048_last_error(), name
    assert fwd(running=base + 2) == -1 and b"misaligned" in L.g2048_last_error()
    for n_out in (0, 2, 5):
        assert fwd(n_out=n_out) == -1 and b"n_out must be 4 (actor) or 1 (critic)" in L.g2048_last_error()
    for net in (-1, 2):
        assert fwd(net=net) == -1 and b"g2048_ppo_forward_train_dropout: net must be 0" in L.g2048_last_error()
    for p in bad_p:
        assert fwd(p=p) == -1 and b"0 <= p < 1" in L.g2048_last_error(), p
    assert fwd(n=4097) == -1 and b"G2048_PPO_BATCH_MAX" in L.g2048_last_error()

    order = ("states", "actions", "old_log_probs", "advantages", "returns", "plain_actor", "plain_critic", "running_actor", "running_critic")
    tail = ("grad_actor", "grad_critic", "loss_out", "workspace")

    def lg(n=8, pa=0.2, pc=0.2, clip=0.3, **kw):
        ptr = {k: base for k in order + tail}
        ptr["running_actor"] = ptr["running_critic"] = None
        ptr.update(kw)
        return L.g2048_ppo_loss_grad_dropout(*[ptr[k] for k in order], f(clip), f(0.4), f(0.05), d(pa), d(pc), 1, 2, n, *[ptr[k] for k in tail], None)
    assert lg(n=0) == 0
    for name in order[:7] + tail:
        assert lg(**{name: None}) == -1 and b"g2048_ppo_loss_grad_dropout: null pointer" in L.g2048_last_error(), name
    for name in ("states", "plain_actor", "plain_critic", "grad_actor", "grad_critic", "workspace", "actions"):
        assert lg(**{name: base + 4}) == -1 and b"misaligned" in L.g2048_last_error(), name
    for name in ("old_log_probs", "advantages", "returns", "running_actor", "running_critic", "loss_out"):
        assert lg(**{name: base + 2}) == -1 and b"misaligned" in L.g2048_last_error(), name
    for p in bad_p:
        assert lg(pa=p) == -1 and b"0 <= p < 1" in L.g2048_last_error(), p
        assert lg(pc=p) == -1 and b"g2048_ppo_loss_grad_dropout" in L.g2048_last_error(), p
    assert lg(clip=-0.1) == -1 and b"finite and not negative" in L.g2048_last_error()
    assert lg(n=4097) == -1 and b"not truncated" in L.g2048_last_error()

    def mask(net=0, site=0, p=0.2, keep=base, n=8):
        return L.g2048_ppo_dropout_mask(1, 2, net, site, d(p), keep, n, None)
    assert mask(n=0) == 0
    assert mask(keep=None) == -1 and b"g2048_ppo_dropout_mask: null pointer" in L.g2048_last_error()
    for kw in (dict(net=2), dict(net=-1), dict(site=2), dict(site=-1)):
        assert mask(**kw) == -1 and b"net must be 0" in L.g2048_last_error(), kw
    for p in bad_p:
        assert mask(p=p) == -1 and b"0 <= p < 1" in L.g2048_last_error(), p
    assert mask(n=4097) == -1 and b"G2048_PPO_BATCH_MAX" in L.g2048_last_error()


def test_learner_dropout_argument():
    """DevicePPOLearner's `dropout`: a probability, an (actor, critic) pair, or "module" for each module's own nn.Dropout; refusals are
    ValueErrors that name the class, raised before any device is needed."""
    from g2048 import ops
    from g2048.ppo import dropout_of
    actor, critic = RefLayout(4), RefLayout(1)
    assert dropout_of(actor, critic, 0.0) == (0.0, 0.0) and dropout_of(actor, critic, 0.25) == (0.25, 0.25)
    assert dropout_of(actor, critic, (0.1, 0.3)) == (0.1, 0.3)
    assert dropout_of(actor, critic, "module") == (0.2, 0.2)
    critic.dropout = nn.Dropout(0.35)
    assert dropout_of(actor, critic, "module") == (0.2, 0.35)
    bare = nn.Sequential(nn.Linear(16, 4))
    with pytest.raises(ValueError, match="DevicePPOLearner.*nn.Dropout"):
        dropout_of(actor, bare, "module")
    critic.dropout = nn.Identity()
    with pytest.raises(ValueError, match="nn.Dropout"):
        dropout_of(actor, critic, "module")
    with pytest.raises(ValueError, match="DevicePPOLearner.*\"module\""):
        dropout_of(actor, critic, "modules")
    for bad in (1.0, -0.1, float("nan"), (0.2, 1.0)):
        with pytest.raises(ValueError, match="DevicePPOLearner.*0 <= p < 1"):
            dropout_of(actor, critic, bad)
    with pytest.raises(ValueError, match="pair"):
        dropout_of(actor, critic, (0.1, 0.2, 0.3))
    assert ops.ppo_dropout_p(0.2) == 0.2
    with pytest.raises(ValueError, match="site"):
        ops.ppo_dropout_mask(4, 0, 2, 0.2)
    for n in (4097, -1):
        with pytest.raises(ValueError, match="0 .. 4096 rows"):
            ops.ppo_dropout_mask(n, 0, 0, 0.2)
