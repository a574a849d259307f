"""CPU-side checks of the PPO update's loss and gradient pass (g2048.DevicePPOLearner, g2048_ppo_loss_grad): the conditions on the
inputs of tests/test_gpu_ppo_update.py and tests/test_gpu_ppo_update_edges.py that keep them from being vacuous or flaky (each edge
case is in the regime it claims: poisoned, saturated, other coefficients, dead features, a whole update), the by-hand Categorical of the clamp case
against torch's own, the fixture of the reference's own classes, the plain layout's offsets, the converter's refusals and the
C-ABI's argument validation. The kernels themselves are checked on the GPU."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

import ppo_update_ref as R
from conftest import load_golden
from test_policy_host import RefLayout, bench_trunk_net


def clipped_share(c):
    """The share of rows on which min(..) takes the clipped branch, from the float64 modules."""
    r, a = c.want["ratio"], c.adv.astype(np.float64)
    return float(np.mean(np.clip(r, 1 - R.CLIP, 1 + R.CLIP) * a < r * a))


@pytest.mark.parametrize("n", R.GPU_SIZES + (R.CLAMP_N,))
def test_case_inputs_meet_the_conditions_of_the_gpu_test(n):
    """Per case: every ReLU input of the float64 modules keeps |z| >= 1e-5 max|z| of its layer (one rounding-flipped mask moves a
    gradient by a percent at large n), stock float32's own error is a fair float32's, no probability is near the clamp and no
    ratio within 1e-3 of a clip edge."""
    c = R.case(n)
    x64 = torch.from_numpy(c.x).double()
    margin = R.relu_margin(c.nets64, x64)
    print("n = %d: seed %d, ReLU margin %.3g, float32 yardstick %.3g, probabilities %.3g .. %.3g, clipped share %.3f"
          % (n, c.seed, margin, c.yardstick, c.want["probs"].min(), c.want["probs"].max(), clipped_share(c)))
    assert margin >= R.RELU_MARGIN
    if n > R.DISTINCT_ABOVE:
        assert len(np.unique(c.x, axis=0)) == R.DISTINCT and np.array_equal(c.x[R.DISTINCT:2 * R.DISTINCT], c.x[:R.DISTINCT])
    else:
        assert len(np.unique(c.x, axis=0)) == n
    if n >= 16:
        assert 0 < c.yardstick <= 1e-5
    elif n in (2, 3):
        assert 0 < c.yardstick <= 1e-4          # BatchNorm over two or three rows divides by a variance near eps
    else:
        assert 0 < c.yardstick <= 1e-5          # n = 1 (no BatchNorm) and 15
    p, r = c.want["probs"], c.want["ratio"]
    assert p.min() >= 1e-3 and p.max() <= 1 - 1e-3
    assert min(np.abs(r - (1 - R.CLIP)).min(), np.abs(r - (1 + R.CLIP)).min()) >= 1e-3
    assert np.isfinite(c.want["losses"]).all() and all(np.isfinite(g).all() for g in c.want["grads"])
    if n >= 15:
        assert set(c.actions.tolist()) == {0, 1, 2, 3}
        assert (r < 1 - R.CLIP).any() and (r > 1 + R.CLIP).any()
    if n >= 127:                                # min(..) takes both branches (at n = 15 .. 17 the recipe's signs leave the clipped one out)
        assert 0.1 < clipped_share(c) < 0.3
    if n == 1:
        assert all(not g.any() for k, g in enumerate(c.want["grads"]) if k % 12 in (2, 3, 6, 7))         # the BatchNorms are skipped


def test_recipe_is_the_issues():
    c = R.case(17)
    i = np.arange(17)
    assert np.array_equal(c.actions, (5 * i + 1) % 4)
    own = R.stock_update(c.nets64, c.x, c.actions, c.old, c.adv, c.ret)
    assert np.allclose(own["log_probs"] - c.old, -((37 * i + 11) % 101 - 50) / 100.0, atol=1e-6)
    assert np.allclose(c.adv, ((13 * i) % 17 - 8) / 4.0 + 2 * c.x[:, 0], atol=1e-6)
    assert np.allclose(c.ret, own["values"] + 0.5 + c.x.sum(1) / 8.0 + ((7 * i) % 11 - 5) / 5.0, atol=1e-5)
    for net in c.nets32:
        assert net.training and net.dropout.p == 0.0 and not torch.equal(net.bn1.weight, torch.ones(256))


def test_by_hand_categorical_is_torchs_in_float32_and_the_clamp_case_binds():
    """The clamp case's float64 yardstick evaluates Categorical by hand with float32's eps. In float32 that evaluation must BE
    torch's: the same loss and gradients bit for bit, with the clamp binding on the suppressed action."""
    c = R.clamp_case()
    assert c.f32["probs"][:, R.CLAMP_ACTION].max() < 1e-9
    assert (c.actions[0::2] == R.CLAMP_ACTION).all() and (c.actions[1::2] != R.CLAMP_ACTION).all()
    hand = R.stock_update(c.nets32, *c.args, eps=R.F32_EPS)
    assert np.array_equal(hand["losses"], c.f32["losses"])
    for a, b in zip(hand["grads"], c.f32["grads"]):
        assert np.array_equal(a, b)
    assert np.allclose(c.f32["log_probs"][0::2], np.log(R.F32_EPS), rtol=1e-6)
    print("clamp case: float32 yardstick %.3g" % c.yardstick)
    assert 0 < c.yardstick <= 1e-5
    r = c.want["ratio"]
    assert (r < 1 - R.CLIP).any() and (r > 1 + R.CLIP).any() and np.isfinite(c.want["losses"]).all()


def golden_modules(g, dtype):
    nets = RefLayout(4), RefLayout(1)
    for net, prefix in zip(nets, ("actor.", "critic.")):
        sd = {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}
        net.load_state_dict(sd, strict=False)
        net.dropout.p = 0.0
        net.to(dtype).train()
    return nets


def test_stock_modules_reproduce_the_reference_classes_fixture():
    """tests/golden/ppo_update.npz holds the gradients of the reference's OWN ActorNetwork / CriticNetwork (float64, stored as
    float32) with the trained weights of policy.npz: the helper's stock modules, through the helper's lines, give the same."""
    import os
    from conftest import GOLDEN
    g, w = load_golden("ppo_update.npz"), load_golden("policy.npz")
    assert os.path.getsize(os.path.join(GOLDEN, "ppo_update.npz")) <= os.path.getsize(os.path.join(GOLDEN, "policy.npz"))
    assert g["states"].shape == (32, 16) and all(g[k].dtype == np.float32 for k in g.files if k not in ("start", "actions"))
    start = int(g["start"])
    assert np.array_equal(g["states"], w["boards"][start:start + 32].astype(np.float32) / np.float32(15.0))
    nets = golden_modules(w, torch.float64)
    assert R.relu_margin(nets, torch.from_numpy(g["states"]).double()) >= R.RELU_MARGIN
    actions, old, adv, ret = R.recipe(nets, g["states"])
    for got, key in ((actions, "actions"), (old, "old_log_probs"), (adv, "advantages"), (ret, "returns")):
        assert np.array_equal(got, g[key]), key
    res = R.stock_update(nets, g["states"], actions, old, adv, ret)
    grads = [g["grad.%02d" % k] for k in range(24)]
    assert R.ratios(res["grads"], [t.astype(np.float64) for t in grads]).max() <= 1e-6
    assert np.allclose(res["losses"], g["losses"], rtol=1e-6) and np.allclose(res["probs"], g["probs"], rtol=1e-6)
    assert R.ratios(res["running"], [g["running.%d" % k].astype(np.float64) for k in range(8)]).max() <= 1e-6


def test_plain_layout_is_the_modules_parameter_order():
    from g2048 import ops
    for n_out in (4, 1):
        offsets, o = ops.ppo_plain_offsets(n_out), 0
        named = list(RefLayout(n_out).named_parameters())
        assert [name for name, _, _ in offsets] == [name for name, _ in named]
        for (name, off, shape), (_, p) in zip(offsets, named):
            assert off == o and tuple(shape) == tuple(p.shape), name
            assert off % 4 == 0, name                                   # every tensor 16-byte aligned in a 16-byte aligned buffer
            o += p.numel()
        assert o == ops.ppo_plain_floats(n_out) == 46272 + 65 * n_out
    assert [(name, o, k) for name, o, k in ops.PPO_RUNNING_OFFSETS] == [("bn1.running_mean", 0, 256), ("bn1.running_var", 256, 256),
                                                                       ("bn2.running_mean", 512, 128), ("bn2.running_var", 640, 128)]
    assert ops.PPO_RUNNING_FLOATS == 768
    with pytest.raises(ValueError):
        ops.ppo_plain_floats(2)


def test_converter_accepts_the_reference_layout_in_either_mode_and_refuses_the_rest():
    import g2048
    from g2048 import ppo
    for net in (RefLayout(4).train(), RefLayout(4).eval()):
        params, bns = ppo.parse(net, 4)
        assert len(params) == 12 and params[0] is net.fc1.weight and params[-1] is net.fc4.bias and bns == [net.bn1, net.bn2]
    with pytest.raises(ValueError, match="not the reference's layout"):
        ppo.parse(bench_trunk_net(4), 4)
    with pytest.raises(ValueError, match="torch.nn.Module"):
        ppo.parse("actor", 4)
    with pytest.raises(ValueError, match="DevicePPOLearner: Linear 4 is 64->4, expected 64->1"):
        ppo.parse(RefLayout(4), 1)
    bad = RefLayout(4)
    bad.fc2 = nn.Linear(256, 64)
    with pytest.raises(ValueError, match="Linear 2"):
        ppo.parse(bad, 4)
    bad = RefLayout(4)
    bad.bn1 = nn.BatchNorm1d(256, track_running_stats=False)
    with pytest.raises(ValueError, match="running statistics"):
        ppo.parse(bad, 4)
    bad = RefLayout(4)
    bad.bn2 = nn.BatchNorm1d(128, momentum=0.2)
    with pytest.raises(ValueError, match="momentum 0.1"):
        ppo.parse(bad, 4)
    bad = RefLayout(4)
    bad.fc3 = nn.ReLU()
    with pytest.raises(ValueError, match="Linear layers"):
        ppo.parse(bad, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        g2048.DevicePPOLearner(RefLayout(4), RefLayout(1))
    for kw in (dict(clip_epsilon=-0.1), dict(value_coef=float("nan")), dict(entropy_coef=float("inf"))):
        with pytest.raises(ValueError, match="finite and not negative"):
            g2048.DevicePPOLearner(RefLayout(4), RefLayout(1), **kw)
    assert "Dropout" in ppo.__doc__ and "IGNORED" in ppo.__doc__


def test_ppo_entry_points_validate_without_device():
    """Every PPO entry point rejects bad arguments before any device call (status -1, a message); n == 0 is G2048_OK."""
    from g2048 import _lib
    L = _lib.lib()
    hdr = open(__import__("os").path.join(__import__("conftest").REPO, "include", "g2048.h")).read()
    assert "#define G2048_PPO_BATCH_MAX 4096" in hdr and _lib.PPO_BATCH_MAX == 4096
    W = L.g2048_ppo_train_workspace
    assert W(0) == 0 and W(4097) == 0 and W(1) > 0
    sizes = [W(n) for n in range(1, 4097)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 for s in sizes)
    buf = (C.c_uint8 * 4096)()
    base = (C.addressof(buf) + 15) & ~15
    f = C.c_float

    # forward_train(states, plain, running_or_null, n_out, out, n, workspace, stream)
    def fwd(states=base, plain=base, running=None, n_out=4, out=base, n=8, workspace=base):
        return L.g2048_ppo_forward_train(states, plain, running, n_out, out, n, workspace, None)
    assert fwd(n=0) == 0 and fwd(n=0, states=None) == 0
    for name in ("states", "plain", "out", "workspace"):
        assert fwd(**{name: None}) == -1 and b"g2048_ppo_forward_train: null pointer" in L.g2048_last_error(), name
        assert fwd(**{name: base + 4}) == -1 and b"misaligned" in L.g2048_last_error(), name
    assert fwd(running=base + 2) == -1 and b"misaligned" in L.g2048_last_error()
    assert fwd(n_out=1, out=base + 2) == -1 and b"misaligned" in L.g2048_last_error()
    for n_out in (0, 2, 3, 5, -1):
        assert fwd(n_out=n_out) == -1 and b"n_out must be 4 (actor) or 1 (critic)" in L.g2048_last_error()
    assert fwd(n=4097) == -1 and b"G2048_PPO_BATCH_MAX" in L.g2048_last_error() and b"not truncated" in L.g2048_last_error()

    # advantages(values, next_values, rewards, dones, gamma, returns_out, adv_out, n, stream)
    def adv(n=8, gamma=0.995, **kw):
        p = dict(values=base, next_values=base, rewards=base, dones=base, returns_out=base, adv_out=base)
        p.update(kw)
        return L.g2048_ppo_advantages(p["values"], p["next_values"], p["rewards"], p["dones"], f(gamma), p["returns_out"], p["adv_out"], n, None)
    assert adv(n=0) == 0
    for name in ("values", "next_values", "rewards", "dones", "returns_out", "adv_out"):
        assert adv(**{name: None}) == -1 and b"g2048_ppo_advantages: null pointer" in L.g2048_last_error(), name
        assert adv(**{name: base + 2}) == -1 and b"misaligned" in L.g2048_last_error(), name
    assert adv(gamma=float("nan")) == -1 and b"gamma" in L.g2048_last_error()
    assert adv(n=4097) == -1 and b"G2048_PPO_BATCH_MAX" in L.g2048_last_error()

    # loss_grad(states, actions, old, adv, returns, plain_a, plain_c, run_a, run_c, clip, vc, ec, n, grad_a, grad_c, loss_out, ws, stream)
    order = ("states", "actions", "old_log_probs", "advantages", "returns", "plain_actor", "plain_critic", "running_actor", "running_critic")
    tail = ("grad_actor", "grad_critic", "loss_out", "workspace")

    def lg(n=8, clip=0.3, vc=0.4, ec=0.05, **kw):
        p = {k: base for k in order + tail}
        p["running_actor"] = p["running_critic"] = None
        p.update(kw)
        return L.g2048_ppo_loss_grad(*[p[k] for k in order], f(clip), f(vc), f(ec), n, *[p[k] for k in tail], None)
    assert lg(n=0) == 0
    for name in order[:7] + tail:
        assert lg(**{name: None}) == -1 and b"g2048_ppo_loss_grad: null pointer" in L.g2048_last_error(), name
    for name in ("states", "plain_actor", "plain_critic", "grad_actor", "grad_critic", "workspace", "actions"):
        assert lg(**{name: base + 4}) == -1 and b"misaligned" in L.g2048_last_error(), name
    for name in ("old_log_probs", "advantages", "returns", "running_actor", "running_critic", "loss_out"):
        assert lg(**{name: base + 2}) == -1 and b"misaligned" in L.g2048_last_error(), name
    for kw in (dict(clip=-0.1), dict(vc=-1.0), dict(ec=-0.01), dict(clip=float("nan")), dict(vc=float("nan")), dict(ec=float("nan")),
               dict(vc=float("inf"))):
        assert lg(**kw) == -1 and b"finite and not negative" in L.g2048_last_error(), kw
    assert lg(n=4097) == -1 and b"G2048_PPO_BATCH_MAX" in L.g2048_last_error() and b"not truncated" in L.g2048_last_error()


# ---------------------------------------------------------------------- the edge cases of tests/test_gpu_ppo_update_edges.py --
def quiet_update(nets, args, **kw):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return R.stock_update(nets, *args, **kw)


@pytest.mark.parametrize("n", R.POISON_SIZES)
def test_poisoned_inputs_are_what_they_claim_in_stock_torch(n):
    """Per poison: exactly the last row of the named array differs from the case's (with a sign asked for, that row's advantage
    too); stock float32 and float64 agree on the class of every loss part and on which gradient tensors hold a non-finite value
    (the pattern the device is held to is no accident of one precision); the network the poison does not reach keeps the case's
    gradients; old = +inf leaves everything finite, every other poison does not; and old = nan and old = -inf with A = 0, the
    two whose loss a minimum that drops NaN would report as finite, have a NaN loss with every actor gradient non-finite."""
    c = R.case(n)
    assert (n - 1) % 64 == 0 or n == 17                  # 129: row 128 is the first row of the head's third block of 64
    assert abs(c.adv[-1]) > 0.1
    for name, which, value, sign, clean in R.POISONS:
        args = R.poisoned_args(c, which, value, sign)
        for got, was, key in zip(args[2:], c.args[2:], ("old", "adv", "ret")):
            assert np.array_equal(got[:-1], was[:-1]), name
            assert np.array_equal(got[-1:], was[-1:], equal_nan=True) == (key != which and not (key == "adv" and sign is not None
                                                                                                   and got[-1] != was[-1])), name
        if sign is not None:
            assert np.sign(args[3][-1]) == sign
        f32, f64 = quiet_update(c.nets32, args), quiet_update(c.nets64, args)
        assert R.classes(f32["losses"]) == R.classes(f64["losses"]), name
        assert R.nonfinite(f32["grads"]) == R.nonfinite(f64["grads"]), name
        keep = slice(12, 24) if clean == "critic" else slice(0, 12)
        assert all(np.array_equal(a, b) for a, b in zip(f64["grads"][keep], c.want["grads"][keep])), name
        print("n = %d, %s: loss parts %s, non-finite gradient tensors %d" % (n, name, R.classes(f32["losses"]), sum(R.nonfinite(f32["grads"]))))
        if name == "old=+inf":
            assert R.classes(f32["losses"]) == ["finite"] * 4 and not any(R.nonfinite(f32["grads"]))
            assert f64["ratio"][-1] == 0.0
        else:
            other = slice(0, 12) if clean == "critic" else slice(12, 24)
            assert all(R.nonfinite(f32["grads"][other])) and not any(R.nonfinite(f32["grads"][keep])), name
        if name in ("old=nan", "old=-inf,A=0"):
            assert R.classes(f32["losses"])[:2] == ["nan", "nan"]
        if name == "old=-inf,A>0":                      # a finite loss over NaN gradients: stock torch's own behaviour (0 x inf in exp's backward)
            assert R.classes(f32["losses"]) == ["finite"] * 4


def test_advantage_block_inputs():
    """The advantages block's NaN case and zero-deviation case in stock torch: a NaN reward makes its own return and every advantage
    NaN; with rewards 1, values 0.25 and next values 0 every float32 step of the block is exact, the deviation is exactly 0 and
    the divisor is 1e-8 in float32 and float64 alike."""
    n = 17
    rewards = np.ones(n, np.float32)
    rewards[5] = np.nan
    ret, adv = R.advantage_lines(torch.float32, np.zeros(n, np.float32), np.ones(n, np.float32), rewards, np.zeros(n, np.float32))
    assert np.isnan(ret).sum() == 1 and np.isnan(ret[5]) and np.isnan(adv).all()
    flat = (np.full(n, 0.25, np.float32), np.zeros(n, np.float32), np.ones(n, np.float32), np.zeros(n, np.float32))
    for dtype in (torch.float32, torch.float64):
        ret, adv = R.advantage_lines(dtype, *flat)
        assert np.array_equal(ret, np.ones(n)) and np.array_equal(adv, np.zeros(n))


def test_saturated_case_is_saturated():
    """The saturated case's conditions, from the float64 modules: the largest logit gap of a row exceeds 89 (an exp without the
    maximum subtracted overflows float32); on a quarter to three quarters of the rows 1 - max q < 2^-23 / 8 (float32's q is
    exactly 1 and the upper clamp binds) and on no row is it within a factor 8 of 2^-23, where float32 and float64 could decide
    differently; no q within 1 % of 2^-23; saturated rows that take the saturated action, rows that take an action clamped from
    below; ratios on both clip branches; the by-hand float32 evaluation is torch's bit for bit; SAT_SEED is the scan's answer.
    The yardstick is held to 1e-4, the bound of the n = 2 and 3 cases: fc4's weights, and with them the trunk's gradients, are
    128 times the fresh modules'."""
    c = R.saturated_case()
    assert R.find_saturated_seed(c.nets64) == R.SAT_SEED == c.seed
    assert R.relu_margin(c.nets64, torch.from_numpy(c.x).double()) >= R.RELU_MARGIN
    m = R.saturated_measures(c.nets64, c.x)
    sat = m["rest"] < R.SAT_LOW
    rows = np.arange(R.SAT_N)
    taken = m["q"][rows, c.actions]
    print("saturated case: seed %d, logit gap %.4g, %d of %d rows saturated, float32 yardstick %.3g, ratios %.3g .. %.3g, 1 - max q %.3g .. %.3g"
          % (c.seed, m["gap"], sat.sum(), R.SAT_N, c.yardstick, c.want["ratio"].min(), c.want["ratio"].max(), m["rest"].min(), m["rest"].max()))
    assert m["gap"] > 89
    assert 0.25 <= sat.mean() <= 0.75
    assert not ((m["rest"] >= R.SAT_LOW) & (m["rest"] <= R.SAT_HIGH)).any()
    assert (np.abs(m["q"] / R.F32_EPS - 1) >= 0.01).all()
    assert (sat & (c.actions == m["top"])).any() and (taken < R.F32_EPS).any() and R.saturated_ok(m)
    assert (c.f32["probs"].max(1)[sat] == 1.0).all() and (c.f32["probs"].max(1)[~sat] < 1.0).all()
    r = c.want["ratio"]
    assert (r < 1 - R.CLIP).any() and (r > 1 + R.CLIP).any()
    assert min(np.abs(r - (1 - R.CLIP)).min(), np.abs(r - (1 + R.CLIP)).min()) >= 1e-3
    hand = R.stock_update(c.nets32, *c.args, eps=R.F32_EPS)
    assert np.array_equal(hand["losses"], c.f32["losses"]) and all(np.array_equal(a, b) for a, b in zip(hand["grads"], c.f32["grads"]))
    assert np.isfinite(c.want["losses"]).all() and all(np.isfinite(g).all() and g.any() for g in c.want["grads"])
    assert 0 < c.yardstick <= 1e-4


def test_coefficient_sets_cannot_be_ignored():
    """The three coefficient sets at n = 17: a fair float32 yardstick, no ratio within 1e-3 of the set's own clip edges, and the
    float64 gradients differ between every two sets (the default's included) and from what each single coefficient replaced by the
    reference's would give, by at least 1e-2 of max|g| on some tensor: over a hundred times the bound, so that a constant in place
    of an argument cannot pass. value_coef = 0 makes every critic gradient exactly 0 in float64."""
    base = R.case(17)
    sets = [base] + [R.coef_case(k) for k in range(3)]

    def differ(a, b):
        r = R.ratios(a, b)
        return float(np.where(np.isfinite(r), r, 1.0).max())       # inf: a tensor that is exactly 0 on one side only
    for i, a in enumerate(sets):
        clip = a.coefs[0]
        r = a.want["ratio"]
        assert 0 < a.yardstick <= 1e-5
        assert min(np.abs(r - (1 - clip)).min(), np.abs(r - (1 + clip)).min()) >= 1e-3
        for b in sets[i + 1:]:
            d = differ(a.want["grads"], b.want["grads"])
            print("coefficients %s against %s: the gradients differ by %.3g of max|g|" % (a.coefs, b.coefs, d))
            assert d >= 1e-2 >= 100 * max(a.bound, b.bound)
    default = (R.CLIP, R.VALUE_COEF, R.ENTROPY_COEF)
    for c in sets[1:]:
        for pos, name in enumerate(("clip", "value_coef", "entropy_coef")):
            alt = list(c.coefs)
            alt[pos] = default[pos]
            other = R.stock_update(c.nets64, *c.args, clip=alt[0], value_coef=alt[1], entropy_coef=alt[2])
            d = differ(other["grads"], c.want["grads"])
            print("coefficients %s with the reference's %s: the gradients differ by %.3g of max|g|" % (c.coefs, name, d))
            assert d >= 1e-2
    zero = R.coef_case(1)
    assert zero.coefs[1] == 0.0 and all(not g.any() for g in zero.want["grads"][12:]) and all(g.any() for g in zero.want["grads"][:12])
    assert R.coef_case(0).coefs[2] == 0.0 and R.coef_case(2).coefs[0] == 0.0


def test_dead_feature_case():
    """fc1.bias = -10 on features 0 - 7 of both modules at n = 17: these are 0 on every row after the ReLU, and so are, at this
    seed, the features DEAD_ACTOR / DEAD_CRITIC name beyond them (found anew here); in float64 their fc1 and bn1.weight gradients
    are exactly 0, bn1.bias's and fc2.weight's columns are not. The ReLU margin is taken without the eight forced features: they lie
    at -10 +- 1, far from 0, and would otherwise only raise the layer's max|z| the margin is relative to."""
    c = R.dead_case()
    x64 = torch.from_numpy(c.x).double()
    for net, dead, base in zip(c.nets64, (R.DEAD_ACTOR, R.DEAD_CRITIC), (0, 12)):
        assert R.dead_features(net, c.x) == tuple(sorted(dead)) and dead[:8] == R.DEAD
        z = R.relu_inputs(net, x64)
        assert float(z[0][:, :8].max()) < -5.0
        z[0] = z[0][:, 8:]
        margin = min(float(t.abs().min() / t.abs().max()) for t in z)
        print("dead-feature case: %d dead features, ReLU margin %.3g" % (len(dead), margin))
        assert margin >= R.RELU_MARGIN
        g = c.want["grads"]
        idx = list(dead)
        assert not g[base + 0].reshape(256, 16)[idx].any() and not g[base + 1][idx].any() and not g[base + 2][idx].any()
        assert np.abs(g[base + 3][idx]).min() > 0 and np.abs(g[base + 4].reshape(128, 256)[:, idx]).max(0).min() > 0
    assert 0 < c.yardstick <= 1e-5
    p, r = c.want["probs"], c.want["ratio"]
    assert p.min() >= 1e-3 and p.max() <= 1 - 1e-3
    assert min(np.abs(r - (1 - R.CLIP)).min(), np.abs(r - (1 + R.CLIP)).min()) >= 1e-3


def test_closed_loop_case():
    """The whole-update case (n = 48, 3 epochs, the advantages block first): LOOP_SEED is the scan's answer; the ReLU margin holds
    for the next states under the initial critic and for the states under the weights of every epoch of the float64 run; the clip
    acts on both networks in every epoch; the ratios are on both clip branches in the last epoch; both done values occur; the
    advantages depend on WHICH forward's values are subtracted; and with Adam's eps = lr the float32 run's parameters stay
    within 1e-6 of max|p| of the float64 run's (at eps = 1e-8 a gradient within rounding of zero moves a weight by 2 lr)."""
    c = R.loop_case()
    assert R.find_loop_seed(c.nets64) == R.LOOP_SEED == c.seed
    x, nx, rewards, dones = c.inputs
    assert not np.array_equal(x, nx) and set(dones.tolist()) == {0.0, 1.0}
    assert R.relu_margin(c.nets64[1:], torch.from_numpy(nx).double()) >= R.RELU_MARGIN
    assert 0 < c.yardstick <= 1e-5
    adv = c.want["adv"]
    swapped = R.advantage_lines(torch.float64, adv["next_values"], adv["next_values"], rewards, dones)[1]
    assert R.rel(swapped, adv["advantages"]) > 1e-2 > 1000 * c.adv_bound
    for e, (w, f) in enumerate(zip(c.want["epochs"], c.f32["epochs"])):
        dev = max(np.abs(a - b).max() / np.abs(s).max() for a, b, s in zip(f["delta"], w["delta"], c.want["start"]))
        print("epoch %d: ReLU margin %.3g, gradient norms %.3g (actor) %.3g (critic), ratios %.3g .. %.3g, float32 run off by %.3g of max|p|"
              % (e, w["margin"], w["norms"][0], w["norms"][1], w["ratio"].min(), w["ratio"].max(), dev))
        assert w["margin"] >= R.RELU_MARGIN
        assert min(w["norms"]) > R.MAX_NORM and min(f["norms"]) > R.MAX_NORM
        assert dev <= 1e-6
        assert all(np.abs(d).max() > 0 for d in w["delta"])
    r = c.want["epochs"][-1]["ratio"]
    assert (r < 1 - R.CLIP).any() and (r > 1 + R.CLIP).any()
    assert c.want["tracked"] == [3, 3, 5, 5] and len(c.want["epochs"]) == R.LOOP_EPOCHS
