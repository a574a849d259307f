"""CPU side of the PPO update's device step (csrc/g2048_ppo_step.hip): the yardstick of tests/test_gpu_ppo_step.py against stock
clip_grad_norm_ + torch.optim.Adam, the layout facts the kernel's tail handling rests on, the C-ABI's refusals (no device is needed:
the arguments are checked before any device call), and the conditions under which the GPU tests can fail: which network is clipped
in which step of the four-step case, and that counting a skipped call cannot pass."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import ppo_step_ref as S
import ppo_update_ref as R


def stock_steps(module64, grads, lr, eps, max_norm):
    """clip_grad_norm_ + Adam.step() on a float64 reference-layout module, one step per flat gradient: (plain, exp_avg, exp_avg_sq)
    flat float64 NumPy after each step."""
    params = list(module64.parameters())
    opt = torch.optim.Adam(params, lr=lr, eps=eps)
    out = []
    for g in grads:
        o = 0
        for p in params:
            p.grad = g[o:o + p.numel()].view(p.shape).clone()
            o += p.numel()
        torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        out.append(tuple(torch.cat([t.detach().reshape(-1) for t in ts]).numpy().copy()
                         for ts in (params, [opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params])))
    return out


def test_yardstick_is_clip_grad_norm_and_adam_in_float64():
    """Four steps with the gradient norm at 2, 1, 0.5 and 3 x max_norm on both networks: weights and both moments within 1e-12 of the
    largest entry of stock float64 (measured: 8.8e-16 with these gradients)."""
    nets = R.make_modules()
    rng = np.random.default_rng(7)
    worst = 0.0
    for k, net in enumerate(nets):
        module = copy.deepcopy(net).double()
        floats = S.FLOATS[k]
        grads = [S.spread_gradient(rng, floats, f * S.MAX_NORM).double() for f in (2.0, 1.0, 0.5, 3.0)]
        want = stock_steps(module, grads, S.LR[k], S.EPS[k], S.MAX_NORM)
        state = (S.flat_of(net).double(), None, torch.zeros(floats, dtype=torch.float64), torch.zeros(floats, dtype=torch.float64))
        for step, (g, w) in enumerate(zip(grads, want), 1):
            p, gc, m, v, norm = S.adam_step_reference(state[0], g, state[2], state[3], S.LR[k], step, eps=S.EPS[k])
            state = (p, gc, m, v)
            for got, stock in ((p, w[0]), (m, w[1]), (v, w[2])):
                worst = max(worst, S.deviation(got.numpy(), stock))
    print("yardstick against stock float64 clip_grad_norm_ + Adam: %.3g of the largest entry" % worst)
    assert worst <= 1e-12


def test_layout_facts():
    from g2048 import ops
    assert ops.ppo_plain_floats(4) == S.ACTOR_FLOATS == 46532 and ops.ppo_plain_floats(1) == S.CRITIC_FLOATS == 46337
    assert 46532 % 4 == 0 and 46337 % 4 == 1
    name, offset, shape = ops.ppo_plain_offsets(1)[-1]
    assert name == "fc4.bias" and offset == S.CRITIC_FLOATS - 1 and shape == (1,)      # the critic's last float is a group of its own


def test_clip_pattern_of_the_four_step_case():
    """What the GPU test's four steps exercise. A norm AT max_norm is clipped (c = max_norm / (max_norm + 1e-6) < 1), so: step 1 the
    actor alone, step 2 both (the actor at its edge), step 3 the critic alone, at its edge, with the actor unclipped, step 4 neither.
    The critic's last float (fc4.bias) has a step-1 gradient far above eps, so its first Adam step is lr to within eps / |g|."""
    plains, grads = S.step_case()
    clipped = [[S.clip_coefficient(float(np.linalg.norm(g[k].numpy().astype(np.float64)))) < 1.0 for k in (0, 1)] for g in grads]
    assert clipped == [[True, False], [True, True], [False, True], [False, False]]
    for s, g in enumerate(grads):
        for k in (0, 1):
            norm = float(np.linalg.norm(g[k].numpy().astype(np.float64)))
            assert norm == pytest.approx(S.FACTORS[k][s] * S.MAX_NORM, rel=1e-6)
            mags = np.abs(g[k].numpy())
            assert np.percentile(mags, 99) / np.percentile(mags, 1) > 1e4, "the gradient does not span several decades"
    c3 = S.clip_coefficient(float(np.linalg.norm(grads[2][1].numpy().astype(np.float64))))
    assert 0.99999 < c3 < 1.0
    assert abs(float(grads[0][1][-1])) > 10 * S.EPS[1]              # the first step is lr |g| / (|g| + eps): above 0.9 lr
    assert S.LR[0] != S.LR[1] and S.EPS[0] != S.EPS[1]


def test_counting_a_skipped_call_cannot_pass():
    """apply, skip, apply: the third call is Adam step 2. The yardstick at step 3 is further from the yardstick at step 2 than TWICE the
    GPU test's bound on the weights of both networks, so a result within the bound of one is outside the bound of the other."""
    at2, at3 = S.run_reference((0, 1), (1, 2)), S.run_reference((0, 1), (1, 3))
    f32 = S.run_reference((0, 1), (1, 2), dtype=torch.float32)
    for k in (0, 1):
        bound = S.F32_FACTOR * S.deviation(f32[k][0], at2[k][0])
        apart = S.deviation(at3[k][0], at2[k][0])
        print("network %d: weights at step 3 are %.3g of max|w| from step 2; the bound is %.3g" % (k, apart, bound))
        assert bound > 0 and apart > 2 * bound
        assert np.array_equal(at3[k][2], at2[k][2]) and np.array_equal(at3[k][3], at2[k][3])      # the moments do not see the number


def test_ppo_adam_step_validates_without_device():
    """Every refusal of g2048_ppo_adam_step (status -1, a message), before any device call; each call below has exactly one defect."""
    from g2048 import _lib
    L = _lib.lib()
    assert L.g2048_abi_version() == 5
    nb = L.g2048_ppo_step_workspace()
    assert nb > 0 and nb % 16 == 0
    buf = (C.c_uint8 * 4096)()
    base = (C.addressof(buf) + 15) & ~15
    f = C.c_float
    pointers = ("plain_actor", "grad_actor", "exp_avg_actor", "exp_avg_sq_actor", "plain_critic", "grad_critic", "exp_avg_critic",
                "exp_avg_sq_critic", "loss", "counters")
    tail = ("norms_out", "workspace")

    def call(lr_a=8e-4, lr_c=2e-3, b1=0.9, b2=0.999, eps_a=1e-8, eps_c=1e-8, max_norm=0.5, **kw):
        p = {k: base for k in pointers + tail}
        p.update(kw)
        return L.g2048_ppo_adam_step(*[p[k] for k in pointers], f(lr_a), f(lr_c), f(b1), f(b2), f(eps_a), f(eps_c), f(max_norm),
                                     *[p[k] for k in tail], None)
    for name in pointers[:8] + ("counters",) + tail:
        assert call(**{name: None}) == -1 and b"g2048_ppo_adam_step: null pointer" in L.g2048_last_error(), name
    for name in pointers[:8] + ("workspace",):
        assert call(**{name: base + 4}) == -1 and b"misaligned" in L.g2048_last_error(), name
        assert call(**{name: base + 8}) == -1 and b"misaligned" in L.g2048_last_error(), name
    assert call(counters=base + 4) == -1 and b"misaligned" in L.g2048_last_error()
    assert call(norms_out=base + 2) == -1 and b"misaligned" in L.g2048_last_error()
    assert call(loss=base + 2) == -1 and b"misaligned" in L.g2048_last_error()
    nan, inf = float("nan"), float("inf")
    for key in ("lr_a", "lr_c", "b1", "b2", "eps_a", "eps_c"):
        for bad in (nan, inf, -inf, -1e-3):
            assert call(**{key: bad}) == -1 and b"finite and not negative" in L.g2048_last_error(), (key, bad)
    for key in ("b1", "b2"):
        for bad in (1.0, 1.5):
            assert call(**{key: bad}) == -1 and b"must be below 1" in L.g2048_last_error(), (key, bad)
    for bad in (nan, 0.0, -0.5, -inf):
        assert call(max_norm=bad) == -1 and b"max_norm must be above 0" in L.g2048_last_error(), bad


def test_ops_checks_before_any_device():
    """ops.ppo_adam_step reads dtype and length of all eight buffers before it touches a device."""
    from g2048 import ops
    good = [torch.zeros(S.FLOATS[k]) for k in (0, 0, 0, 0, 1, 1, 1, 1)]
    counters = torch.zeros(4, dtype=torch.int64)
    for i in range(8):
        bad = list(good)
        bad[i] = torch.zeros(S.FLOATS[0 if i < 4 else 1] + 1)
        with pytest.raises(ValueError, match="flat float32 tensor of %d floats" % S.FLOATS[0 if i < 4 else 1]):
            ops.ppo_adam_step(*bad, counters)
        bad[i] = good[i].double()
        with pytest.raises(TypeError, match="flat float32 tensor"):
            ops.ppo_adam_step(*bad, counters)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.ppo_adam_step(*good, counters)
    with pytest.raises(ValueError, match="scalar or an \\(actor, critic\\) pair"):
        ops.ppo_pair((1, 2, 3), "lr")
    assert ops.ppo_pair(3e-4, "lr") == (3e-4, 3e-4) and ops.ppo_pair((1e-3, 2e-3), "lr") == (1e-3, 2e-3)
