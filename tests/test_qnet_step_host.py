"""CPU-side checks of the Q-network's device update (DeviceQNetwork.adamw_step, g2048_qnet_adamw_step): the plain-torch yardstick
adamw_step_reference in float64 against clip_grad_norm_ + torch.optim.AdamW on the stock module, the two schedule helpers against
CosineAnnealingLR and the reference's epsilon formula, the C-ABI's argument validation and workspace arithmetic without a device, and
the refusals of ops.qnet_adamw_step. The kernels themselves are checked on the GPU (tests/test_gpu_qnet_step.py)."""
import ctypes as C

import pytest
import torch

import qnet_grad_ref as R
from test_qnet_host import random_model

MAX_NORM, WEIGHT_DECAY = 10.0, 1e-4
NORM_FACTORS = (2.0, 1.5, 0.5, 0.25)                       # the gradient norm as a multiple of MAX_NORM, step by step


def flat64(parsed):
    """The parsed float64 module as one float64 buffer in the plain layout (qnet.flatten writes float32)."""
    return torch.cat([t.detach().reshape(-1) if isinstance(t, torch.Tensor) else torch.tensor([t], dtype=torch.float64)
                      for t in parsed.plain_tensors()])


@pytest.mark.parametrize("seed, dim_ff, layers", [(2, 32, 1), (2, 160, 2)], ids=["ff32-L1", "ff160-L2"])
def test_adamw_step_reference_is_clip_grad_norm_and_stock_adamw(seed, dim_ff, layers):
    import g2048
    from g2048 import qnet
    model = random_model(seed, dim_ff, layers).double()
    parsed = qnet.parse(model)
    slices, eps_at, total = R.plain_slices(parsed)
    assert total == g2048.ops.qnet_plain_floats(dim_ff, layers) and len(eps_at) == 2 * layers
    params = list(model.parameters())
    optimizer = torch.optim.AdamW(params, lr=1e-3, weight_decay=WEIGHT_DECAY)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=150000, eta_min=1e-4)
    plain = flat64(parsed)
    eps_values = plain[eps_at].clone()
    assert torch.all(eps_values > 0)
    m, v = torch.zeros_like(plain), torch.zeros_like(plain)
    rng = torch.Generator().manual_seed(17)
    clipped_steps = []
    for t, factor in enumerate(NORM_FACTORS):
        grad = torch.randn(total, generator=rng, dtype=torch.float64)
        grad[eps_at] = 0.0
        grad *= factor * MAX_NORM / grad.norm()
        for p, (o, k) in zip(params, slices):
            p.grad = grad[o:o + k].reshape(p.shape).clone()
        want_norm = torch.nn.utils.clip_grad_norm_(params, max_norm=MAX_NORM)
        lr = g2048.cosine_lr(t)
        assert optimizer.param_groups[0]["lr"] == pytest.approx(lr, rel=1e-12)
        optimizer.step()
        scheduler.step()
        plain, g, m, v, norm = qnet.adamw_step_reference(plain, grad, m, v, eps_at, lr, t + 1, weight_decay=WEIGHT_DECAY, max_norm=MAX_NORM)
        clipped_steps.append(bool(norm > MAX_NORM))
        assert abs(float(norm) - float(want_norm)) <= 1e-12 * float(want_norm) and float(norm) == pytest.approx(factor * MAX_NORM, rel=1e-12)
        state = [optimizer.state[p] for p in params]
        for what, got, want in (("weights", plain, [p.detach() for p in params]), ("clipped gradients", g, [p.grad for p in params]),
                                ("exp_avg", m, [s["exp_avg"] for s in state]), ("exp_avg_sq", v, [s["exp_avg_sq"] for s in state])):
            want = torch.cat([w.reshape(-1) for w in want])
            got = torch.cat([got[o:o + k] for o, k in slices])
            err = float((got - want).abs().max() / want.abs().max())
            print("step %d, %s: %.3g of the largest entry" % (t + 1, what, err))
            assert err <= 1e-12, (t, what)
        assert all(int(s["step"]) == t + 1 for s in state)
        assert torch.equal(plain[eps_at], eps_values), "a LayerNorm-eps slot of plain moved"
        assert not g[eps_at].any() and not m[eps_at].any() and not v[eps_at].any()
    assert clipped_steps == [True, True, False, False]
    # a gradient that is not finite changes nothing; no clipping at all with max_norm None
    bad = grad.clone()
    bad[5] = float("inf")
    out = qnet.adamw_step_reference(plain, bad, m, v, eps_at, 1e-3, 5)
    assert all(torch.equal(x, y) for x, y in zip(out[:4], (plain, bad, m, v))) and not torch.isfinite(out[4])
    out = qnet.adamw_step_reference(plain, 100 * grad, m, v, eps_at, 1e-3, 5, max_norm=None)
    assert torch.equal(out[1], 100 * grad) and float(out[4]) == pytest.approx(25 * MAX_NORM, rel=1e-12)


def test_cosine_lr_is_cosine_annealing_lr():
    import g2048
    p = torch.nn.Parameter(torch.zeros(1))
    optimizer = torch.optim.AdamW([p], lr=1e-3)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=2000, eta_min=1e-4)
    worst = 0.0
    for t in range(2001):
        want = optimizer.param_groups[0]["lr"]
        got = g2048.cosine_lr(t, t_max=2000)
        worst = max(worst, abs(got - want) / want)
        optimizer.step()
        scheduler.step()
    print("cosine_lr against CosineAnnealingLR over 2001 steps: %.3g" % worst)
    assert worst <= 1e-12
    assert g2048.cosine_lr(0) == 1e-3 and g2048.cosine_lr(150000) == pytest.approx(1e-4, rel=1e-12)
    assert g2048.cosine_lr(5, base_lr=2e-3, t_max=10, eta_min=0.0) == pytest.approx(1e-3, rel=1e-12)
    for bad in (-1, 150001):
        with pytest.raises(ValueError, match="0 <= t <= t_max"):
            g2048.cosine_lr(bad)


def test_dqn_epsilon_is_the_references_formula():
    import g2048
    start, end, decay = 1.0, 0.001, 150000
    for steps in (0, 1, decay // 2, decay, 2 * decay):
        progress = min(steps / decay, 1.0)
        assert g2048.dqn_epsilon(steps) == max(end, start - (start - end) * (progress ** 0.6)), steps
    assert g2048.dqn_epsilon(0) == 1.0 and g2048.dqn_epsilon(decay) == pytest.approx(0.001) and g2048.dqn_epsilon(2 * decay) == g2048.dqn_epsilon(decay)
    assert g2048.dqn_epsilon(50, start=0.5, end=0.1, decay_steps=100) == max(0.1, 0.5 - 0.4 * 0.5 ** 0.6)


def test_step_entry_points_validate_without_device():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib, ops
    L = _lib.lib()
    assert L.g2048_abi_version() == 5
    hdr = open(__import__("os").path.join(__import__("conftest").REPO, "include", "g2048.h")).read()
    assert "g2048_qnet_adamw_step" in hdr and "g2048_qnet_step_workspace" in hdr
    assert "#define G2048_QNET_STEP_MAX_PARTIALS %d\n" % _lib.QNET_STEP_MAX_PARTIALS in hdr
    W = L.g2048_qnet_step_workspace
    for bad in ((48, 2), (0, 2), (-32, 2), (64, 0), (64, 65), (64, -1)):
        assert W(*bad) == 0, bad
    for ff, layers in ((32, 1), (2048, 2), (4096, 64), (160, 2), (96, 3), (65536, 64)):
        nb = W(ff, layers)
        assert 0 < nb <= 8 * _lib.QNET_STEP_MAX_PARTIALS and nb % 16 == 0, (ff, layers, nb)
        # the chunks are whole passes of 1,024 floats and no more of them than the buffer needs
        floats = ops.qnet_plain_floats(ff, layers)
        chunk = -(-(-(-floats // _lib.QNET_STEP_MAX_PARTIALS)) // 1024) * 1024
        assert nb == -(-(-(-floats // chunk) * 8) // 16) * 16, (ff, layers, nb)
        assert ops.qnet_step_workspace_bytes(ff, layers) == nb
    with pytest.raises(ValueError, match="multiple of 32 and 1 .. 64 layers"):
        ops.qnet_step_workspace_bytes(48, 2)
    buf = (C.c_uint8 * 256)()
    p = (C.addressof(buf) + 15) & ~15
    F = L.g2048_qnet_adamw_step
    names = ("plain", "grad", "exp_avg", "exp_avg_sq", "norm", "workspace")

    def call(ff=64, layers=2, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-4, max_norm=10.0, step=1, **ptr):
        v = {k: ptr.get(k, p) for k in names}
        return F(v["plain"], v["grad"], v["exp_avg"], v["exp_avg_sq"], ff, layers, lr, beta1, beta2, eps, wd, max_norm, step, v["norm"],
                 v["workspace"], None)

    def refused(word, **kw):
        return call(**kw) == -1 and b"g2048_qnet_adamw_step" in L.g2048_last_error() and word in L.g2048_last_error()

    for name in names:
        assert refused(b"null pointer", **{name: None}), name
    for name, off in (("plain", 8), ("grad", 4), ("exp_avg", 8), ("exp_avg_sq", 4), ("workspace", 8), ("norm", 2)):
        assert refused(b"misaligned", **{name: p + off}), name
    assert refused(b"dim_ff", ff=48) and refused(b"n_layers", layers=0) and refused(b"n_layers", layers=65)
    assert refused(b"step", step=0)
    assert refused(b"below 1", beta1=1.0) and refused(b"below 1", beta2=1.0) and refused(b"below 1", beta2=1.5)
    for name in ("lr", "beta1", "beta2", "eps", "wd"):
        for value in (-1e-3, float("nan"), float("inf")):
            assert refused(b"finite and not negative", **{name: value}), (name, value)
    for value in (float("nan"), 0.0, -1.0, float("-inf")):
        assert refused(b"max_norm", max_norm=value), value


def test_adamw_step_refusals_name_their_reason():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import ops
    floats = ops.qnet_plain_floats(64, 2)
    ok = torch.zeros(floats)
    with pytest.raises(RuntimeError, match="plain must live on a ROCm device.*no CPU path"):
        ops.qnet_adamw_step(ok, ok, ok, ok, 64, 2, 1e-3, 1)
    with pytest.raises(TypeError, match="plain must be a torch.Tensor"):
        ops.qnet_adamw_step([0.0] * 4, ok, ok, ok, 64, 2, 1e-3, 1)
    for i, name in enumerate(("plain", "grad", "exp_avg", "exp_avg_sq")):
        args = [ok] * 4
        for wrong in (ok[:-1], torch.zeros(floats + 2), ok.reshape(2, -1)):
            args[i] = wrong
            with pytest.raises(ValueError, match="%s must be a flat float32 tensor of %d floats" % (name, floats)):
                ops.qnet_adamw_step(*args, 64, 2, 1e-3, 1)
        for wrong in (ok.double(), ok.to(torch.bfloat16)):
            args[i] = wrong
            with pytest.raises(TypeError, match="%s must be a flat float32 tensor" % name):
                ops.qnet_adamw_step(*args, 64, 2, 1e-3, 1)
    with pytest.raises(ValueError, match="dim_ff"):            # the length is that of (dim_ff, n_layers): a bad pair fits no buffer
        ops.qnet_step_workspace_bytes(64, 0)
