"""CPU side of the transformer policy's device step (csrc/g2048_tpolicy_step.hip): the yardstick of tests/test_gpu_tpolicy_step.py
against stock clip_grad_norm_ + torch.optim.Adam on the float64 module, the layout facts the kernel's tail and eps-slot handling
rest on, the conditions under which the GPU tests can fail, and ops' refusals before any device."""
import copy

import numpy as np
import pytest
import torch

import tpolicy_step_ref as T
from qnet_grad_ref import plain_slices

HOST_SHAPES = ((32, 1), (96, 2))


def parsed_of(module):
    from g2048 import tpolicy
    return tpolicy.parse(module)


@pytest.mark.parametrize("dim_ff, layers", HOST_SHAPES)
def test_yardstick_is_clip_grad_norm_and_adam_in_float64(dim_ff, layers):
    """The case's four steps (norms 2, 1, 0.5, 0.5 x max_norm): per tensor, weights and both moments within 1e-12 of the tensor's
    largest entry of stock float64, and the eps slots of all four buffers keep their values."""
    plain, grads = T.step_case(dim_ff, layers)
    module = copy.deepcopy(T.module_of(dim_ff, layers)).double()
    parsed = parsed_of(module)
    slices, eps_at, total = plain_slices(parsed)
    assert total == plain.numel() and list(T.eps_slots(dim_ff, layers)) == eps_at
    params = [t for t in parsed.plain_tensors() if isinstance(t, torch.Tensor)]
    opt = torch.optim.Adam(params, lr=T.LR, eps=T.EPS, betas=T.BETAS)
    state = (T.flat_of(module, torch.float64), None, torch.zeros(total, dtype=torch.float64), torch.zeros(total, dtype=torch.float64))
    start_eps = state[0][eps_at].clone()
    worst = 0.0
    for step, g in enumerate(grads, 1):
        for p, (o, k) in zip(params, slices):
            p.grad = g[o:o + k].double().view(p.shape).clone()
        torch.nn.utils.clip_grad_norm_(params, T.MAX_NORM)
        opt.step()
        state = T.adam_step_reference(state[0], g.double(), state[2], state[3], eps_at, T.LR, step)[:4]
        for got, stock in ((state[0], params), (state[2], [opt.state[p]["exp_avg"] for p in params]),
                           (state[3], [opt.state[p]["exp_avg_sq"] for p in params])):
            for (o, k), w in zip(slices, stock):
                w = w.detach().reshape(-1).numpy()
                worst = max(worst, T.deviation(got[o:o + k].numpy(), w))
        assert torch.equal(state[0][eps_at], start_eps) and not state[2][eps_at].any() and not state[3][eps_at].any()
        assert not state[1][eps_at].any()
    print("yardstick against stock float64 clip_grad_norm_ + Adam, worst tensor: %.3g of its largest entry" % worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("dim_ff, layers", HOST_SHAPES)
def test_float32_yardstick_deviates_so_the_tolerance_is_not_empty(dim_ff, layers):
    plain, grads = T.step_case(dim_ff, layers)
    n = plain.numel()
    pre = (plain, grads[0], grads[1] * 0.1, grads[2] * grads[2])
    y64, y32 = T.yardsticks(pre, T.eps_slots(dim_ff, layers), 3)
    for i, name in ((0, "plain"), (2, "exp_avg"), (3, "exp_avg_sq")):
        d = T.deviation(y32[i], y64[i])
        print("%s: the float32 yardstick is %.3g of the largest entry from the float64 one" % (name, d))
        assert 0 < d < 1e-5, name
    assert n == T.plain_floats(dim_ff, layers)


def test_layout_facts():
    """The buffer is 1 mod 4 floats long with an even layer count and 3 mod 4 with an odd one; a layer's block starts at a multiple
    of 4 plus 2 l and is 2 mod 4 long, so the eps pair is the first half of a 16-byte group in layers 0, 2, .. and the second in layers 1, 3, ..."""
    from g2048 import ops
    for dim_ff in (32, 96, 2048, 4096, 65536):
        for layers in (1, 2, 3, 64):
            n = ops.tpolicy_plain_floats(dim_ff, layers)
            assert n == T.plain_floats(dim_ff, layers) and n % 4 == (1 if layers % 2 == 0 else 3)
            assert (16962 + 129 * dim_ff) % 4 == 2
            at = T.eps_slots(dim_ff, layers)
            assert len(at) == 2 * layers and [int(a) % 4 for a in at[:4]] == [0, 1, 2, 3][:len(at[:4])]
    assert [T.plain_floats(*s) for s in T.SHAPES] == [160999, 198601, 702217, 1230601]
    assert T.plain_floats(4096, 2) > 1024 * 1024 >= T.plain_floats(2048, 2)      # above 1,024 chunks of 1,024 floats: two passes a block
    module = T.module_of(96, 2)
    slices, eps_at, total = plain_slices(parsed_of(module))
    assert eps_at == list(T.eps_slots(96, 2)) and total == 198601


def test_clip_pattern_of_the_four_step_case():
    """A norm AT max_norm is clipped (c = max_norm / (max_norm + 1e-6) < 1): steps 1 and 2 clip, 3 and 4 do not; the gradients span
    several decades, their eps slots are 0 and their last float (the short tail group) is far above eps."""
    for dim_ff, layers in HOST_SHAPES:
        _, grads = T.step_case(dim_ff, layers)
        at = T.eps_slots(dim_ff, layers)
        for s, g in enumerate(grads):
            norm = float(np.linalg.norm(g.numpy().astype(np.float64)))
            assert norm == pytest.approx(T.FACTORS[s] * T.MAX_NORM, rel=1e-6)
            assert (T.clip_coefficient(norm) < 1.0) == (s < 2)
            mags = np.abs(g.numpy())
            assert np.percentile(mags, 99) / np.percentile(mags, 1) > 1e4
            assert not g[at].any() and abs(float(g[-1])) > 10 * T.EPS


def test_counting_a_skipped_call_cannot_pass():
    """apply, skip, apply: the third call is Adam step 2. The yardstick at step 3 is further from the yardstick at step 2 than TWICE the
    GPU test's bound on the weights, so a result within the bound of one is outside the bound of the other."""
    for dim_ff, layers in HOST_SHAPES:
        at2, at3 = T.run_reference(dim_ff, layers, (0, 1), (1, 2)), T.run_reference(dim_ff, layers, (0, 1), (1, 3))
        f32 = T.run_reference(dim_ff, layers, (0, 1), (1, 2), dtype=torch.float32)
        bound = T.F32_FACTOR * T.deviation(f32[0], at2[0])
        apart = T.deviation(at3[0], at2[0])
        print("weights at step 3 are %.3g of max|w| from step 2; the bound is %.3g" % (apart, bound))
        assert bound > 0 and apart > 2 * bound


def test_ops_checks_before_any_device():
    """ops.tpolicy_adam_step reads dtype and length of all four buffers before it touches a device or the library."""
    from g2048 import ops
    n = T.plain_floats(32, 1)
    good = [torch.zeros(n) for _ in range(4)]
    counters = torch.zeros(3, dtype=torch.int64)
    for i in range(4):
        bad = list(good)
        bad[i] = torch.zeros(n + 1)
        with pytest.raises(ValueError, match="flat float32 tensor of %d floats" % n):
            ops.tpolicy_adam_step(*bad, 32, 1, counters)
        bad[i] = good[i].double()
        with pytest.raises(TypeError, match="flat float32 tensor"):
            ops.tpolicy_adam_step(*bad, 32, 1, counters)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.tpolicy_adam_step(*good, 32, 1, counters)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.tpolicy_step_workspace_bytes(48, 2)
    assert ops.tpolicy_step_workspace_bytes(2048, 2) % 16 == 0


def test_the_two_clip_forms_differ_where_the_gpu_test_looks():
    """With max_norm a power of two the two float32 forms of the clip coefficient are the same bits (scaling by 2^k commutes with
    rounding), so PPOAgent's 0.5 cannot tell them apart; at max_norm 0.3 and the case's scales they differ by an ulp."""
    _, grads = T.step_case(96, 2)
    for scale in T.CLIP_FORM_SCALES:
        g = (grads[1] * np.float32(scale)).numpy()
        norm = np.float32(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        first, direct = T.clip_forms(norm, T.CLIP_FORM_MAX_NORM)
        assert first != direct and first < 1.0, (scale, first, direct)
        assert np.array_equal(*T.clip_forms(norm, 0.5)) and np.array_equal(*T.clip_forms(norm, 0.25))
