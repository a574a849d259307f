"""CPU-side checks of the transformer policy's loss and gradient pass: g2048.tpolicy.loss_grad_reference (the definition of the
function, in plain torch ops with autograd) against autograd through a stock nn.Module of the reference's layout with the same
loss, and against the reference class's recorded gradients (tests/golden/tpolicy_grad.npz); the conditions that make the GPU
cases and the fixture pin something; the host side of the wrapper. The kernels are checked on the GPU
(tests/test_gpu_tpolicy_grad.py)."""
import os

import numpy as np
import pytest
import torch

import tpolicy_grad_ref as R
from conftest import GOLDEN, load_golden
from test_tpolicy_host import golden_model

tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731


def reference(model64, args, **kw):
    from g2048 import tpolicy
    p = tpolicy.parse(model64)
    losses, probs, value, flat = tpolicy.loss_grad_reference(p, *(tt(a) for a in args), **kw)
    grads, eps = R.split(p, flat.numpy())
    assert flat.dtype == torch.float64 and np.all(eps == 0) and len(eps) == 2 * len(p.layers)
    return dict(losses=losses.numpy(), probs=probs.numpy(), value=value.numpy(), grads=grads)


@pytest.mark.parametrize("shape", R.HOST_CASES, ids=["n%d-ff%d-L%d" % c for c in R.HOST_CASES])
def test_reference_equals_stock_autograd_in_float64(shape):
    c = R.case(*shape)
    c.conditions()
    got = reference(c.model64, c.args)
    r = R.ratios(got["grads"], c.want["grads"])
    assert len(got["grads"]) == len(c.want["grads"]) == 2 + 12 * c.layers + 8
    assert r.max() <= 1e-12, r
    assert np.abs(got["losses"] - c.want["losses"]).max() <= 1e-12 * np.abs(c.want["losses"]).max()
    assert np.abs(got["probs"] - c.want["probs"]).max() <= 1e-12 and R.rel(got["value"], c.want["value"]) <= 1e-12
    assert all(p.grad is None for p in c.model64.parameters()), "the module's own .grad fields are not touched"


def test_other_coefficients_reach_the_reference():
    c = R.case(17, 96, 2)
    coefs = dict(clip=0.1, value_coef=1.0, entropy_coef=0.2)
    want = R.stock_loss_grad(c.model64, *c.args, **coefs)
    got = reference(c.model64, c.args, clip_epsilon=0.1, value_coef=1.0, entropy_coef=0.2)
    assert R.ratios(got["grads"], want["grads"]).max() <= 1e-12 and np.abs(got["losses"] - want["losses"]).max() <= 1e-12
    assert np.abs(want["losses"] - c.want["losses"]).max() > 1e-3


@pytest.mark.parametrize("shape", R.GPU_CASES, ids=["n%d-ff%d-L%d" % c for c in R.GPU_CASES])
def test_the_gpu_cases_meet_their_conditions(shape):
    """The clipped branch binds on 10 .. 90 % of the rows (N > 2), both signs of advantage, no zero gradient tensor, a value head
    that does not cancel, a float32 yardstick above zero: asserted here too, where a change of recipe shows at once."""
    c = R.case(*shape)
    c.conditions()
    assert c.boards.shape == (c.n, 16) and sorted(set(c.actions.tolist())) == sorted(set(((5 * np.arange(c.n) + 1) % 4).tolist()))


def test_reference_equals_the_reference_class_recorded_gradients():
    g = load_golden("tpolicy_grad.npz")
    _, model = golden_model()
    args = (g["boards"], g["actions"], g["old_log_probs"], g["advantages"], g["returns"])
    got = reference(model, args)
    names = g["tensor_names"].tolist()
    assert len(names) == len(got["grads"]) == 34
    for i, (k, x) in enumerate(zip(names, got["grads"])):
        pos = R.golden_positions(x.size)
        assert g["grad." + k].shape == pos.shape and (x.size <= R.GOLDEN_FULL) == (pos.size == x.size)
        assert np.abs(x[pos] - g["grad." + k]).max() <= 1e-12 * g["gmax"][i], k
        assert abs(np.abs(x).max() - g["gmax"][i]) <= 1e-12 * g["gmax"][i] and g["gmax"][i] > 0, k
    assert np.abs(got["losses"] - g["losses_f64"]).max() <= 1e-12
    assert np.abs(got["probs"] - g["probs_f64"]).max() <= 1e-12 and R.rel(got["value"], g["value_f64"]) <= 1e-12


def test_the_fixture_pins_something():
    g = load_golden("tpolicy_grad.npz")
    _, model = golden_model()
    args = (g["boards"], g["actions"], g["old_log_probs"], g["advantages"], g["returns"])
    want = R.stock_loss_grad(model, *args)
    share = want["clipped"].mean()
    assert g["boards"].shape == (R.GOLDEN_ROWS, 16) and R.BAND[0] <= share <= R.BAND[1], share
    assert (g["advantages"] > 0).any() and (g["advantages"] < 0).any()
    assert float(g["yardstick_f32"]) > 0 and (g["gmax"] > 0).all()
    assert np.array_equal(g["boards"], load_golden("policy.npz")["boards"][int(g["start"]):int(g["start"]) + R.GOLDEN_ROWS])
    assert os.path.getsize(os.path.join(GOLDEN, "tpolicy_grad.npz")) <= os.path.getsize(os.path.join(GOLDEN, "ppo_update.npz"))


def test_the_clamp_of_the_probabilities_is_float32_eps_in_every_dtype():
    """Categorical(probs=p) clamps at the dtype's eps; the kernel is f32, so the float64 yardstick clamps at float32's too. A head
    bias of -40 puts one action below it: its log-probability is log(2^-23), not log(p)."""
    c = R.case(17, 96, 2)
    import copy
    m = copy.deepcopy(c.model64)
    with torch.no_grad():
        m.actor.bias[1] = -40.0
    got = reference(m, c.args)
    q = got["probs"][:, 1]
    assert q.max() < 2.0 ** -23
    # the entropy's term of that action is -q log(eps), and the taken action's log-probability log(eps)
    zero = np.zeros(c.n, np.float32)
    own = reference(m, (c.boards, c.actions, zero, np.ones(c.n, np.float32), zero), clip_epsilon=1e9, entropy_coef=0.0, value_coef=0.0)
    rows = c.actions == 1
    others = got["probs"][~rows, :][np.arange((~rows).sum()), c.actions[~rows]]
    want_actor = -(np.where(rows, 2.0 ** -23, 0).sum() + others.sum()) / c.n
    assert abs(own["losses"][1] - want_actor) <= 1e-9, (own["losses"][1], want_actor)


def test_wrapper_checks_its_inputs_on_the_host():
    from g2048 import tpolicy
    n = 4
    good = dict(actions=torch.zeros(n, dtype=torch.int64), old_log_probs=torch.zeros(n), advantages=torch.zeros(n), returns=torch.zeros(n))
    tpolicy._check_loss_inputs(n, **good)
    with pytest.raises(TypeError, match="actions must be torch.int64"):
        tpolicy._check_loss_inputs(n, **dict(good, actions=torch.zeros(n, dtype=torch.int32)))
    with pytest.raises(ValueError, match="returns must have shape"):
        tpolicy._check_loss_inputs(n, **dict(good, returns=torch.zeros(n + 1)))
    with pytest.raises(TypeError, match="advantages must be torch.float32"):
        tpolicy._check_loss_inputs(n, **dict(good, advantages=torch.zeros(n, dtype=torch.float64)))
    from g2048 import DeviceQNetwork, DeviceTransformerPolicy
    from g2048._encoder_net import PackedNet
    for cls in (DeviceQNetwork, DeviceTransformerPolicy):           # one implementation for both networks
        for name in ("grad", "attach_grads", "attach_params", "params_attached", "refresh"):
            assert getattr(cls, name) is getattr(PackedNet, name), (cls.__name__, name)
