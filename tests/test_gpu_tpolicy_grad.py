"""g2048_tpolicy_loss_grad on the MI355X (DeviceTransformerPolicy.loss_and_grad): PPOAgent.update()'s loss on the transformer
policy's two heads and the gradient of every parameter against the stock module's float64 autograd, at the 16-row tile edge, at
the row-split weight gradient's chunk edge, at the reference's shape and at the limit of 1,024 boards; the reference class's
recorded gradients (tests/golden/tpolicy_grad.npz); guard bands round everything the entry point writes; the refusal past the
limit; repeatability and a permuted batch; attach_grads() + clip_grad_norm_ + a stock Adam + refresh(); advantages(); a NaN
advantage.

Tolerance (tests/tpolicy_grad_ref.py, the project's own from tests/ppo_update_ref.py): per tensor max|g - g64| / max|g64| <= 8 x the
worst such ratio of stock CPU float32 autograd on the same inputs; loss parts, probs and value to the same bound relative to their
maxima. Every case but N = 1 and N = 2 has the clipped branch binding on 10 .. 90 % of its rows and no zero gradient tensor
(asserted). The measured multiples are printed per case.

Measured on an MI355X: the worst gradient tensor of a case 0.08 - 1.36 x the case's yardstick (4.3e-7 .. 2.7e-6), loss parts at most
0.51 x, probs 0.82 x, value 1.98 x; the fixture 0.77 x; per case in docs/LOG.md R29.1, with the six one-line faults this file catches."""
import copy

import numpy as np
import pytest
import torch

import guard
import tpolicy_grad_ref as R
from conftest import load_golden
from test_gpu_policy import TOL
from test_tpolicy_host import golden_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDS = ["n%d-ff%d-L%d" % c for c in R.GPU_CASES]


def to_dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in arrays)


def device_net(model32, precision="f32"):
    from g2048 import DeviceTransformerPolicy
    return DeviceTransformerPolicy(copy.deepcopy(model32).to(DEV).eval(), precision)


def run(net, args, **kw):
    """loss_and_grad through the wrapper: dict(losses, probs, value, grads per tensor) as float64 NumPy."""
    losses, probs, value = net.loss_and_grad(*to_dev(*args), **kw)
    grads, eps = R.split(net.parsed, net.grad.cpu().numpy())
    assert np.all(eps == 0) and len(eps) == 2 * net.n_layers, "a LayerNorm-eps slot of grad is not 0"
    f64 = lambda t: t.cpu().numpy().astype(np.float64)       # noqa: E731
    return dict(losses=f64(losses), probs=f64(probs), value=f64(value), grads=grads)


def check(got, c, what):
    """The bound on every gradient tensor, on the loss parts, probs and value; returns the worst multiple of the yardstick."""
    r = R.ratios(got["grads"], c.want["grads"])
    worst = int(np.argmax(r))
    others = dict(losses=R.rel(got["losses"], c.want["losses"]), probs=R.rel(got["probs"], c.want["probs"]),
                  value=R.rel(got["value"], c.want["value"]))
    print("%s: gradients %.3g of max|g| (tensor %d) = %.2f x the CPU-f32 error %.3g (bound %.0f x); losses %.2f x, probs %.2f x, value "
          "%.2f x; clipped share %.2f" % (what, r[worst], worst, r[worst] / c.yardstick, c.yardstick, R.F32_FACTOR,
                                          others["losses"] / c.yardstick, others["probs"] / c.yardstick, others["value"] / c.yardstick,
                                          c.clipped_share))
    assert all(np.all(np.isfinite(g)) for g in got["grads"]) and np.all(np.isfinite(got["losses"])), what
    assert all(np.abs(g).max() > 0 for g in got["grads"]), "%s: a gradient tensor is zero" % what
    assert r.max() <= c.bound, "%s: tensor %d is %.2f x the yardstick" % (what, worst, r[worst] / c.yardstick)
    for k, v in others.items():
        assert v <= c.bound, "%s: %s is %.2f x the yardstick" % (what, k, v / c.yardstick)
    return r[worst] / c.yardstick


@pytest.mark.parametrize("shape", R.GPU_CASES, ids=IDS)
def test_loss_and_gradients_against_the_float64_module(shape):
    c = R.case(*shape)
    c.conditions()
    net = device_net(c.model32)
    got = run(net, c.args)
    check(got, c, "n=%d dim_ff %d L %d" % shape)
    assert got["probs"].shape == (c.n, 4) and got["value"].shape == (c.n, 1)


def test_bf16_acting_blob_changes_nothing():
    """The pass is f32 and reads net.plain, whatever precision the acting blob was packed in: the same bits."""
    c = R.case(17, 96, 2)
    a, b = device_net(c.model32, "f32"), device_net(c.model32, "bf16")
    ra = [t.clone() for t in a.loss_and_grad(*to_dev(*c.args))] + [a.grad.clone()]
    rb = list(b.loss_and_grad(*to_dev(*c.args))) + [b.grad]
    assert all(torch.equal(x, y) for x, y in zip(ra, rb))


def test_reference_class_gradients_on_the_recipe_weights():
    """The golden fixture: the reference's own TransformerModel on the weights of tests/tpolicy_weights.py, 32 boards of policy.npz."""
    g = load_golden("tpolicy_grad.npz")
    _, model = golden_model()
    net = device_net(model.float())
    args = (g["boards"], g["actions"], g["old_log_probs"], g["advantages"], g["returns"])
    got = run(net, args)
    names = g["tensor_names"].tolist()
    r = np.array([np.abs(x[R.golden_positions(x.size)] - g["grad." + k]).max() / g["gmax"][i] for i, (k, x) in enumerate(zip(names, got["grads"]))])
    yard = float(g["yardstick_f32"])
    bound = R.F32_FACTOR * yard
    worst = int(np.argmax(r))
    e = [R.rel(got[k], g[k + "_f64"]) for k in ("losses", "probs", "value")]
    print("fixture: sampled gradients %.3g of max|g| (%s) = %.2f x the CPU-f32 error %.3g; losses %.2f x, probs %.2f x, value %.2f x"
          % (r[worst], names[worst], r[worst] / yard, yard, e[0] / yard, e[1] / yard, e[2] / yard))
    assert yard > 0 and r.max() <= bound and max(e) <= bound


@pytest.mark.parametrize("shape", [(17, 96, 2), (1024, 32, 2)], ids=["n17-ff96-L2", "limit"])
def test_guard_bands_round_everything_the_entry_point_writes(shape):
    """The two-run protocol of tests/guard.py: grad, the four outputs and the workspace between bands that must stay intact,
    poison in the inputs' bands, and both runs (bands and prefill of 0x00 / 0x3C, then 0xFF / 0xC3) bit-equal: nothing outside
    what the call was given reaches a result, and no workspace element is read before the call wrote it."""
    from g2048 import ops
    c = R.case(*shape)
    net = device_net(c.model32)
    n, floats = c.n, net.plain.numel()
    nb = ops.tpolicy_grad_workspace_bytes(n, net.dim_ff, net.n_layers)

    def call(s):
        boards = s.inp("boards", c.boards, align=16)
        plain = s.inp("plain", net.plain, align=16)
        actions = s.inp("actions", c.actions)
        old, adv, ret = s.inp("old_log_probs", c.old), s.inp("advantages", c.adv), s.inp("returns", c.ret)
        grad = s.out("grad", floats, (), torch.float32, align=16)
        losses = s.out("losses", 4, (), torch.float32)
        probs = s.out("probs", n, (4,), torch.float32, align=16)
        value = s.out("value", n, (1,), torch.float32)
        ws = s.out("workspace", nb, (), torch.uint8, align=16)
        ops.tpolicy_loss_grad(boards, plain, actions, old, adv, ret, net.dim_ff, net.n_layers, grad=grad, losses=losses, probs=probs,
                              value=value, workspace=ws)
        return dict(grad=grad, losses=losses, probs=probs, value=value)

    out = guard.twice(DEV, call)
    grads, eps = R.split(net.parsed, out["grad"].numpy())
    assert np.all(eps == 0)
    f64 = lambda t: t.numpy().astype(np.float64)       # noqa: E731
    check(dict(losses=f64(out["losses"]), probs=f64(out["probs"]), value=f64(out["value"]), grads=grads), c, "guarded, n=%d" % n)


def test_more_than_the_limit_is_refused_with_the_limit_named():
    c = R.case(17, 96, 2)
    net = device_net(c.model32)
    n = 1025
    boards = torch.zeros((n, 16), dtype=torch.uint8, device=DEV)
    z = torch.zeros(n, device=DEV)
    before = net.grad.clone()
    with pytest.raises(ValueError, match="1024"):
        net.loss_and_grad(boards, torch.zeros(n, dtype=torch.int64, device=DEV), z, z, z)
    from g2048 import ops
    with pytest.raises(ValueError, match="1024"):
        ops.tpolicy_loss_grad(boards, net.plain, torch.zeros(n, dtype=torch.int64, device=DEV), z, z, z, net.dim_ff, net.n_layers)
    assert torch.equal(net.grad, before)
    empty = net.loss_and_grad(boards[:0], torch.zeros(0, dtype=torch.int64, device=DEV), z[:0], z[:0], z[:0])
    assert empty[1].shape == (0, 4) and torch.equal(net.grad, before), "N = 0 launches nothing"


def test_two_calls_give_the_same_bits_and_the_order_of_the_boards_does_not_matter():
    c = R.case(33, 160, 1)
    net = device_net(c.model32)
    args = to_dev(*c.args)
    first = [t.clone() for t in net.loss_and_grad(*args)] + [net.grad.clone()]
    ptrs = [t.data_ptr() for t in net.loss_and_grad(*args)]
    again = list(net.loss_and_grad(*args)) + [net.grad]
    assert all(torch.equal(x, y) for x, y in zip(first, again)), "two calls differ"
    assert ptrs == [t.data_ptr() for t in again[:3]], "the outputs are the network's own, one set per (N, stream)"
    got = run(net, c.args)
    perm = np.random.default_rng(3).permutation(c.n)
    gp = run(net, tuple(np.ascontiguousarray(t[perm]) for t in c.args))
    moved = max(np.abs(x - y).max() / np.abs(z).max() for x, y, z in zip(gp["grads"], got["grads"], c.want["grads"]))
    dl = np.abs(gp["losses"] - got["losses"]).max() / np.abs(c.want["losses"]).max()
    print("permuted batch: loss parts moved by %.3g, gradients by %.3g of max|g| (bound %.3g)" % (dl, moved, c.bound))
    assert dl <= c.bound and moved <= c.bound
    assert np.abs(gp["probs"] - got["probs"][perm]).max() <= c.bound and R.rel(gp["value"], got["value"][perm]) <= c.bound


def test_attached_views_clipping_a_stock_adam_step_and_refresh():
    """attach_params() / attach_grads() make the module's tensors views of net.plain / net.grad; loss_and_grad,
    clip_grad_norm_, one stock Adam step on the views and refresh() against the same step on a stock float32 copy driven by
    stock autograd. The step's bound is test_front_end_attached_adam_step_and_policy_refresh's (tests/test_gpu_ppo_update.py):
    Adam's first step is lr . g / (|g| + eps), whose slope in g is at most lr / eps, so with lr = eps the step's error is at most
    the gradient's, bound x max|g| (the clipping factor is at most 1), plus the float32 rounding of the updated weight (2^-23 max|p|)
    and of the step's own arithmetic (4 x 2^-23 max|step|). net(boards) then agrees with the updated module within the forward's
    existing tolerance."""
    from g2048 import tpolicy
    lr = eps = 0.05
    max_norm = 0.5
    c = R.case(17, 96, 2)
    net = device_net(c.model32)
    m = net.model
    assert net.attach_params() is net.plain and net.params_attached
    assert net.attach_grads() is net.grad and net.grad.shape == net.plain.shape
    slices, _, _ = R.plain_slices(net.parsed)
    params = [t for t in net.parsed.plain_tensors() if isinstance(t, torch.Tensor)]
    assert [id(p) for p in params] == [id(p) for p in m.parameters()]
    for p, (o, k) in zip(params, slices):
        assert p.data_ptr() == net.plain.data_ptr() + 4 * o and p.grad.data_ptr() == net.grad.data_ptr() + 4 * o
    got = run(net, c.args)
    check(got, c, "attached, n=17")
    stock = copy.deepcopy(c.model32)
    f32 = R.stock_loss_grad(stock, *c.args)
    for p, g in zip(stock.parameters(), f32["grads"]):
        p.grad = torch.from_numpy(g.astype(np.float32)).view(p.shape)
    old_p = [p.detach().cpu().numpy().astype(np.float64) for p in params]
    norms = float(torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm)), float(torch.nn.utils.clip_grad_norm_(stock.parameters(), max_norm))
    assert abs(norms[0] - norms[1]) <= 1e-4 * norms[1] and norms[1] > max_norm, norms      # both sides are clipped
    b = to_dev(c.boards)[0]
    before = [t.clone() for t in net(b)]
    torch.optim.Adam(m.parameters(), lr=lr, eps=eps).step()
    torch.optim.Adam(stock.parameters(), lr=lr, eps=eps).step()
    assert all(torch.equal(x, y) for x, y in zip(net(b), before)), "the acting blob moved without refresh()"
    worst = 0.0
    for k, (p, q, o) in enumerate(zip(params, stock.parameters(), old_p)):
        step, want = p.detach().cpu().numpy().astype(np.float64) - o, q.detach().numpy().astype(np.float64) - o
        gmax, top = np.abs(c.want["grads"][k]).max(), np.abs(want).max()
        tol = (lr / eps) * c.bound * gmax + 2.0 ** -23 * np.abs(o).max() + 4 * 2.0 ** -23 * top
        err = np.abs(step - want).max()
        worst = max(worst, err / tol)
        assert top > 0 and err <= tol, "tensor %d: step error %.3g, tolerance %.3g (max|step| %.3g)" % (k, err, tol, top)
    print("one clipped Adam step on the views: at most %.2f of the tolerance" % worst)
    net.refresh()
    assert net.params_attached
    p64, v64 = tpolicy.forward_reference(tpolicy.parse(copy.deepcopy(m).cpu().double()), torch.from_numpy(c.boards))
    probs, value = net(b)
    assert np.abs(probs.cpu().numpy() - p64.numpy()).max() <= TOL["f32"]["probs"]
    assert np.abs(value.cpu().numpy() - v64.numpy()).max() <= TOL["f32"]["values"] * np.abs(v64.numpy()).max()
    assert np.abs(probs.cpu().numpy() - before[0].cpu().numpy()).max() > 1e-3, "a step of 0.05 must move the policy"


@pytest.mark.parametrize("n", (1, 2, 17, 1024))
def test_advantages_against_the_same_lines_in_float64(n):
    """ppo_agent.py:357-373 with this network's critic head against stock torch float64, the MLP learner's bound formula
    (tests/ppo_update_ref.py advantage_bound: 8 x stock float32's own error, at least 8 float32 roundings)."""
    import ppo_update_ref as P
    c = R.case(17, 96, 2)
    net = device_net(c.model32)
    boards, nxt = R.boards_of(n, 300 + n), R.boards_of(n, 600 + n)
    i = np.arange(n)
    rewards = (((11 * i) % 13 - 4) / 2.0 + boards[:, 1] / 4.0).astype(np.float32)
    dones = (i % 5 == 2).astype(np.float32)
    lines = {}
    for name, model in (("f64", c.model64), ("f32", c.model32)):
        dtype = next(model.parameters()).dtype
        with torch.no_grad():
            v = model(torch.from_numpy(boards).to(dtype) / 15)[1].reshape(-1).numpy()
            nv = model(torch.from_numpy(nxt).to(dtype) / 15)[1].reshape(-1).numpy()
        lines[name] = P.advantage_lines(dtype, v, nv, rewards, dones)
    bound = P.advantage_bound(lines["f32"], lines["f64"])
    returns, adv = net.advantages(*to_dev(boards, nxt, rewards, dones))
    e = R.rel(returns.cpu().numpy(), lines["f64"][0]), R.rel(adv.cpu().numpy(), lines["f64"][1])
    print("advantages n=%d: returns %.3g, advantages %.3g (bound %.3g)" % (n, e[0], e[1], bound))
    assert returns.shape == adv.shape == (n,) and max(e) <= bound
    if n == 1:
        assert abs(float(adv[0]) - (float(returns[0]) - float(net(to_dev(boards)[0])[1][0, 0]))) <= 1e-6 * max(1.0, abs(float(returns[0])))


def test_a_nan_advantage_gives_a_nan_loss_as_torch_does():
    c = R.case(17, 96, 2)
    net = device_net(c.model32)
    adv = c.adv.copy()
    adv[-1] = np.nan
    args = (c.boards, c.actions, c.old, adv, c.ret)
    want = R.stock_loss_grad(c.model32, *args)
    losses, _, _ = net.loss_and_grad(*to_dev(*args))
    assert bool(torch.isnan(losses[0])) == bool(np.isnan(want["losses"][0])) is True
