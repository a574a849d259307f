"""The transformer policy's training-mode dropout on the MI355X (csrc/g2048_tpolicy_train.hip, include/g2048_ttrain.h): the masks
against their NumPy restatement bit for bit, the loss and every gradient tensor against the STOCK module in .train() mode fed the
restated masks (tests/tpolicy_dropout_ref.py) in float64, the training-mode forward and advantages() against the same module,
p = 0 against the learner library's pass bit for bit, repeatability, guard bands round everything the two passes write, one closed
update() without a host synchronisation and as a captured graph, a NaN advantage, and the example.

Tolerance, the rule of tests/test_gpu_tpolicy_grad.py: for every gradient tensor max|g - g64| / max|g64| <= 8 x the worst such
ratio of the float32 masked module over the gradient tensors of the same case; loss parts, probs and value are held to the same
bound relative to their own maxima. tests/test_tpolicy_dropout_host.py asserts on the CPU that this yardstick lies in (0, 1e-5] and
that every case meets its conditions under the masks. Every measured multiple is printed; the figures of one MI355X run are in
docs/LOG.md R32."""
import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import guard
import tpolicy_dropout_ref as D
import tpolicy_grad_ref as R
import tpolicy_step_ref as T
from conftest import REPO
from test_gpu_tpolicy_grad import check, to_dev
from test_gpu_tpolicy_step import check_buffers, no_sync

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
bits = guard.bits


def drop_net(model32, p4=D.P4, seed=0, index=0, precision="f32"):
    from g2048 import DeviceTransformerPolicy
    net = DeviceTransformerPolicy(copy.deepcopy(model32).to(DEV).eval(), precision, dropout=p4, dropout_seed=seed)
    net.set_dropout_state((seed, index))
    return net


def outputs(net, result):
    """loss_and_grad's result and net.grad as test_gpu_tpolicy_grad.check takes them."""
    losses, probs, value = result
    grads, eps = R.split(net.parsed, net.grad.cpu().numpy())
    assert np.all(eps == 0) and len(eps) == 2 * net.n_layers, "a LayerNorm-eps slot of grad is not 0"
    f64 = lambda t: t.cpu().numpy().astype(np.float64)       # noqa: E731
    return dict(losses=f64(losses), probs=f64(probs), value=f64(value), grads=grads)


# ------------------------------------------------------------------------------------------------------------ 1: masks --
def mask_with_canary(n, layer, site, p, dim_ff, index, first=0, rows=None):
    from g2048 import ops
    height, width = D.site_shape(site, n, dim_ff)
    rows = height - first if rows is None else rows
    buf = torch.full((rows + 3, width), 7, dtype=torch.uint8, device=DEV)
    out = ops.tpolicy_dropout_mask(n, layer, site, p, dim_ff=dim_ff, seed=3, call_index=index, first_row=first, rows=rows, out=buf[:rows])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr() and torch.all(buf[rows:] == 7), "bytes past the window were written"
    want = D.keep_mask(3, index, layer, site, p, n, dim_ff, rows=(first, rows))
    got = out.cpu().numpy()
    assert set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got.astype(bool), want), "site %d of layer %d, n = %d, p = %g, call %d" % (site, layer, n, p, index)
    return got


@pytest.mark.parametrize("n", (1, 17, 33))
def test_masks_equal_the_restatement(n):
    for site in range(4):
        for layer in (0, 1):
            for dim_ff in (32, 96):
                for p, index in ((0.1, 5), (0.5, D.HIGH_INDEX)):
                    mask_with_canary(n, layer, site, p, dim_ff, index)
        height = D.site_shape(site, n, 96)[0]
        mask_with_canary(n, 1, site, 0.1, 96, D.HIGH_INDEX, first=height - 5, rows=5)          # a window that starts past row 0
    if n == 33:
        for p in (0.1, 0.5):
            keep = mask_with_canary(n, 0, 2, p, 2048, 5)
            sigma = (p * (1 - p) / keep.size) ** 0.5
            print("site 2, %d x 2048 at p = %g: kept share %.5f (1 - p +- 5 sigma = %.5f)" % (16 * n, p, keep.mean(), 5 * sigma))
            assert abs(keep.mean() - (1 - p)) < 5 * sigma


# ----------------------------------------------------------------------------------------------- 2: loss and gradients --
@pytest.mark.parametrize("case", D.LOSS_CASES, ids=D.case_id)
def test_loss_and_gradients_against_the_masked_float64_module(case):
    c = D.loss_case(case)
    c.conditions()
    net = drop_net(c.model32, c.p4, c.seed, c.index)
    got = outputs(net, net.loss_and_grad(*to_dev(*c.args)))
    check(got, c, "%s, dropout seed %d" % (D.case_id(case), c.seed))
    assert got["probs"].shape == (c.n, 4) and got["value"].shape == (c.n, 1) and net.dropout_state() == (c.seed, c.index + 1)


# ------------------------------------------------------------------------------------------- 3: the training-mode forward --
@pytest.mark.parametrize("shape", ((17, 96, 2), (33, 160, 1)), ids=("n17", "n33"))
def test_forward_dropout_against_the_masked_module_and_loss_and_grads_bits(shape):
    from g2048 import ops
    case = shape + (D.P4, D.INDEX)
    c = D.loss_case(case)
    want, f32 = (D.masked_forward(m, c.p4, c.seed, c.index, c.boards) for m in (c.train64, c.train32))
    net = drop_net(c.model32, c.p4, c.seed, c.index)
    probs, value = ops.tpolicy_forward_train(to_dev(c.boards)[0], net.plain, net.dim_ff, net.n_layers, c.p4, c.seed, c.index)
    for name, got, w64, w32 in (("probs", probs, want[0], f32[0]), ("value", value, want[1], f32[1])):
        yard, e = R.rel(w32, w64), R.rel(got.cpu().numpy(), w64)
        print("n = %d: %s %.3g of the largest = %.2f x the float32 masked module's own %.3g" % (c.n, name, e, e / yard, yard))
        assert 0 < yard <= D.FAIR_F32 and e <= R.F32_FACTOR * yard
    _, p2, v2 = net.loss_and_grad(*to_dev(*c.args))
    assert torch.equal(bits(probs), bits(p2)) and torch.equal(bits(value), bits(v2)), "the forward alone and the pass's forward differ"


# ------------------------------------------------------------------------------------------------------ 4: advantages --
@pytest.mark.parametrize("n", (17, 33))
def test_advantages_in_training_mode_against_the_same_lines_in_float64(n):
    import ppo_update_ref as P
    c = D.loss_case((17, 96, 2, D.P4, D.INDEX))
    boards, nxt = R.boards_of(n, 300 + n), R.boards_of(n, 600 + n)
    i = np.arange(n)
    rewards = (((11 * i) % 13 - 4) / 2.0 + boards[:, 1] / 4.0).astype(np.float32)
    dones = (i % 5 == 2).astype(np.float32)
    lines = {}
    for name, model in (("f64", c.train64), ("f32", c.train32)):
        v = D.masked_forward(model, D.P4, 5, 3, boards)[1].reshape(-1)
        nv = D.masked_forward(model, D.P4, 5, 4, nxt)[1].reshape(-1)
        lines[name] = P.advantage_lines(next(model.parameters()).dtype, v, nv, rewards, dones)
    bound = P.advantage_bound(lines["f32"], lines["f64"])
    net = drop_net(c.model32, D.P4, 5, 3)
    args = to_dev(boards, nxt, rewards, dones)
    returns, adv = (t.clone() for t in net.advantages(*args))
    assert net.dropout_state() == (5, 5), "two forwards, two indices"
    e = R.rel(returns.cpu().numpy(), lines["f64"][0]), R.rel(adv.cpu().numpy(), lines["f64"][1])
    print("training-mode advantages n=%d: returns %.3g, advantages %.3g (bound %.3g)" % (n, e[0], e[1], bound))
    assert returns.shape == adv.shape == (n,) and max(e) <= bound
    off = drop_net(c.model32, 0.0)
    today = [bits(t).clone() for t in off.advantages(*args)]
    assert off.dropout_index == 0
    evald = [t.clone() for t in net.advantages(*args, training=False)]
    assert all(torch.equal(bits(x), y) for x, y in zip(evald, today)) and net.dropout_index == 5, "training=False gives today's bits"
    moved = np.abs(evald[0].cpu().numpy() - returns.cpu().numpy()).max() / np.abs(lines["f64"][0]).max()
    print("    the eval-mode returns differ by %.3g of the largest" % moved)
    assert moved > 1e-3, "training mode must be on"
    forced = off.advantages(*args, training=True)                 # p = 0 through the training library: the f32 pass's forward
    assert off.dropout_index == 2 and R.rel(forced[0].cpu().numpy(), today[0].view(torch.float32).cpu().numpy()) <= bound


# --------------------------------------------------------------------------------------------------------- 5: p = 0 --
@pytest.mark.parametrize("shape", ((1, 32, 1), (17, 96, 2), (33, 160, 1)), ids=("n1", "n17", "n33"))
def test_p_zero_is_todays_pass_bit_for_bit(shape):
    """losses, probs, value and the whole grad: the *_dropout entry points with p = {0, 0, 0, 0} (a seed and an index that must
    not matter), ops with dropout = 0 and DeviceTransformerPolicy(dropout=0.0), against the learner library's entry point; and
    advantages() against today's."""
    from g2048 import DeviceTransformerPolicy, _lib as L, ops
    c = R.case(*shape)
    n = c.n
    net = DeviceTransformerPolicy(copy.deepcopy(c.model32).to(DEV).eval())
    args = to_dev(*c.args)
    want = [bits(x).clone() for x in ops.tpolicy_loss_grad(args[0], net.plain, *args[1:], net.dim_ff, net.n_layers)]
    lib, zeros = L.ttrain_lib(), (C.c_double * 4)(0.0, 0.0, 0.0, 0.0)
    floats = net.plain.numel()
    grad, losses, probs, value = (torch.full(s, float("nan"), device=DEV) for s in ((floats,), (4,), (n, 4), (n, 1)))
    nb = ops.tpolicy_train_workspace_bytes(n, net.dim_ff, net.n_layers)
    ws = torch.full((nb // 4,), float("nan"), device=DEV)
    f = C.c_float
    L.ttrain_call(net.device, lib.g2048_tpolicy_loss_grad_dropout, args[0].data_ptr(), net.plain.data_ptr(), args[1].data_ptr(),
                  args[2].data_ptr(), args[3].data_ptr(), args[4].data_ptr(), n, net.dim_ff, net.n_layers, zeros, 0xDEADBEEF, D.HIGH_INDEX,
                  f(R.CLIP), f(R.VALUE_COEF), f(R.ENTROPY_COEF), grad.data_ptr(), losses.data_ptr(), probs.data_ptr(), value.data_ptr(),
                  ws.data_ptr(), nb, L.stream_ptr(net.device))
    assert all(torch.equal(bits(x), y) for x, y in zip((losses, probs, value, grad), want)), "g2048_tpolicy_loss_grad_dropout at p = 0"
    probs.fill_(float("nan"))
    value.fill_(float("nan"))
    L.ttrain_call(net.device, lib.g2048_tpolicy_forward_dropout, args[0].data_ptr(), net.plain.data_ptr(), n, net.dim_ff, net.n_layers, zeros,
                  0xDEADBEEF, D.HIGH_INDEX, probs.data_ptr(), value.data_ptr(), ws.data_ptr(), nb, L.stream_ptr(net.device))
    assert torch.equal(bits(probs), want[1]) and torch.equal(bits(value), want[2]), "g2048_tpolicy_forward_dropout at p = 0"
    for dropout in (None, 0, 0.0, (0, 0, 0, 0)):
        got = ops.tpolicy_loss_grad(args[0], net.plain, *args[1:], net.dim_ff, net.n_layers, dropout=dropout, seed=5, call_index=6)
        assert all(torch.equal(bits(x), y) for x, y in zip(got, want))
    off = drop_net(c.model32, 0.0, seed=99)
    assert off.dropout == (0.0,) * 4
    got = list(off.loss_and_grad(*args)) + [off.grad]
    assert all(torch.equal(bits(x), y) for x, y in zip(got, want)) and off.dropout_index == 1, "the index counts with dropout 0 too"
    nxt, rewards, dones = to_dev(np.roll(c.boards, 1, axis=0), c.ret, (np.arange(n) % 3 == 0).astype(np.float32))
    today = [bits(t).clone() for t in net.advantages(args[0], nxt, rewards, dones)]
    assert all(torch.equal(bits(x), y) for x, y in zip(off.advantages(args[0], nxt, rewards, dones), today)) and off.dropout_index == 1


# ------------------------------------------------------------------------------------------------------ 6: repeatability --
def test_the_same_seed_and_index_give_the_same_bits_and_masks_belong_to_positions():
    c = D.loss_case((33, 160, 1, D.P4, D.INDEX))
    net = drop_net(c.model32, D.P4, c.seed, 7)
    args = to_dev(*c.args)
    first = [bits(x).clone() for x in net.loss_and_grad(*args)] + [bits(net.grad).clone()]
    net.set_dropout_state((c.seed, 7))
    net.grad.fill_(float("nan"))
    again = [bits(x).clone() for x in net.loss_and_grad(*args)] + [bits(net.grad).clone()]
    assert all(torch.equal(x, y) for x, y in zip(first, again)), "two calls with the same (seed, index) differ"
    assert net.dropout_state() == (c.seed, 8)
    nxt = [bits(x).clone() for x in net.loss_and_grad(*args)] + [bits(net.grad).clone()]
    assert not torch.equal(nxt[1], first[1]) and not torch.equal(nxt[3], first[3]), "the next index must draw other masks"
    fresh = drop_net(c.model32, D.P4, c.seed + 1, 7)
    assert not torch.equal(bits(fresh.loss_and_grad(*args)[1]), first[1]), "another seed must draw other masks"
    fresh.set_dropout_state((c.seed, 7))
    assert torch.equal(bits(fresh.loss_and_grad(*args)[1]), first[1]), "dropout_state() carries the masks to another network"
    # the boards permuted, the index kept: row perm[i] of the first call is now at position i, under position i's masks
    perm = np.random.default_rng(3).permutation(c.n)
    fresh.set_dropout_state((c.seed, 7))
    probs = fresh.loss_and_grad(*to_dev(*(np.ascontiguousarray(t[perm]) for t in c.args)))[1].cpu().numpy()
    before = first[1].view(torch.float32).reshape(c.n, 4).cpu().numpy()
    moved = np.abs(probs - before[perm]).max()
    print("permuted boards under the same index: a row's probabilities move by up to %.3g" % moved)
    assert moved > 1e-3, "the masks belong to positions, not to boards"


# ------------------------------------------------------------------------------------------------------ 7: guard bands --
@pytest.mark.parametrize("shape", [(17, 96, 2), (1024, 32, 2)], ids=["n17-ff96-L2", "limit"])
def test_guard_bands_round_everything_the_two_passes_write(shape):
    """The two-run protocol of tests/guard.py round g2048_tpolicy_loss_grad_dropout and g2048_tpolicy_forward_dropout: grad, the
    outputs and the workspace (of exactly the size the query gives) between bands that must stay intact, poison in the inputs'
    bands, and both runs bit-equal: nothing outside what the call was given reaches a result, and no workspace element is read
    before the call wrote it."""
    from g2048 import ops
    c = D.loss_case(shape + (D.P4, D.INDEX))
    net = drop_net(c.model32)
    n, floats = c.n, net.plain.numel()
    nb = ops.tpolicy_train_workspace_bytes(n, net.dim_ff, net.n_layers)

    def call(s):
        boards = s.inp("boards", c.boards, align=16)
        plain = s.inp("plain", net.plain, align=16)
        actions = s.inp("actions", c.args[1])
        old, adv, ret = s.inp("old_log_probs", c.args[2]), s.inp("advantages", c.args[3]), s.inp("returns", c.args[4])
        grad = s.out("grad", floats, (), torch.float32, align=16)
        losses = s.out("losses", 4, (), torch.float32)
        probs = s.out("probs", n, (4,), torch.float32, align=16)
        value = s.out("value", n, (1,), torch.float32)
        ws = s.out("workspace", nb, (), torch.uint8, align=16)
        fprobs = s.out("forward probs", n, (4,), torch.float32, align=16)
        fvalue = s.out("forward value", n, (1,), torch.float32)
        fws = s.out("forward workspace", nb, (), torch.uint8, align=16)
        ops.tpolicy_loss_grad(boards, plain, actions, old, adv, ret, net.dim_ff, net.n_layers, grad=grad, losses=losses, probs=probs,
                              value=value, workspace=ws, dropout=c.p4, seed=c.seed, call_index=c.index)
        ops.tpolicy_forward_train(boards, plain, net.dim_ff, net.n_layers, c.p4, c.seed, c.index, probs=fprobs, value=fvalue, workspace=fws)
        return dict(grad=grad, losses=losses, probs=probs, value=value, fprobs=fprobs, fvalue=fvalue)

    out = guard.twice(DEV, call)
    grads, eps = R.split(net.parsed, out["grad"].numpy())
    assert np.all(eps == 0)
    f64 = lambda t: t.numpy().astype(np.float64)       # noqa: E731
    check(dict(losses=f64(out["losses"]), probs=f64(out["probs"]), value=f64(out["value"]), grads=grads), c, "guarded, n=%d" % n)
    assert guard.same_bits(out["fprobs"], out["probs"]) and guard.same_bits(out["fvalue"], out["value"])


# ----------------------------------------------------------------------------------------------------- 8: a closed update --
def full_buffer(parsed, params, like):
    """A reference vector over the parameters as a buffer in the plain layout: the eps slots are `like`'s."""
    slices, _, total = R.plain_slices(parsed)
    out, o = np.array(like, dtype=np.float64), 0
    assert out.shape == (total,)
    for at, k in slices:
        out[at:at + k] = params[o:o + k]
        o += k
    return out


def test_one_closed_update_without_a_host_synchronisation_and_as_a_graph():
    """update(epochs=2) at N = 48 with torch's synchronisation check set to raise, against the masked stock float64 module stepping
    through tests/tpolicy_step_ref.py's Adam with the same index sequence (0, 1: the advantage block; 2, 3: the epochs): per epoch
    the gradients to the bound, the weights and moments after each step to tests/test_gpu_tpolicy_step.py's bound. update() leaves
    the bits of its parts called one by one. Then the update as a captured graph, replayed twice from restored weights, moments
    and counters: the eager run's bits."""
    base, inputs = D.update_inputs()
    returns64, adv64, want = D.closed_update(torch.float64)
    f32 = D.closed_update(torch.float32)[2]
    dev_in = to_dev(*inputs)
    boards, actions, old, rewards, nxt, dones = dev_in
    kw = dict(lr=D.UPDATE_LR, max_norm=T.MAX_NORM, betas=T.BETAS, eps=T.EPS)
    twin = drop_net(base.model32)
    eps_at = T.eps_slots(twin.dim_ff, twin.n_layers)
    state = lambda net: [net.plain, net.grad, net.exp_avg, net.exp_avg_sq]       # noqa: E731
    with no_sync():
        ret, adv = twin.advantages(boards, nxt, rewards, dones, D.GAMMA)
        kept = []
        for e in range(D.UPDATE_EPOCHS):
            losses, probs, value = twin.loss_and_grad(boards, actions, old, adv, ret)
            pre = [t.clone() for t in state(twin)]
            norm = twin.adam_step(losses, **kw)
            kept.append([t.clone() for t in (losses, probs, value, norm)] + [pre, [t.clone() for t in state(twin)]])
    torch.cuda.synchronize()
    assert twin.dropout_index == 2 + D.UPDATE_EPOCHS == 4 and twin.opt_counters.tolist() == [D.UPDATE_EPOCHS, 0, 0]
    e_adv = R.rel(ret.cpu().numpy(), returns64), R.rel(adv.cpu().numpy(), adv64)
    print("closed update: returns %.3g, advantages %.3g of their largest" % e_adv)
    for e, ((losses, probs, value, norm, pre, post), w64, w32) in enumerate(zip(kept, want, f32)):
        grads, eps = R.split(twin.parsed, pre[1].cpu().numpy())
        assert np.all(eps == 0)
        f64 = lambda t: t.cpu().numpy().astype(np.float64)       # noqa: E731
        yard = float(R.ratios(w32["grads"], w64["grads"]).max())
        assert 0 < yard <= D.FAIR_F32
        r = R.ratios(grads, w64["grads"])
        others = [R.rel(f64(losses), w64["losses"]), R.rel(f64(probs), w64["probs"]), R.rel(f64(value), w64["value"])]
        print("epoch %d: gradients %.3g of max|g| = %.2f x the float32 masked module's %.3g; losses %.2f x, probs %.2f x, value %.2f x"
              % (e, r.max(), r.max() / yard, yard, others[0] / yard, others[1] / yard, others[2] / yard))
        assert r.max() <= R.F32_FACTOR * yard and max(others) <= R.F32_FACTOR * yard, "epoch %d" % e
        post_cpu = [t.cpu() for t in post]
        truth = tuple(full_buffer(twin.parsed, w64[k], post_cpu[i].numpy()) if k else None
                      for i, k in enumerate(("params", None, "exp_avg", "exp_avg_sq")))
        check_buffers([t.cpu() for t in pre], post_cpu, eps_at, e + 1, "closed update, step %d" % (e + 1), want=truth, lr=D.UPDATE_LR)
        assert abs(float(norm) - w64["norm"]) <= 4 * R.F32_FACTOR * yard * w64["norm"]

    net = drop_net(base.model32)
    start = [t.clone() for t in state(net)] + [net.opt_counters.clone()]

    def restore():
        for t, t0 in zip(state(net) + [net.opt_counters], start):
            t.copy_(t0)
        net._plain_changed()
        net.set_dropout_state((0, 0))

    net.update(*dev_in, epochs=D.UPDATE_EPOCHS, gamma=D.GAMMA, **kw)             # the warm-up call: buffers are allocated
    restore()
    with no_sync():
        losses, norms = net.update(*dev_in, epochs=D.UPDATE_EPOCHS, gamma=D.GAMMA, **kw)
    torch.cuda.synchronize()
    assert net.dropout_index == 4
    eager = [bits(t).clone() for t in state(net) + [net.opt_counters, net.packed, losses, norms]]
    for name, a, b in zip(("plain", "grad", "exp_avg", "exp_avg_sq"), eager, state(twin)):
        assert torch.equal(a, bits(b)), "update() and its parts called one by one leave other bits in %s" % name
    assert all(torch.equal(bits(losses[e]), bits(k[0])) for e, k in enumerate(kept))

    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        net.update(*dev_in, epochs=D.UPDATE_EPOCHS, gamma=D.GAMMA, **kw)         # this stream's buffers exist before the capture
        restore()
        side.synchronize()
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            glosses, gnorms = net.update(*dev_in, epochs=D.UPDATE_EPOCHS, gamma=D.GAMMA, **kw)
    torch.cuda.current_stream(DEV).wait_stream(side)
    assert net.dropout_index == 4
    names = ("plain", "grad", "exp_avg", "exp_avg_sq", "opt_counters", "packed", "losses", "norms")
    for replay in range(2):
        restore()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = [bits(t) for t in state(net) + [net.opt_counters, net.packed, glosses, gnorms]]
        differ = ["%s (%d of %d elements, the first at %s: %s for %s)" % (k, int((x != y).sum()), x.numel(), (x != y).reshape(-1).nonzero()[:4, 0].tolist(),
                                                                     x.reshape(-1)[(x != y).reshape(-1)][:4].tolist(), y.reshape(-1)[(x != y).reshape(-1)][:4].tolist())
                  for k, x, y in zip(names, got, eager) if not torch.equal(x, y)]
        assert not differ, "replay %d of the captured update is not the eager run, bit for bit: %s" % (replay, ", ".join(differ))


# ------------------------------------------------------------------------------------------------------ 9: a NaN advantage --
def test_a_nan_advantage_gives_a_nan_loss_and_the_step_is_skipped():
    c = D.loss_case((17, 96, 2, D.P4, D.INDEX))
    adv = c.adv.copy()
    adv[-1] = np.nan
    args = (c.boards, c.args[1], c.args[2], adv, c.args[4])
    want = D.masked_loss_grad(c.train32, c.p4, c.seed, c.index, *args)
    net = drop_net(c.model32, c.p4, c.seed, c.index)
    before = [t.clone() for t in (net.plain, net.exp_avg, net.exp_avg_sq)]
    losses, _, _ = net.loss_and_grad(*to_dev(*args))
    assert bool(torch.isnan(losses[0])) == bool(np.isnan(want["losses"][0])) is True
    net.adam_step(losses)
    assert net.opt_counters.tolist() == [0, 1, 0], "a NaN loss skips the step and is counted"
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip((net.plain, net.exp_avg, net.exp_avg_sq), before))


# -------------------------------------------------------------------------------------------------------- 10: the example --
def test_the_example_runs_with_dropout():
    script = os.path.join(REPO, "examples", "tpolicy_update.py")
    out = subprocess.run([sys.executable, script, "--dropout", "0.1", "--optimizer", "device"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "dropout (0.1, 0.1, 0.1, 0.1)" in out.stdout, out.stdout[-2000:]
