"""The Q-network's training-mode dropout on the MI355X (csrc/g2048_qnet_train.hip, include/g2048_train.h): the masks against their
NumPy restatement bit for bit, p = 0 against the main library's passes bit for bit, the loss and every gradient tensor against the
STOCK module in .train() mode fed the restated masks (tests/qnet_dropout_ref.py) in float64, the training forwards and the
Double-DQN targets against the same modules, repeatability, one closed round of train_step without a host synchronisation and as
a captured graph, a poisoned row, and the example.

Tolerance, the rule of tests/test_gpu_qnet_grad.py: for every gradient tensor max|g - g64| / max|g64| <= 8 x the worst such ratio
of the float32 masked module over the gradient tensors of the same case; the loss, td and q are held to the same bound relative to
their own maxima. tests/test_qnet_dropout_host.py asserts on the CPU that this yardstick lies in (0, 1e-5] in every case. Every
measured multiple is printed.

Measured on an MI355X over the 20 loss-and-gradient cases: 0.45 - 1.40 x the case's yardstick (4.6e-7 .. 1.8e-6), at most 2.86 x a
tensor's own float32 error, loss at most 0.20 x, td 0.49 x, q 0.02 - 0.06 of the bound; the training forwards' q 0.56 - 0.92 x the
float32 masked module's own error; the closed round 0.74 and 0.80 x, its weights 0.38 and 0.40 of their bound. Five mutated builds
of the training library (a wrong site, call index, layer, element index, a multiplier left out) each fail 16 - 21 of the 36 tests
here; per case in docs/LOG.md R28.1."""
import contextlib
import copy
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import qnet_dropout_ref as D
import qnet_grad_ref as R
from conftest import REPO
from test_gpu_qnet_grad import check, split, to_dev

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = D.DROPOUT_SEED


def drop_net(model, p4=D.P4, seed=SEED, index=0):
    from g2048 import DeviceQNetwork
    net = DeviceQNetwork(copy.deepcopy(model).float().eval().to(DEV), dropout=p4, dropout_seed=seed)
    net.set_dropout_state((seed, index))
    return net


def bits(t):
    return t.detach().contiguous().view(torch.uint8).reshape(-1).clone() if t.dim() else t.detach().reshape(1).view(torch.uint8).clone()


@contextlib.contextmanager
def no_sync():
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


# ------------------------------------------------------------------------------------------------------------ 1: masks --
def mask_with_canary(n, layer, site, p, dim_ff, index, first=0, rows=None):
    from g2048 import ops
    height, width = D.site_shape(site, n, dim_ff)
    rows = height - first if rows is None else rows
    buf = torch.full((rows + 3, width), 7, dtype=torch.uint8, device=DEV)
    out = ops.qnet_dropout_mask(n, layer, site, p, dim_ff=dim_ff, seed=SEED + 3, call_index=index, first_row=first, rows=rows, out=buf[:rows])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr() and torch.all(buf[rows:] == 7), "bytes past the window were written"
    want = D.keep_mask(SEED + 3, index, layer, site, p, n, dim_ff, rows=(first, rows))
    got = out.cpu().numpy()
    assert set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got.astype(bool), want), "site %d of layer %d, n = %d, p = %g, call %d" % (site, layer, n, p, index)


@pytest.mark.parametrize("n", (1, 2, 16, 17, 33, 257))
def test_masks_equal_the_restatement(n):
    for site in range(4):
        for layer in (0, 2):
            for p in (0.1, 0.5):
                for index in (5, D.HIGH_INDEX):
                    mask_with_canary(n, layer, site, p, 64, index)


def test_masks_at_the_batch_limit_through_the_row_window():
    n = 4096
    for site, height in ((0, 8 * n), (2, n)):
        for first in (0, height - 16):
            mask_with_canary(n, 1, site, 0.1, 2048, D.HIGH_INDEX, first=first, rows=16)


# --------------------------------------------------------------------------------------------------------- 2: p = 0 --
@pytest.mark.parametrize("n", (1, 17, 257))
def test_p_zero_is_todays_pass_bit_for_bit(n):
    """q, loss, td and the whole grad: the *_dropout entry points with p = {0, 0, 0, 0} (a seed and an index that must not matter),
    DeviceQNetwork(dropout=0.0) and ops with dropout=0, against the main library's entry points."""
    import ctypes as C
    from g2048 import _lib as L, ops
    from test_gpu_qnet_batch import device_net
    model, boards, a, t, w = D.loss_case(("early", D.EARLY_SHAPES[0], n, D.P4, 7))[:5]
    net = device_net(model)
    args = to_dev(boards, a, t, w)
    want = [bits(x) for x in ops.qnet_loss_grad(args[0], net.plain, *args[1:], net.dim_ff, net.n_layers)]
    want_q = bits(ops.qnet_forward_batch(args[0], net.plain, net.dim_ff, net.n_layers))
    assert torch.equal(want_q, want[2])
    T, zeros = L.train_lib(), (C.c_double * 4)(0.0, 0.0, 0.0, 0.0)
    floats = net.plain.numel()
    grad, td, q, loss = (torch.full(s, float("nan"), device=DEV) for s in ((floats,), (n,), (n, 4), ()))
    ws = torch.full((ops.qnet_train_workspace_bytes(n, net.dim_ff, net.n_layers) // 4,), float("nan"), device=DEV)
    L.train_call(net.device, T.g2048_qnet_loss_grad_dropout, args[0].data_ptr(), net.plain.data_ptr(), args[1].data_ptr(), args[2].data_ptr(),
                 args[3].data_ptr(), n, net.dim_ff, net.n_layers, zeros, 0xDEADBEEF, D.HIGH_INDEX, grad.data_ptr(), td.data_ptr(), loss.data_ptr(),
                 q.data_ptr(), ws.data_ptr(), L.stream_ptr(net.device))
    assert all(torch.equal(bits(x), y) for x, y in zip((loss, td, q, grad), want)), "g2048_qnet_loss_grad_dropout at p = 0"
    q.fill_(float("nan"))
    L.train_call(net.device, T.g2048_qnet_forward_batch_dropout, args[0].data_ptr(), net.plain.data_ptr(), q.data_ptr(), n, net.dim_ff,
                 net.n_layers, zeros, 0xDEADBEEF, D.HIGH_INDEX, ws.data_ptr(), L.stream_ptr(net.device))
    assert torch.equal(bits(q), want_q), "g2048_qnet_forward_batch_dropout at p = 0"
    for dropout in (0, 0.0, (0, 0, 0, 0)):
        got = ops.qnet_loss_grad(args[0], net.plain, *args[1:], net.dim_ff, net.n_layers, dropout=dropout, seed=5, call_index=6)
        assert all(torch.equal(bits(x), y) for x, y in zip(got, want))
        assert torch.equal(bits(ops.qnet_forward_batch(args[0], net.plain, net.dim_ff, net.n_layers, dropout=dropout, seed=5, call_index=6)), want_q)
    off = drop_net(model, 0.0, seed=99)
    assert off.dropout == (0.0,) * 4
    loss, td, q = off.loss_and_grad(*args)
    assert all(torch.equal(bits(x), y) for x, y in zip((loss, td, q, off.grad), want))
    assert torch.equal(bits(off.forward_batch(args[0], training=True)), want_q) and torch.equal(bits(off.forward_batch(args[0])), want_q)
    assert off.dropout_index == 2, "the index counts the training forwards with dropout 0 too"


# ----------------------------------------------------------------------------------------------- 3: loss and gradients --
def run_with_canaries(net, boards, a, t, w, p4, seed, index):
    """ops.qnet_loss_grad with dropout into padded outputs and a workspace that held NaN, none of whose spare room may be touched:
    (loss, td, q, per-tensor gradients) as float64 NumPy."""
    from g2048 import ops
    n, floats = len(boards), net.plain.numel()
    b, da, dt, dw = to_dev(boards, a, t, w)
    nb = ops.qnet_train_workspace_bytes(n, net.dim_ff, net.n_layers)
    grad = torch.full((floats + 64,), 7.0, device=DEV)
    td, q = torch.full((n + 67,), 7.0, device=DEV), torch.full((n + 67, 4), 7.0, device=DEV)
    loss = torch.full((3,), 7.0, device=DEV)
    ws = torch.full((nb // 4 + 1024,), float("nan"), device=DEV)
    ops.qnet_loss_grad(b, net.plain, da, dt, dw, net.dim_ff, net.n_layers, grad=grad[:floats], td=td[:n], loss=loss[:1].view(()), q=q[:n],
                       workspace=ws.view(torch.uint8)[:nb], dropout=p4, seed=seed, call_index=index)
    torch.cuda.synchronize()
    assert torch.all(grad[floats:] == 7.0) and torch.all(td[n:] == 7.0) and torch.all(q[n:] == 7.0) and torch.all(loss[1:] == 7.0), n
    assert torch.all(torch.isnan(ws[nb // 4:])), "bytes past the workspace were written (n = %d)" % n
    grads, eps = split(net, grad[:floats])
    assert np.all(eps == 0) and len(eps) == 2 * net.n_layers, "the LayerNorm-eps slots of grad must be 0"
    return float(loss[0]), td[:n].cpu().numpy().astype(np.float64), q[:n].cpu().numpy().astype(np.float64), grads


def check_q(q, want_q, bound, what):
    e = np.abs(q - want_q).max() / np.abs(want_q).max()
    print("    %s: q %.3g of max|q| = %.2f of the bound" % (what, e, e / bound))
    assert e <= bound, what


@pytest.mark.parametrize("case", D.LOSS_CASES, ids=[D.case_id(c) for c in D.LOSS_CASES])
def test_loss_and_gradients_against_the_masked_float64_module(case):
    from test_gpu_qnet_batch import device_net
    kind, shape, n, p4, index = case
    model, boards, a, t, w, want, f32 = D.loss_case(case)
    net = device_net(model)
    got = run_with_canaries(net, boards, a, t, w, p4, SEED, index)
    bound = check(got, want, f32, True, D.case_id(case))
    assert 0 < bound / R.F32_FACTOR <= D.FAIR_F32
    check_q(got[2], want[2], bound, D.case_id(case))
    if n == 17:                                                     # through the wrapper: the same bits
        wrapped = drop_net(model, p4, SEED, index)
        loss, td, q = wrapped.loss_and_grad(*to_dev(boards, a, t, w))
        grads, _ = split(wrapped, wrapped.grad)
        assert float(loss) == got[0] and all(np.array_equal(x, y) for x, y in zip(grads, got[3])) and wrapped.dropout_index == index + 1


# ------------------------------------------------------------------------------------- 4: the forwards and the targets --
@pytest.mark.parametrize("n", D.FORWARD_SIZES)
def test_training_forwards_and_targets_against_the_masked_modules(n):
    import g2048
    from g2048 import ops
    online_m, target_m, boards, shaped, dones, ((q_on, q_t), (f_on, f_t)) = D.forward_case(n)
    online, target = drop_net(online_m, D.P4, SEED, 3), drop_net(target_m, D.P4, SEED + 1, 5)
    b, ds, dd = to_dev(boards, shaped, dones)
    # the entry point with canaries
    nb = ops.qnet_batch_workspace_bytes(n, online.dim_ff)
    q = torch.full((n + 67, 4), 7.0, device=DEV)
    ws = torch.full((nb // 4 + 1024,), float("nan"), device=DEV)
    ops.qnet_forward_batch(b, online.plain, online.dim_ff, online.n_layers, q=q[:n], workspace=ws.view(torch.uint8)[:nb], dropout=D.P4, seed=SEED,
                           call_index=3)
    torch.cuda.synchronize()
    assert torch.all(q[n:] == 7.0) and torch.all(torch.isnan(ws[nb // 4:]))
    bounds = []
    for name, got, want, f32 in (("online", q[:n].cpu().numpy().astype(np.float64), q_on, f_on),
                                 ("target", target.forward_batch(b, training=True).cpu().numpy().astype(np.float64), q_t, f_t)):
        yard = np.abs(f32 - want).max() / np.abs(want).max()
        e = np.abs(got - want).max() / np.abs(want).max()
        print("n = %d, %s network: q %.3g of max|q| = %.2f x the float32 masked module's %.3g" % (n, name, e, e / yard, yard))
        assert 0 < yard <= D.FAIR_F32 and e <= R.F32_FACTOR * yard
        bounds.append(R.F32_FACTOR * yard)
    assert torch.equal(online.forward_batch(b, training=True), q[:n]) and (online.dropout_index, target.dropout_index) == (4, 6)
    eval_q = online.forward_batch(b).cpu().numpy()
    assert np.abs(eval_q - q_on).max() > 1e-3 * np.abs(q_on).max() and online.dropout_index == 4, "training=False stays eval mode"
    # dqn_targets(training=True): the same two forwards again, from the same indices
    online.set_dropout_state((SEED, 3))
    target.set_dropout_state((SEED + 1, 5))
    targets, next_actions = g2048.dqn_targets(online, target, b, ds, dd, D.GAMMA, training=True)
    assert (online.dropout_index, target.dropout_index) == (4, 6)
    want_t, want_a, margin = D.dqn_targets_of(q_on, q_t, shaped, dones)
    sure = margin > 2 * bounds[0] * np.abs(q_on).max()
    got_a = next_actions.cpu().numpy()
    assert sure.sum() > n // 2 and np.array_equal(got_a[sure], want_a[sure])
    same = got_a == want_a
    e = np.abs(targets.cpu().numpy().astype(np.float64) - want_t)[same].max() / np.abs(want_t).max()
    print("n = %d: targets %.3g of their maximum (bound %.3g), %d of %d actions decided by a margin above the bound" % (n, e, max(bounds), sure.sum(), n))
    assert e <= max(bounds) * max(1.0, np.abs(q_t).max() / np.abs(want_t).max())


# ------------------------------------------------------------------------------------------------------ 5: repeatability --
def test_the_same_seed_and_index_give_the_same_bits_and_the_next_index_other_masks():
    model, boards, a, t, w = D.loss_case(("early", D.EARLY_SHAPES[0], 257, D.P4, 7))[:5]
    net = drop_net(model, D.P4, SEED, 7)
    args = to_dev(boards, a, t, w)
    first = [bits(x) for x in net.loss_and_grad(*args)] + [bits(net.grad)]
    net.set_dropout_state((SEED, 7))
    net.grad.fill_(float("nan"))
    again = [bits(x) for x in net.loss_and_grad(*args)] + [bits(net.grad)]
    assert all(torch.equal(x, y) for x, y in zip(first, again)), "two calls with the same (seed, index) differ"
    assert net.dropout_state() == (SEED, 8)
    nxt = [bits(x) for x in net.loss_and_grad(*args)]
    assert not torch.equal(nxt[2], first[2]), "the next index must draw other masks"
    fresh = drop_net(model, D.P4, SEED + 1, 7)
    assert not torch.equal(bits(fresh.loss_and_grad(*args)[2]), first[2]), "another seed must draw other masks"
    fresh.set_dropout_state((SEED, 7))
    assert torch.equal(bits(fresh.loss_and_grad(*args)[2]), first[2]), "dropout_state() carries the masks to another network"
    with pytest.raises(ValueError, match="negative"):
        fresh.set_dropout_state((SEED, -1))
    with pytest.raises(ValueError, match="bf16"):
        from g2048 import DeviceQNetwork
        DeviceQNetwork(copy.deepcopy(model).float().eval().to(DEV), precision="bf16", dropout=0.1).forward_batch(args[0], training=True)


# ----------------------------------------------------------------------------------------------------- 6: a closed round --
def per_tensor(flat, sizes):
    out, o = [], 0
    for k in sizes:
        out.append(flat[o:o + k])
        o += k
    return out


def test_one_closed_round_without_a_host_synchronisation_and_as_a_graph():
    """sample-shaped inputs -> dqn_targets(training=True) -> loss_and_grad -> adamw_step, twice, with torch's synchronisation check
    set to raise, against the masked float64 modules and g2048.qnet.adamw_step_reference (tests/qnet_dropout_ref.py closed_round);
    the bound per step is 8 x the float32 masked modules' own deviation in the same step (for the weights never tighter than
    2^-23 max|p|). Then the same round captured as a graph: every replay from the same weights draws the same masks."""
    import g2048
    from test_qnet_host import random_model
    (boards, next_boards, actions, weights, shaped, dones), want = D.closed_round(torch.float64)
    f32 = D.closed_round(torch.float32)[1]
    mseed, dim_ff, layers = D.EARLY_SHAPES[0]
    online = drop_net(D.case_model("early", D.EARLY_SHAPES[0])[0], D.P4, SEED)
    target = drop_net(random_model(mseed + 1, dim_ff, layers), D.P4, SEED + 1)
    online.attach_params()
    target.attach_params()
    b, nb, a, w, s, d = to_dev(boards, next_boards, actions, weights, shaped, dones)
    start = [t.clone() for t in (online.plain, online.exp_avg, online.exp_avg_sq)]
    torch.cuda.synchronize()
    kept = []
    with no_sync():
        for step in range(D.ROUND_STEPS):
            targets, next_a = g2048.dqn_targets(online, target, nb, s, d, D.GAMMA, training=True)
            loss, td, q = online.loss_and_grad(b, a, targets, w)
            grad = online.grad.clone()                               # adamw_step leaves the gradient clipped
            norm = online.adamw_step(D.ROUND_LR)
            kept.append([t.clone() for t in (targets, next_a, loss, td, q, grad, online.plain, norm)])
    torch.cuda.synchronize()
    assert (online.dropout_index, target.dropout_index, online.opt_step) == (2 * D.ROUND_STEPS, D.ROUND_STEPS, D.ROUND_STEPS)
    sizes = [p.numel() for p in online.model.parameters()]
    for k, ((targets, next_a, loss, td, q, grad, plain, norm), w64, w32) in enumerate(zip(kept, want, f32)):
        assert np.array_equal(next_a.cpu().numpy(), w64["next_actions"]), "step %d: margins %.3g" % (k + 1, w64["margin"].min())
        grads, _ = split(online, grad)
        got = (float(loss), td.cpu().numpy().astype(np.float64), q.cpu().numpy().astype(np.float64), grads)
        bound = check(got, (w64["loss"], w64["td"], w64["q"], w64["grads"]), (w32["loss"], w32["td"], w32["q"], w32["grads"]), True,
                      "closed round, step %d" % (k + 1))
        assert 0 < bound / R.F32_FACTOR <= D.FAIR_F32
        check_q(got[2], w64["q"], bound, "step %d" % (k + 1))
        e_t = np.abs(targets.cpu().numpy() - w64["targets"]).max() / np.abs(w64["targets"]).max()
        assert e_t <= bound, "step %d: targets %.3g of their maximum" % (k + 1, e_t)
        params, _ = split(online, plain)
        worst = 0.0
        for p, p64, p32 in zip(params, per_tensor(w64["params"], sizes), per_tensor(w32["params"], sizes)):
            tol = max(R.F32_FACTOR * np.abs(p32 - p64).max(), 2.0 ** -23 * np.abs(p64).max())
            worst = max(worst, np.abs(p - p64).max() / tol)
        print("    step %d: targets %.2f of the bound, weights after AdamW at most %.2f of their bound, norm %.6g (float64 %.6g)"
              % (k + 1, e_t / bound, worst, float(norm), w64["norm"]))
        assert worst <= 1.0 and abs(float(norm) - w64["norm"]) <= bound * w64["norm"] * 4
    # the round as a captured graph: the call indices are launch scalars, so every replay draws the masks of the capture
    def restore():
        for t, t0 in zip((online.plain, online.exp_avg, online.exp_avg_sq), start):
            t.copy_(t0)
        online._plain_changed()
    restore()
    online.set_dropout_state((SEED, 0))
    target.set_dropout_state((SEED + 1, 0))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        for _ in range(2):                                           # the buffers of this stream exist before the capture
            targets, _ = g2048.dqn_targets(online, target, nb, s, d, D.GAMMA, training=True)
            online.loss_and_grad(b, a, targets, w)
            online.adamw_step(D.ROUND_LR, step=1)
        restore()
        online.set_dropout_state((SEED, 0))
        target.set_dropout_state((SEED + 1, 0))
        side.synchronize()
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            targets, _ = g2048.dqn_targets(online, target, nb, s, d, D.GAMMA, training=True)
            loss, td, q = online.loss_and_grad(b, a, targets, w)
            online.adamw_step(D.ROUND_LR, step=1)
    torch.cuda.current_stream(DEV).wait_stream(side)
    replays = []
    for _ in range(2):
        restore()
        g.replay()
        torch.cuda.synchronize()
        replays.append([bits(t) for t in (targets, loss, td, q, online.plain)])
    assert all(torch.equal(x, y) for x, y in zip(*replays)), "two replays from the same weights differ"
    first = kept[0]
    assert all(torch.equal(x, bits(y)) for x, y in zip(replays[0], (first[0], first[2], first[3], first[4], first[6]))), \
        "the captured round is not the eager first step, bit for bit"


# ------------------------------------------------------------------------------------------------------ 7: a poisoned row --
def test_a_poisoned_row_shows_as_in_the_masked_float32_module():
    """One board's target is +inf at n = 17: the set of non-finite gradient tensors, and the class of the loss, are the masked
    float32 stock module's."""
    import warnings
    case = ("early", D.EARLY_SHAPES[0], 17, D.P4, 7)
    model, boards, a, t, w = D.loss_case(case)[:5]
    t = t.copy()
    t[5] = np.inf
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f32 = D.masked_loss_grad(D.training_copy(model, D.P4, torch.float32), D.P4, SEED, 7, boards, a, t, w)
    net = drop_net(model, D.P4, SEED, 7)
    loss, td, q = net.loss_and_grad(*to_dev(boards, a, t, w))
    grads, _ = split(net, net.grad)
    cls = lambda v: "nan" if np.isnan(v) else "inf" if np.isinf(v) else "finite"
    bad = lambda gs: [bool(~np.isfinite(g).all()) for g in gs]
    print("target +inf: loss %s (stock float32 %s), td[5] %s; non-finite gradient tensors %d (stock %d)"
          % (cls(float(loss)), cls(f32[0]), cls(float(td[5])), sum(bad(grads)), sum(bad(f32[3]))))
    assert cls(float(loss)) == cls(f32[0]) and bad(grads) == bad(f32[3])
    assert np.array_equal(np.isfinite(td.cpu().numpy()), np.isfinite(f32[1]))


# --------------------------------------------------------------------------------------------------------- 8: the example --
def test_the_example_runs_with_dropout():
    script = os.path.join(REPO, "examples", "dqn_replay.py")
    out = subprocess.run([sys.executable, script, "--envs", "256", "--steps", "16", "--capacity", "4096", "--batch", "64", "--dim-ff", "64", "--train",
                          "--device-step", "--dropout", "0.1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = re.search(r"last weighted Huber loss (\S+)", out.stdout)
    assert line and np.isfinite(float(line.group(1))), out.stdout[-2000:]
    counts = re.search(r"dropout \(0\.1, 0\.1, 0\.1, 0\.1\): (\d+) training forwards of the online network, (\d+) of the target network", out.stdout)
    assert counts and int(counts.group(1)) == 2 * int(counts.group(2)) > 0, out.stdout[-2000:]
