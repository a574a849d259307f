"""g2048_qnet_loss_grad on the MI355X: the loss and the gradients of every parameter against the stock module's float64 autograd
through the lines of train_step (random-init modules at every tile edge, with canaries) and against the reference class's
recorded gradients (tests/golden/qnet_grad.npz), q bit for bit against forward_batch, repeatability and a poisoned workspace, zero
weights, a permuted batch, and attach_grads() with a stock optimiser.

Tolerance, the f32 convention of test_gpu_qnet_batch.py applied per case: for every checked tensor max|g - g64| / max|g64| <= 8 x
the worst such ratio of the stock module's float32 CPU autograd over the checked tensors of the same case; loss and td are held
to the same bound relative to their own maxima. The measured multiples are printed.

Two kinds of case. On EARLY boards (codes 0..3, tiles <= 8) every parameter is checked. On FULL boards (tiles up to 131,072)
layer 0's attention logits reach 1e9 and its softmax is nearly one-hot: at n >= 2 the gradients that pass through it (cnn.*,
embedding.*, layer 0's in_proj_*) are no float32 quantity -- stock float32 autograd is off by up to eight times the gradient
there -- so they are asserted finite and their error is printed, and the other parameters are checked. At n = 1 the softmax is
exactly 1 and all of them are checked."""
import copy
import functools

import numpy as np
import pytest
import torch

import qnet_grad_ref as R
from conftest import load_golden
from test_gpu_qnet_batch import RAGGED, case_boards, device_net
from test_policy_host import random_boards
from test_qnet_host import golden_model, random_model

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(2, 64, 2), (12, 32, 1)]
IDS = ["ff64-L2", "ff32-L1"]
FULL_SIZES = (1, 17, 257)


def to_dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in arrays)


@functools.lru_cache(maxsize=None)
def random_case(seed, dim_ff, layers, kind):
    """A random-init module and, per size, its boards and inputs with the stock module's CPU float64 and float32 loss and
    gradients (shared, never modified). kind: 'early' (every ragged size) or 'full' (FULL_SIZES)."""
    model = random_model(seed, dim_ff, layers)
    boards = (random_boards(max(RAGGED), 9 + seed) % 4).astype(np.uint8) if kind == "early" else case_boards(max(RAGGED), 9 + seed)
    m64, m32 = copy.deepcopy(model).double(), copy.deepcopy(model).float()
    cases = {}
    for n in (RAGGED if kind == "early" else FULL_SIZES):
        a, t, w = R.case_inputs(m64, boards[:n])
        cases[n] = (a, t, w, R.stock_loss_grad(m64, boards[:n], a, t, w), R.stock_loss_grad(m32, boards[:n], a, t, w))
    return m32, boards, cases


def split(net, grad):
    slices, eps, total = R.plain_slices(net.parsed)
    g = grad.cpu().numpy().astype(np.float64)
    assert g.shape == (total,)
    return [g[o:o + k] for o, k in slices], g[eps]


def check(got, want, f32, every, what):
    """got, want, f32: (loss, td, q, grads). Asserts the bound on the checked tensors (all of them, or those downstream of layer
    0's softmax), on loss and on td; returns the relative bound 8 x the case's float32 error."""
    first = 0 if every else R.N_UPSTREAM
    r, y = R.ratios(got[3], want[3]), R.ratios(f32[3], want[3])
    yard = y[first:].max()
    bound = R.F32_FACTOR * yard
    worst = first + int(np.argmax(r[first:]))
    e_loss, e_td = abs(got[0] - want[0]) / abs(want[0]), np.abs(got[1] - want[1]).max() / np.abs(want[1]).max()
    print("%s: gradients %.3g of max|g| (tensor %d) = %.2f x the CPU-f32 error %.3g (bound %.0f x); loss %.2f x, td %.2f x%s"
          % (what, r[worst], worst, r[worst] / yard, yard, R.F32_FACTOR, e_loss / yard, e_td / yard,
             "" if every else "; upstream of the layer-0 softmax, not checked: %.3g (CPU f32: %.3g)" % (r[:first].max(), y[:first].max())))
    assert all(np.all(np.isfinite(g)) for g in got[3]) and np.isfinite(got[0]) and np.all(np.isfinite(got[1])), what
    assert yard > 0 and r[first:].max() <= bound, what
    assert e_loss <= bound and e_td <= bound, what
    return bound


def run(net, boards, a, t, w):
    """loss_and_grad through the wrapper: (loss, td, q, per-tensor gradients) as float64 NumPy."""
    loss, td, q = net.loss_and_grad(*to_dev(boards, a, t, w))
    grads, eps = split(net, net.grad)
    assert np.all(eps == 0), "a LayerNorm-eps slot of grad is not 0"
    return float(loss), td.cpu().numpy().astype(np.float64), q.cpu().numpy().astype(np.float64), grads


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_tile_edges_with_canaries(shape):
    from g2048 import ops
    model, boards, cases = random_case(*shape, "early")
    net = device_net(model)
    floats = net.plain.numel()
    for n in RAGGED:
        a, t, w, want, f32 = cases[n]
        b, da, dt, dw = to_dev(boards[:n], a, t, w)
        nb = ops.qnet_grad_workspace_bytes(n, net.dim_ff, net.n_layers)
        grad = torch.full((floats + 64,), 7.0, device=DEV)
        td, q = torch.full((n + 67,), 7.0, device=DEV), torch.full((n + 67, 4), 7.0, device=DEV)
        loss = torch.full((3,), 7.0, device=DEV)
        ws = torch.full((nb + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
        ops.qnet_loss_grad(b, net.plain, da, dt, dw, net.dim_ff, net.n_layers, grad=grad[:floats], td=td[:n], loss=loss[:1].view(()), q=q[:n],
                           workspace=ws[:nb])
        torch.cuda.synchronize()
        assert torch.all(grad[floats:] == 7.0) and torch.all(td[n:] == 7.0) and torch.all(q[n:] == 7.0) and torch.all(loss[1:] == 7.0), n
        assert torch.all(ws[nb:] == 0xA5), "bytes past the workspace were written (n = %d)" % n
        assert torch.equal(q[:n], net.forward_batch(b)), "q is not forward_batch's, bit for bit (n = %d)" % n
        grads, eps = split(net, grad[:floats])
        assert np.all(eps == 0) and len(eps) == 2 * net.n_layers, "the LayerNorm-eps slots of grad must be 0"
        got = (float(loss[0]), td[:n].cpu().numpy().astype(np.float64), None, grads)
        check(got, want, f32, True, "early boards, dim_ff %d L %d n=%d" % (net.dim_ff, net.n_layers, n))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_full_boards(shape):
    model, boards, cases = random_case(*shape, "full")
    net = device_net(model)
    for n in FULL_SIZES:
        a, t, w, want, f32 = cases[n]
        check(run(net, boards[:n], a, t, w), want, f32, n == 1, "full boards, dim_ff %d L %d n=%d" % (net.dim_ff, net.n_layers, n))


@functools.lru_cache(maxsize=None)
def fixture_net():
    _, policy_boards, model = golden_model()
    return load_golden("qnet_grad.npz"), policy_boards, device_net(model)


def test_reference_class_gradients_on_the_fixture_weights():
    g, policy_boards, net = fixture_net()
    assert net.dim_ff == 2048 and net.n_layers == 2
    pos = g["positions"]
    for case in g["cases"].tolist():
        n = int(case.split("_")[1])
        early = case.startswith("early")
        boards = g["early_boards"][:n] if early else policy_boards[:n]
        a, _, w = R.recipe(n)
        loss, td, q, grads = run(net, boards, a, g[case + "_targets"], w)
        first = 0 if early else R.N_UPSTREAM
        gmax = g[case + "_gmax_f64"]
        r = np.array([np.abs(x[p] - want).max() for x, p, want in zip(grads, pos, g[case + "_g_f64"])]) / gmax
        y = np.abs(g[case + "_g_f32"].astype(np.float64) - g[case + "_g_f64"]).max(axis=1) / gmax
        yard = y[first:].max()
        bound = R.F32_FACTOR * yard
        e_loss = abs(loss - float(g[case + "_loss_f64"])) / float(g[case + "_loss_f64"])
        e_td = np.abs(td - g[case + "_td_f64"]).max() / g[case + "_td_f64"].max()
        # |norm - norm64| <= |g - g64|_2 <= sqrt(numel) max|g - g64|: what the bound on the entries implies for the whole tensor
        numel = np.array([x.size for x in grads])
        e_norm = np.abs(np.array([np.linalg.norm(x) for x in grads]) - g[case + "_norm_f64"]) / (np.sqrt(numel) * gmax)
        worst = first + int(np.argmax(r[first:]))
        print("%s: sampled gradients %.3g of max|g| (%s) = %.2f x the CPU-f32 error %.3g; norms %.2f x, loss %.2f x, td %.2f x%s"
              % (case, r[worst], g["tensor_names"][worst], r[worst] / yard, yard, e_norm[first:].max() / yard, e_loss / yard, e_td / yard,
                 "" if early else "; upstream of the layer-0 softmax, not checked: %.3g (CPU f32: %.3g)" % (r[:first].max(), y[:first].max())))
        assert all(np.all(np.isfinite(x)) for x in grads)
        assert r[first:].max() <= bound and e_norm[first:].max() <= bound and e_loss <= bound and e_td <= bound, case
        assert np.abs(q - g[case + "_q_f64"]).max() <= 1e-4 * np.abs(g[case + "_q_f64"]).max()


def test_repeatable_and_nothing_accumulates():
    from g2048 import ops
    g, policy_boards, fixture = fixture_net()
    model, boards, cases = random_case(2, 64, 2, "early")
    small = device_net(model)
    a256, _, w256 = R.recipe(256)
    for net, codes, (a, t, w) in ((small, boards[:17], cases[17][:3]), (small, boards[:257], cases[257][:3]),
                                  (fixture, policy_boards[:256], (a256, g["full_256_targets"], w256))):
        n = len(codes)
        args = to_dev(codes, a, t, w)
        first = [x.clone() for x in net.loss_and_grad(*args)] + [net.grad.clone()]
        again = list(net.loss_and_grad(*args)) + [net.grad]
        assert all(torch.equal(x, y) for x, y in zip(first, again)), "two calls differ (n = %d)" % n
        nb = ops.qnet_grad_workspace_bytes(n, net.dim_ff, net.n_layers)
        ws = torch.full((nb // 4,), float("nan"), device=DEV)
        grad = torch.full_like(net.grad, float("nan"))
        out = ops.qnet_loss_grad(*args[:1], net.plain, *args[1:], net.dim_ff, net.n_layers, grad=grad, workspace=ws.view(torch.uint8))
        assert all(torch.equal(x, y) for x, y in zip(first, out)), "NaN in grad or in the workspace before the call changes the result (n = %d)" % n
        ws.fill_(float("nan"))
        grad.fill_(float("nan"))
        out = ops.qnet_loss_grad(*args[:1], net.plain, *args[1:], net.dim_ff, net.n_layers, grad=grad, workspace=ws.view(torch.uint8))
        assert all(torch.equal(x, y) for x, y in zip(first, out))


def test_zero_weights_and_a_permuted_batch():
    model, boards, cases = random_case(2, 64, 2, "early")
    net = device_net(model)
    n = 257
    a, t, w, want, f32 = cases[n]
    loss, td, _ = net.loss_and_grad(*to_dev(boards[:n], a, t, np.zeros(n, np.float32)))
    assert float(loss) == 0.0 and torch.all(net.grad == 0), "zero weights must give a zero loss and exactly zero gradients"
    assert np.abs(td.cpu().numpy() - want[1]).max() <= 1e-4 * want[1].max()
    got = run(net, boards[:n], a, t, w)
    bound = check(got, want, f32, True, "n=%d" % n)
    perm = np.random.default_rng(3).permutation(n)
    gp = run(net, boards[:n][perm], a[perm], t[perm], w[perm])
    diff = R.ratios(gp[3], want[3]), abs(gp[0] - want[0]) / abs(want[0]), np.abs(gp[1] - want[1][perm]).max() / want[1].max()
    moved = max(np.abs(x - y).max() / np.abs(z).max() for x, y, z in zip(gp[3], got[3], want[3]))
    print("permuted batch: gradients %.3g of max|g| from float64, %.3g from the unpermuted call (bound %.3g)" % (diff[0].max(), moved, bound))
    assert diff[0].max() <= bound and diff[1] <= bound and diff[2] <= bound and moved <= bound
    assert np.abs(gp[2] - got[2][perm]).max() <= 1e-4 * np.abs(got[2]).max()


def test_attach_grads_feeds_a_stock_optimiser():
    model, boards, cases = random_case(2, 64, 2, "early")
    net = device_net(model)
    m = net.model
    assert net.attach_grads() is net.grad and net.grad.shape == net.plain.shape and net.grad.dtype == torch.float32
    lo, hi = net.grad.data_ptr(), net.grad.data_ptr() + 4 * net.grad.numel()
    slices, _, _ = R.plain_slices(net.parsed)
    params = [x for x in net.parsed.plain_tensors() if isinstance(x, torch.Tensor)]
    assert len(params) == len(list(m.parameters())) and set(map(id, params)) == set(map(id, m.parameters()))
    for n in (33, 17):                                           # the second call lands in the same views: no copy
        a, t, w = cases[n][:3]
        net.loss_and_grad(*to_dev(boards[:n], a, t, w))
        for p, (o, k) in zip(params, slices):
            assert p.grad.data_ptr() == lo + 4 * o and p.grad.data_ptr() + 4 * k <= hi and p.grad.shape == p.shape
            assert torch.equal(p.grad.reshape(-1), net.grad[o:o + k])
    grads, _ = split(net, net.grad)
    check((cases[17][3][0], cases[17][3][1], None, grads), cases[17][3], cases[17][4], True, "through param.grad, n=17")
    whole = float(net.grad.norm())
    norm = float(torch.nn.utils.clip_grad_norm_(m.parameters(), 10.0))
    assert abs(norm - whole) <= 1e-6 * whole, (norm, whole)
    b = to_dev(boards[:17])[0]
    before, plain = net.forward_batch(b).clone(), net.plain.clone()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
    opt.step()
    assert torch.equal(net.plain, plain) and torch.equal(net.forward_batch(b), before), "the weights moved without refresh()"
    net.refresh()
    assert not torch.equal(net.plain, plain)
    step = (net.plain - plain).abs().max()
    assert 0.5e-3 < float(step) < 1.5e-3, "one AdamW step at lr 1e-3 moves a weight by about 1e-3 (got %.3g)" % float(step)
    from g2048 import qnet
    cpu = copy.deepcopy(m).cpu()
    want = qnet.forward_batch_reference(qnet.parse(cpu.double()), torch.from_numpy(boards[:17])).numpy()
    after = net.forward_batch(b).cpu().numpy().astype(np.float64)
    assert np.abs(after - want).max() <= 1e-4 * np.abs(want).max() and np.abs(after - before.cpu().numpy()).max() > 1e-3
