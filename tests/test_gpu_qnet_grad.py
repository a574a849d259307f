"""g2048_qnet_loss_grad on the MI355X: the loss and the gradients of every parameter against the stock module's float64 autograd
through the lines of train_step (random-init modules at every tile edge, with canaries) and against the reference class's
recorded gradients (tests/golden/qnet_grad.npz), q bit for bit against forward_batch, repeatability and a poisoned workspace, zero
weights, a permuted batch, attach_grads() with a stock optimiser, the shape matrix of test_gpu_qnet_batch.py (a main group
followed by tail steps in the forward's products and in dX, a third layer, the sizes up to G2048_QNET_BATCH_MAX), and its
peaked-attention cases (a layer-0 softmax that is neither uniform nor one-hot, with canaries and repeatability).

Tolerance, the f32 convention of test_gpu_qnet_batch.py applied per case: for every checked tensor max|g - g64| / max|g64| <= 8 x
the worst such ratio of the stock module's float32 CPU autograd over the checked tensors of the same case; loss and td are held
to the same bound relative to their own maxima. The measured multiples are printed, and below them every checked tensor's error
as a multiple of that tensor's OWN float32 error (not asserted: it shows how much slack the shared yardstick leaves). On the shape
matrix's early boards the yardstick itself must lie in (0, 1e-5].

Measured on an MI355X over the shape matrix (early boards): 0.49 - 2.14 x the case's yardstick, at most 5.67 x a tensor's own float32
error (out_proj.weight at n = 4,096); dim_ff 160 with 3 layers on full boards 0.78 x (n = 1) and 0.47 x (n = 17). The yardstick at
the batch limit sits just under the fairness bound: 5.6e-6 (n = 2,049), 9.6e-6 (4,095), 6.6e-6 (4,096), and it depends on the CPU's
thread count (docs/LOG.md R19.1).

Three kinds of case. On EARLY boards (codes 0..3, tiles <= 8) every parameter is checked; layer 0's attention is uniform there
(logits <= 0.3, max P = 1 / n), so its backward's dS is next to nothing. On FULL boards (tiles up to 131,072) layer 0's attention
logits reach 1e9 and its softmax is nearly one-hot: at n >= 2 the gradients that pass through it (cnn.*, embedding.*, layer 0's
in_proj_*) are no float32 quantity -- stock float32 autograd is off by up to eight times the gradient there -- so they are asserted
finite and their error is printed, and the other parameters are checked. At n = 1 the softmax is exactly 1 and all of them are
checked. The PEAKED-ATTENTION cases (REGIME_CASES of test_gpu_qnet_batch.py) lie in between, every parameter checked and the
yardstick held to (0, 1e-5]: 'mid' boards (codes 0..7: mean max-P 0.19 - 0.31), full boards under the 'conditioned' module
(cnn[0].weight x 2^-10: codes up to 17 in conv1's weight gradient, logits -111 .. 37, max-P about 2 / n) and 'distinct' (mid, three
layers whose tensors differ from layer to layer, which a fresh nn.TransformerEncoder's do not), at n = 17, 257 and 1,025 (four
boards per thread in conv1's weight gradient). tests/test_qnet_grad_host.py asserts on the CPU that the cases are in these regimes.

Measured on an MI355X over the peaked-attention cases: 0.50 - 1.93 x the case's yardstick (8.1e-7 .. 4.2e-6), at most 3.86 x a
tensor's own float32 error (layer 0's in_proj_weight, mid boards at n = 1,025); per case in docs/LOG.md R22.1."""
import copy
import functools

import numpy as np
import pytest
import torch

import qnet_grad_ref as R
from conftest import load_golden
from test_gpu_qnet_batch import (FAIR_F32, MATRIX_CASES, MATRIX_IDS, MODEL_SEED, RAGGED, REGIME_CASES, REGIME_IDS, REGIMES, case_boards,
                                 device_net, matrix_boards, matrix_net, regime_boards, regime_model, regime_net)
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


@functools.lru_cache(maxsize=None)
def matrix_case(dim_ff, layers, n, kind):
    """(boards, actions, targets, weights, the stock module's CPU float64 and float32 loss and gradients) of a case of the shape
    matrix of test_gpu_qnet_batch.py (shared, never modified)."""
    model = random_model(MODEL_SEED, dim_ff, layers)
    boards = matrix_boards(n, kind)
    m64, m32 = copy.deepcopy(model).double(), copy.deepcopy(model).float()
    a, t, w = R.case_inputs(m64, boards)
    return boards, a, t, w, R.stock_loss_grad(m64, boards, a, t, w), R.stock_loss_grad(m32, boards, a, t, w)


@functools.lru_cache(maxsize=None)
def regime_case(regime, dim_ff, layers, n):
    """matrix_case for a peaked-attention case of test_gpu_qnet_batch.py ('mid' boards, or full boards under the conditioned
    module); the float64 module comes last for the regime test of test_qnet_grad_host.py (shared, never modified)."""
    model = regime_model(regime, dim_ff, layers)
    boards = regime_boards(regime, n)
    m64, m32 = copy.deepcopy(model).double(), copy.deepcopy(model).float()
    a, t, w = R.case_inputs(m64, boards)
    return boards, a, t, w, R.stock_loss_grad(m64, boards, a, t, w), R.stock_loss_grad(m32, boards, a, t, w), m64


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
    # not asserted: how much slack the shared yardstick leaves. 0/0 (both exact) counts as 0, x/0 as inf
    with np.errstate(divide="ignore", invalid="ignore"):
        own = np.where(r[first:] > 0, r[first:] / y[first:], 0.0)
    print("    every checked tensor against its OWN CPU-f32 error: max %.2f x (tensor %d); %s"
          % (own.max(), first + int(np.argmax(own)), " ".join("%.2f" % v for v in own)))
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


def run_with_canaries(net, boards, a, t, w):
    """ops.qnet_loss_grad into outputs and a workspace with room to spare, none of which may be touched; q against forward_batch
    bit for bit and the LayerNorm-eps slots: (loss, td, None, per-tensor gradients) as float64 NumPy."""
    from g2048 import ops
    n, floats = len(boards), net.plain.numel()
    b, da, dt, dw = to_dev(boards, a, t, w)
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
    return float(loss[0]), td[:n].cpu().numpy().astype(np.float64), None, grads


def check_repeatable(net, codes, a, t, w):
    """Two calls give the same bits, and so does a call whose workspace and grad held NaN before it, twice."""
    from g2048 import ops
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


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_tile_edges_with_canaries(shape):
    model, boards, cases = random_case(*shape, "early")
    net = device_net(model)
    for n in RAGGED:
        a, t, w, want, f32 = cases[n]
        got = run_with_canaries(net, boards[:n], a, t, w)
        check(got, want, f32, True, "early boards, dim_ff %d L %d n=%d" % (net.dim_ff, net.n_layers, n))


@pytest.mark.parametrize("case", MATRIX_CASES, ids=MATRIX_IDS)
def test_shape_matrix_with_canaries(case):
    """The shape matrix of test_gpu_qnet_batch.py on early boards, every tensor checked: a main group followed by tail steps in
    the forward's products and in dX, GradWorkspace::x(l), layer(l) and the backward's loop at a third layer, and the sizes up to
    G2048_QNET_BATCH_MAX, where the call must also be repeatable and independent of what grad and the workspace held."""
    dim_ff, layers, n = case
    net = matrix_net(dim_ff, layers)
    boards, a, t, w, want, f32 = matrix_case(dim_ff, layers, n, "early")
    bound = check(run_with_canaries(net, boards, a, t, w), want, f32, True, "early boards, dim_ff %d L %d n=%d" % (dim_ff, layers, n))
    assert 0 < bound / R.F32_FACTOR <= FAIR_F32, "stock float32 autograd is no fair yardstick on this case: %.3g" % (bound / R.F32_FACTOR)
    if n == 4096:
        check_repeatable(net, boards, a, t, w)


@pytest.mark.parametrize("case", REGIME_CASES, ids=REGIME_IDS)
def test_peaked_attention_with_canaries(case):
    """Every tensor under a layer-0 softmax that is neither uniform nor one-hot: the attention backward's dS, and through it the
    embedding's and the three convolution backward kernels' results, on mid boards (codes 0..7) and, under the conditioned
    module, on full boards (codes up to 17, logits past float32 exp's overflow, several boards per thread in conv1's weight
    gradient at n = 1,025). The yardstick must be a fair one, as on the shape matrix."""
    regime, dim_ff, layers, n = case
    net = regime_net(regime, dim_ff, layers)
    boards, a, t, w, want, f32, _ = regime_case(*case)
    bound = check(run_with_canaries(net, boards, a, t, w), want, f32, True, "%s, dim_ff %d L %d n=%d" % case)
    assert 0 < bound / R.F32_FACTOR <= FAIR_F32, "stock float32 autograd is no fair yardstick on this case: %.3g" % (bound / R.F32_FACTOR)


@pytest.mark.parametrize("regime", REGIMES)
def test_peaked_attention_is_repeatable(regime):
    net = regime_net(regime, 64, 2)
    boards, a, t, w = regime_case(regime, 64, 2, 257)[:4]
    check_repeatable(net, boards, a, t, w)


@pytest.mark.parametrize("n", (1, 17))
def test_full_boards_at_a_third_layer(n):
    """test_full_boards' convention at dim_ff 160 with 3 layers: every tensor at n = 1, those downstream of layer 0's softmax at 17."""
    net = matrix_net(160, 3)
    boards, a, t, w, want, f32 = matrix_case(160, 3, n, "full")
    check(run(net, boards, a, t, w), want, f32, n == 1, "full boards, dim_ff 160 L 3 n=%d" % n)


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
    g, policy_boards, fixture = fixture_net()
    model, boards, cases = random_case(2, 64, 2, "early")
    small = device_net(model)
    a256, _, w256 = R.recipe(256)
    for net, codes, (a, t, w) in ((small, boards[:17], cases[17][:3]), (small, boards[:257], cases[257][:3]),
                                  (fixture, policy_boards[:256], (a256, g["full_256_targets"], w256))):
        check_repeatable(net, codes, a, t, w)


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
