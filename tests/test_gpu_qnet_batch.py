"""g2048_qnet_forward_batch and g2048_dqn_targets on the MI355X: the reference's HybridDQN called on a whole batch (one sequence of
n tokens that attend to each other) on the fixture's weights (tests/golden/qnet_batch.npz), random-init modules against their own
CPU f64 batch forward at every tile edge with canaries, n = 1 against the per-board kernel, determinism bit for bit and a poisoned
workspace, the proof that the other boards of a call are attended to, permutation, the Double-DQN targets against torch on the
launch's own Q bit for bit and against the reference's f64 actions and targets, and refresh(); a shape matrix (MATRIX) that runs the
products' main-plus-tail loop in every combination, a third layer and the sizes up to G2048_QNET_BATCH_MAX, with the targets at the
limit; and the peaked-attention cases (REGIME_CASES, shared with test_gpu_qnet_grad.py): layer 0's softmax spread over a few keys,
on mid boards, on full boards under the conditioned module, and at three layers whose tensors differ from layer to layer.

Tolerance, the f32 convention of test_gpu_qnet.py: |q - q_f64| <= 8 x max|q_f32 - q_f64| of the case, q_f32 the stock module's
float32 CPU batch call on the same boards and weights; the measured multiple is printed. On the shape matrix's early boards
(codes 0..3) the yardstick itself must lie in (0, 1e-5], so that a blown yardstick cannot hide a failure.

Measured on an MI355X over the shape matrix: early boards 0.47 - 2.49 x (yardstick 5.5e-8 .. 5.1e-7), full boards 0.39 - 1.08 x
(yardstick 1.5e-7 .. 5.3e-4); per shape in docs/LOG.md R19.1. Peaked-attention cases: 0.61 - 1.09 x (yardstick 1.9e-7 .. 5.6e-7;
R22.1)."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_qnet_batch_host import SIZES, target_model, torch_targets
from test_qnet_host import golden_model, random_model, tiles

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32_FACTOR = 8.0
LEFT_OUT_CAP = 0.01
RAGGED = (1, 15, 16, 17, 31, 33, 255, 257, 1025)            # every tile edge, and one size beyond any single LDS key tile
# The shape matrix: (dim_ff, layers, sizes). The products walk their contraction in groups of 128 (eight accumulators) and finish
# in steps of 32 into the first two: 96 = three tail steps alone, 160 = one group and one step (and a third layer), 224 = one group
# and three steps, 416 = three groups and one step with the last block of the dim_ff / 64 grid half empty; 32 carries the sizes
# around and at G2048_QNET_BATCH_MAX.
MATRIX = ((96, 1, (1, 17, 33, 257)), (160, 3, (1, 17, 33, 257)), (224, 2, (1, 17, 33, 257)), (416, 1, (17, 33)), (32, 1, (2049, 4095, 4096)))
MATRIX_CASES = [(ff, layers, n) for ff, layers, sizes in MATRIX for n in sizes]
MATRIX_IDS = ["ff%d-L%d-n%d" % c for c in MATRIX_CASES]
MODEL_SEED, BOARD_SEED = 2, 11
FAIR_F32 = 1e-5                                             # above this stock float32 is no yardstick (test_qnet_grad_host.py)
# The peaked-attention cases (regime, dim_ff, layers, n): layer 0's softmax neither uniform (early boards) nor one-hot (full boards).
# 1,025 is one beyond a single LDS key tile and four boards per thread in the conv1 weight gradient's reduction.
# 'distinct' is 'mid' at three layers with the second and third layers' tensors made their own: nn.TransformerEncoder deep-copies one
# layer, so in every other random-init module here the layers carry the same weights and a wrong layer offset l * pl_layer(ff)
# would read the right numbers.
REGIMES = ("mid", "conditioned")
REGIME_CASES = ([(r, ff, layers, n) for r in REGIMES for ff, layers, sizes in ((64, 2, (17, 257, 1025)), (160, 3, (17, 257))) for n in sizes]
                + [("distinct", 160, 3, n) for n in (17, 257)])
REGIME_IDS = ["%s-ff%d-L%d-n%d" % c for c in REGIME_CASES]


def check(q, want, f32_cpu, what):
    """|q - want| <= 8 x the stock CPU-f32 error of the case; returns the absolute bound."""
    q = np.asarray(q, np.float64)
    qmax = np.abs(want).max()
    err, yard = np.abs(q - want).max() / qmax, np.abs(f32_cpu - want).max() / qmax
    print("%s: Q max error %.3g of max|Q| %.4g = %.2f x the CPU-f32 error %.3g (bound %.0f x)" % (what, err, qmax, err / yard, yard, F32_FACTOR))
    assert np.all(np.isfinite(q)), what
    assert err <= F32_FACTOR * yard, what
    return F32_FACTOR * yard * qmax


def case_boards(n, seed):
    """random_boards with the fixture's first boards mixed in (codes up to 17), as test_gpu_qnet.case_boards does."""
    from test_policy_host import random_boards
    b = random_boards(n, seed)
    g = load_golden("policy.npz")["boards"]
    k = min(n // 4, len(g))
    b[8:8 + k] = g[:k]
    return b


@functools.lru_cache(maxsize=None)
def random_case(seed, dim_ff, layers):
    """A random-init module and, per ragged size, its boards with the CPU f64 and f32 batch forwards (shared, never modified)."""
    from g2048 import qnet
    model = random_model(seed, dim_ff, layers)
    boards = case_boards(max(RAGGED), 9 + seed)
    p64 = qnet.parse(model.double())
    truth = {n: qnet.forward_batch_reference(p64, torch.from_numpy(boards[:n])).numpy() for n in RAGGED}
    m32 = model.float()
    with torch.no_grad():
        f32 = {n: m32(tiles(boards[:n], torch.float32)).numpy().astype(np.float64) for n in RAGGED}
    return m32, boards, truth, f32


def device_net(model):
    import copy
    from g2048 import DeviceQNetwork
    return DeviceQNetwork(copy.deepcopy(model).float().to(DEV))


def matrix_boards(n, kind):
    """'early': random_boards % 4, codes 0..3 (tiles <= 8), on which every quantity is a fair float32 quantity and layer 0's
    attention is uniform; 'mid': random_boards % 8, codes 0..7 (tiles <= 128), on which layer 0's attention is peaked and float32
    still fair; 'full': case_boards. Below 16 boards the last n of 16 (the recipes need a few rows; one board is then a random one,
    not the empty one)."""
    from test_policy_host import random_boards
    m = max(n, 16)
    if kind in ("early", "mid"):
        return (random_boards(m, BOARD_SEED) % (4 if kind == "early" else 8)).astype(np.uint8)[m - n:]
    assert kind == "full", kind
    return case_boards(m, BOARD_SEED)[m - n:]


@functools.lru_cache(maxsize=None)
def matrix_net(dim_ff, layers):
    """The shape's random-init module on the device: one network for all its sizes, so its buffers are reused across them."""
    return device_net(random_model(MODEL_SEED, dim_ff, layers))


@functools.lru_cache(maxsize=None)
def matrix_forward(dim_ff, layers, n, kind):
    """(boards, the CPU f64 batch forward, the stock module's CPU f32 batch call) of a matrix case (shared, never modified)."""
    from g2048 import qnet
    model = random_model(MODEL_SEED, dim_ff, layers)
    boards = matrix_boards(n, kind)
    with torch.no_grad():
        f32 = model(tiles(boards, torch.float32)).numpy().astype(np.float64)
    return boards, qnet.forward_batch_reference(qnet.parse(model.double()), torch.from_numpy(boards)).numpy(), f32


def regime_model(regime, dim_ff, layers):
    """The module of a peaked-attention case. 'mid': the matrix's random-init module. 'conditioned': the same with cnn[0].weight
    times 2^-10 (exact in every format), taken before any float64 or float32 copy: full boards then leave layer 0's logits near
    100 instead of 1e9, a softmax that is sharp but a float32 quantity. 'distinct': 'mid' with the layers after the first
    perturbed each by its own draws (distinct_layers), layer 0 and with it the attention regime as in 'mid'."""
    from test_policy_host import distinct_layers
    model = random_model(MODEL_SEED, dim_ff, layers)
    if regime == "conditioned":
        with torch.no_grad():
            model.cnn[0].weight.mul_(2.0 ** -10)
    elif regime == "distinct":
        distinct_layers(model.transformer.layers[1:], 5)
    else:
        assert regime == "mid", regime
    return model


def regime_boards(regime, n):
    return matrix_boards(n, "full" if regime == "conditioned" else "mid")


@functools.lru_cache(maxsize=None)
def regime_net(regime, dim_ff, layers):
    return device_net(regime_model(regime, dim_ff, layers))


@functools.lru_cache(maxsize=None)
def regime_forward(regime, dim_ff, layers, n):
    """(boards, the CPU f64 batch forward, the stock module's CPU f32 batch call) of a peaked-attention case (shared, never
    modified)."""
    from g2048 import qnet
    model = regime_model(regime, dim_ff, layers)
    boards = regime_boards(regime, n)
    with torch.no_grad():
        f32 = model(tiles(boards, torch.float32)).numpy().astype(np.float64)
    return boards, qnet.forward_batch_reference(qnet.parse(model.double()), torch.from_numpy(boards)).numpy(), f32


def forward_with_canaries(net, boards):
    """ops.qnet_forward_batch into a q with 67 rows and a workspace with 4,096 bytes to spare, neither of which may be touched."""
    from g2048 import ops
    n = len(boards)
    b = torch.from_numpy(boards).to(DEV)
    nb = ops.qnet_batch_workspace_bytes(n, net.dim_ff)
    q = torch.full((n + 67, 4), 7.0, device=DEV)
    ws = torch.full((nb + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    ops.qnet_forward_batch(b, net.plain, net.dim_ff, net.n_layers, q=q[:n], workspace=ws[:nb])
    torch.cuda.synchronize()
    assert torch.all(q[n:] == 7.0), "rows past n were written (n = %d)" % n
    assert torch.all(ws[nb:] == 0xA5), "bytes past the workspace were written (n = %d)" % n
    return q[:n].cpu().numpy()


@functools.lru_cache(maxsize=None)
def fixture_nets():
    g = load_golden("qnet_batch.npz")
    _, boards, online = golden_model()
    return g, boards, device_net(online), device_net(target_model(g))


def test_reference_class_on_the_fixture_weights():
    g, boards, online, target = fixture_nets()
    assert online.dim_ff == 2048 and online.n_layers == 2
    for key, net in (("online", online), ("target", target)):
        for n in SIZES:
            q = net.forward_batch(torch.from_numpy(boards[:n]).to(DEV))
            assert q.shape == (n, 4) and q.dtype == torch.float32
            check(q.cpu().numpy(), g["%s_q_f64_%d" % (key, n)], g["%s_q_f32_%d" % (key, n)], "reference class, %s network, n=%d" % (key, n))


@pytest.mark.parametrize("shape", [(2, 64, 2), (12, 32, 1)], ids=["ff64-L2", "ff32-L1"])
def test_ragged_sizes_and_canaries(shape):
    model, boards, truth, f32 = random_case(*shape)
    net = device_net(model)
    assert (net.dim_ff, net.n_layers) == shape[1:]
    for n in RAGGED:
        check(forward_with_canaries(net, boards[:n]), truth[n], f32[n], "dim_ff %d L %d n=%d" % (net.dim_ff, net.n_layers, n))


@pytest.mark.parametrize("case", MATRIX_CASES, ids=MATRIX_IDS)
def test_shape_matrix_with_canaries(case):
    """Every combination of the products' main groups and tail steps, a third layer, and the sizes up to the stated maximum, on
    early boards (the tight check: stock float32 must itself be within 1e-5 there) and on full boards."""
    dim_ff, layers, n = case
    net = matrix_net(dim_ff, layers)
    assert (net.dim_ff, net.n_layers) == (dim_ff, layers)
    for kind in ("early", "full"):
        boards, truth, f32 = matrix_forward(dim_ff, layers, n, kind)
        yard = np.abs(f32 - truth).max() / np.abs(truth).max()
        assert kind == "full" or 0 < yard <= FAIR_F32, "stock float32 is no fair yardstick on this case: %.3g" % yard
        check(forward_with_canaries(net, boards), truth, f32, "%s boards, dim_ff %d L %d n=%d" % (kind, dim_ff, layers, n))


@pytest.mark.parametrize("case", REGIME_CASES, ids=REGIME_IDS)
def test_peaked_attention_with_canaries(case):
    """Layer 0's softmax peaked on a few keys: mid boards, and full boards (codes up to 17, logits past float32 exp's overflow)
    under the conditioned module."""
    regime, dim_ff, layers, n = case
    net = regime_net(regime, dim_ff, layers)
    assert (net.dim_ff, net.n_layers) == (dim_ff, layers)
    boards, truth, f32 = regime_forward(*case)
    check(forward_with_canaries(net, boards), truth, f32, "%s, dim_ff %d L %d n=%d" % case)


def test_one_board_is_the_per_board_function():
    model, boards, truth, f32 = random_case(2, 64, 2)
    net = device_net(model)
    b = torch.from_numpy(boards[:1]).to(DEV)
    bound = check(net.forward_batch(b).cpu().numpy(), truth[1], f32[1], "n=1")
    assert np.abs(net.forward_batch(b).cpu().numpy().astype(np.float64) - net(b).cpu().numpy()).max() <= bound


def test_repeatable_and_independent_of_the_workspace_contents():
    from g2048 import ops
    g, boards, online, _ = fixture_nets()
    for n in (17, 300):
        b = torch.from_numpy(boards[:n]).to(DEV)
        first = online.forward_batch(b).clone()
        assert torch.equal(online.forward_batch(b), first), "two calls differ (n = %d)" % n
        nb = ops.qnet_batch_workspace_bytes(n, 2048)
        ws = torch.full((nb // 4,), float("nan"), device=DEV).view(torch.uint8)
        again = ops.qnet_forward_batch(b, online.plain, 2048, 2, workspace=ws)
        assert torch.equal(again, first), "a NaN-poisoned workspace changes the result (n = %d)" % n
        ws.view(torch.float32).fill_(float("nan"))
        assert torch.equal(ops.qnet_forward_batch(b, online.plain, 2048, 2, workspace=ws), first)


def test_the_other_boards_of_a_call_are_attended_to():
    g, boards, online, _ = fixture_nets()
    alone = online.forward_batch(torch.from_numpy(boards[:17]).to(DEV)).cpu().numpy().astype(np.float64)
    among = online.forward_batch(torch.from_numpy(boards[:300]).to(DEV)).cpu().numpy().astype(np.float64)[:17]
    bound = F32_FACTOR * max(np.abs(g["online_q_f32_%d" % n] - g["online_q_f64_%d" % n]).max() for n in (17, 300))
    diff = np.abs(alone - among).max()
    want = np.abs(g["online_q_f64_17"] - g["online_q_f64_300"][:17]).max()
    print("the same 17 boards alone and among 300: differ by %.3g (f64: %.3g; bound %.3g)" % (diff, want, bound))
    assert diff > bound and abs(diff - want) <= 2 * bound


def test_permuting_the_boards_permutes_q():
    g, boards, online, _ = fixture_nets()
    n = 300
    perm = np.random.default_rng(3).permutation(n)
    q = online.forward_batch(torch.from_numpy(boards[:n]).to(DEV)).cpu().numpy().astype(np.float64)
    qp = online.forward_batch(torch.from_numpy(boards[:n][perm].copy()).to(DEV)).cpu().numpy().astype(np.float64)
    bound = F32_FACTOR * np.abs(g["online_q_f32_300"] - g["online_q_f64_300"]).max()
    print("permuted call vs permuted rows: %.3g (bound %.3g)" % (np.abs(qp - q[perm]).max(), bound))
    assert np.abs(qp - q[perm]).max() <= bound


def test_dqn_targets_on_the_launchs_own_q():
    import g2048
    from g2048 import ops
    g, boards, online, target = fixture_nets()
    n = 300
    b = torch.from_numpy(boards[:n]).to(DEV)
    shaped, dones = torch.from_numpy(g["shaped"][:n]).to(DEV), torch.from_numpy(g["dones"][:n]).to(DEV)
    targets, actions = g2048.dqn_targets(online, target, b, shaped, dones, gamma=0.99)
    assert targets.dtype == torch.float32 and targets.shape == (n,) and actions.dtype == torch.int64 and actions.shape == (n,)
    q_online, q_target = online.forward_batch(b), target.forward_batch(b)       # bit-repeatable: the Q the launch read
    want, want_actions = torch_targets(q_online, q_target, shaped, dones, 0.99)
    assert torch.equal(actions, want_actions), "next_actions is not argmax(1) of the launch's own online Q"
    assert torch.equal(targets, want), "targets differ from the torch expression on the launch's own Q"
    assert torch.equal(targets[dones == 1], shaped[dones == 1])
    # hand-made Q with exact ties: the first maximum, unmasked
    qo = torch.tensor([[1, 1, 1, 1], [0, 2, 2, 1], [-1, -3, -1, -2], [0, 0, 0, 5], [3, 1, 3, 3], [-0.0, 0.0, -1, -1]], dtype=torch.float32, device=DEV)
    qt = torch.arange(24, dtype=torch.float32, device=DEV).reshape(6, 4) / 7
    sh, dn = torch.linspace(-2, 3, 6, device=DEV), torch.tensor([0, 1, 0, 0, 1, 0], dtype=torch.float32, device=DEV)
    t, a = ops.dqn_targets(qo, qt, sh, dn, 0.99)
    assert a.tolist() == [0, 1, 0, 3, 0, 0] and torch.equal(a, qo.argmax(1))
    assert torch.equal(t, torch_targets(qo, qt, sh, dn, 0.99)[0])
    # canaries: nothing past n
    tt, aa = torch.full((n + 9,), 7.0, device=DEV), torch.full((n + 9,), 9, dtype=torch.int64, device=DEV)
    ops.dqn_targets(q_online, q_target, shaped, dones, 0.99, targets=tt[:n], next_actions=aa[:n])
    assert torch.all(tt[n:] == 7.0) and torch.all(aa[n:] == 9) and torch.equal(tt[:n], targets)


def test_dqn_targets_at_the_batch_limit():
    import g2048
    from g2048 import ops
    n = 4096
    online, target = matrix_net(32, 1), device_net(random_model(MODEL_SEED + 1, 32, 1))
    rng = np.random.default_rng(5)
    b = torch.from_numpy(matrix_boards(n, "early")).to(DEV)
    shaped = torch.from_numpy(rng.normal(4.0, 3.0, n).astype(np.float32)).to(DEV)
    dones = torch.from_numpy((rng.random(n) < 0.1).astype(np.float32)).to(DEV)
    targets, actions = g2048.dqn_targets(online, target, b, shaped, dones, gamma=0.99)
    assert targets.shape == (n,) and actions.shape == (n,)
    q_online, q_target = online.forward_batch(b), target.forward_batch(b)       # bit-repeatable: the Q the launch read
    want, want_actions = torch_targets(q_online, q_target, shaped, dones, 0.99)
    assert torch.equal(actions, want_actions) and torch.equal(targets, want), "n = 4096: not the torch expression on the launch's own Q"
    assert torch.equal(targets[dones == 1], shaped[dones == 1]) and 0 < int(dones.sum()) < n
    assert len(torch.unique(actions)) > 1 and not torch.equal(q_online, q_target)
    tt, aa = torch.full((n + 9,), 7.0, device=DEV), torch.full((n + 9,), 9, dtype=torch.int64, device=DEV)
    ops.dqn_targets(q_online, q_target, shaped, dones, 0.99, targets=tt[:n], next_actions=aa[:n])
    assert torch.all(tt[n:] == 7.0) and torch.all(aa[n:] == 9) and torch.equal(tt[:n], want) and torch.equal(aa[:n], want_actions)


def test_dqn_targets_against_the_reference():
    import g2048
    g, boards, online, target = fixture_nets()
    for n in (17, 256, 300):
        b = torch.from_numpy(boards[:n]).to(DEV)
        shaped, dones = torch.from_numpy(g["shaped"][:n]).to(DEV), torch.from_numpy(g["dones"][:n]).to(DEV)
        targets, actions = (t.cpu().numpy() for t in g2048.dqn_targets(online, target, b, shaped, dones, gamma=float(g["gamma"])))
        q = g["online_q_f64_%d" % n]
        bound = F32_FACTOR * np.abs(g["online_q_f32_%d" % n] - q).max()
        srt = np.sort(q, axis=1)
        clear = (srt[:, 3] - srt[:, 2]) > 2 * bound
        wrong = actions != g["actions_f64_%d" % n]
        t_bound = F32_FACTOR * np.abs(g["target_q_f32_%d" % n] - g["target_q_f64_%d" % n]).max()
        want = g["targets_f64_%d" % n]
        err = np.abs(targets.astype(np.float64) - want)
        allowed = float(g["gamma"]) * t_bound + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        print("n=%d: %.2f %% of the boards within twice the Q bound of a tie; differing actions %d among the clear; target error %.3g "
              "(allowed %.3g)" % (n, 100 * (1 - clear.mean()), (wrong & clear).sum(), err[clear].max(), allowed[clear].min()))
        assert 1 - clear.mean() <= LEFT_OUT_CAP
        assert not np.any(wrong & clear)
        assert np.all(err[clear] <= allowed[clear])
        assert np.array_equal(targets[g["dones"][:n] == 1], g["shaped"][:n][g["dones"][:n] == 1])


def test_refresh_after_an_in_place_weight_change():
    import copy
    from g2048 import qnet
    model, boards, _, _ = random_case(2, 64, 2)
    net = device_net(model)
    m = net.model
    b = torch.from_numpy(boards[:33]).to(DEV)
    before = net.forward_batch(b).clone()
    with torch.no_grad():
        m.fc.bias.add_(0.5)
        m.transformer.layers[0].self_attn.in_proj_weight[:256].mul_(0.5)         # Q and K rows: the per-board kernel never reads them
    assert torch.equal(net.forward_batch(b), before), "the weights changed without refresh()"
    net.refresh()
    after = net.forward_batch(b).cpu().numpy()
    cpu = copy.deepcopy(m).cpu()
    with torch.no_grad():
        f32 = cpu(tiles(boards[:33], torch.float32)).numpy().astype(np.float64)
    want = qnet.forward_batch_reference(qnet.parse(cpu.double()), torch.from_numpy(boards[:33])).numpy()
    check(after, want, f32, "after refresh()")
    old = before.cpu().numpy().astype(np.float64)
    assert np.abs(after - old).max() > 0.1
    assert np.abs(after - 0.5 - old).max() > 1e-3, "only fc.bias arrived: the Q / K rows of in_proj were not refreshed"


def test_refusals_on_the_device():
    from g2048 import DeviceQNetwork
    model, boards, _, _ = random_case(2, 64, 2)
    import copy
    net16 = DeviceQNetwork(copy.deepcopy(model).float().to(DEV), precision="bf16")
    b = torch.from_numpy(boards[:16]).to(DEV)
    with pytest.raises(ValueError, match="bf16"):
        net16.forward_batch(b)
    assert net16(b).shape == (16, 4)                         # the per-board path keeps accepting bf16
    net = device_net(model)
    with pytest.raises(ValueError, match="4096"):
        net.forward_batch(torch.zeros((4097, 16), dtype=torch.uint8, device=DEV))
    with pytest.raises(TypeError):
        net.forward_batch(b.to(torch.int32))
