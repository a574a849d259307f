"""g2048_qnet_forward on the MI355X: the reference's HybridDQN on the fixture's weights (tests/golden/qnet.npz), a random-init
module against its own CPU f64 per-board forward at ragged sizes with canaries, the smallest legal shape, two shapes that are no
power of two (dim_ff 96 with one layer, 160 with three: the packed blob's odd slice counts and third-layer offsets), position independence
and determinism bit for bit, the exploit action against the launch's own Q-values and against the reference's f64 actions,
in-place refresh and argument validation.

Tolerances, all relative to max |Q| of the case and printed as measured multiples.
f32: 8 x the error stock CPU-float32 torch makes against f64 on the same boards and weights (q_f32 in the fixture; the module in
float32 with the (1, B, 128) encoder input for the random-weight cases). The margin is for the device's 1,024- and 2,048-term
sums running in another order; a misplaced fragment costs 1e-2 and more.
bf16: BF16_FACTOR = 4 x the error that rounding the weights alone to bf16 costs (the same network in f64 with bf16 weights
against f64: q_bf16w in the fixture, computed here for the random-weight cases), the convention and the reason of
test_gpu_tpolicy.py: every matmul rounds one weight and one activation operand, errors of about equal size.
Actions against the reference: every board whose top-two valid-move gap in q_f64 exceeds twice the Q bound must match; the boards
left out are capped at 1 % (f32) and 20 % (bf16)."""
import functools

import numpy as np
import pytest
import torch

import qnet_weights as qw
from conftest import load_golden
from test_policy_host import distinct_layers, random_boards
from test_qnet_host import bf16_round, golden_model, random_model, tiles

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32_FACTOR, BF16_FACTOR = 8.0, 4.0
LEFT_OUT_CAP = {"f32": 0.01, "bf16": 0.20}
BLOCK = 128                                                  # boards per block of the forward kernel (four wavefronts of 32)


def q_bound(precision, want, f32_cpu, weights_only):
    """The absolute bound on |q - want| of the case."""
    return (F32_FACTOR * np.abs(f32_cpu - want).max()) if precision == "f32" else (BF16_FACTOR * np.abs(weights_only - want).max())


def check(precision, q, want, f32_cpu, weights_only, what):
    """f32_cpu: stock CPU float32 torch; weights_only: the f64 network with bf16 weights; the yardsticks of the two bounds."""
    q = np.asarray(q, np.float64)
    qmax = np.abs(want).max()
    err = np.abs(q - want).max() / qmax
    yard = (np.abs(f32_cpu - want).max() if precision == "f32" else np.abs(weights_only - want).max()) / qmax
    factor = F32_FACTOR if precision == "f32" else BF16_FACTOR
    print("%s %s: Q max error %.3g of max|Q| %.4g = %.2f x the %s error %.3g (bound %.0f x)" % (
        what, precision, err, qmax, err / yard, "CPU-f32" if precision == "f32" else "weights-only", yard, factor))
    assert np.all(np.isfinite(q)), what
    assert err <= factor * yard, what


def module_rows_f32(model, boards):
    """Stock torch in float32 on the CPU computing the per-board function: the module with the (1, B, 128) encoder input."""
    m = model.float()
    x = tiles(boards, torch.float32)
    with torch.no_grad():
        h = m.embedding(m.cnn(x.view(-1, 1, 4, 4)).view(len(x), -1))
        return m.fc(m.transformer(h.unsqueeze(0)).squeeze(0)).numpy().astype(np.float64)


def cpu_forwards(model, boards):
    """(f64 truth, stock CPU f32, f64 with bf16 weights) of a RefSpelling module on uint8 boards, as NumPy arrays."""
    from g2048 import qnet
    p = qnet.parse(model)
    b = torch.from_numpy(boards)
    truth = qnet.forward_reference(p, b).numpy()
    rounded = qnet.forward_reference(p, b, round_weights=bf16_round).numpy()
    return truth, module_rows_f32(model, boards), rounded


def case_boards(n, seed):
    """Random boards (codes 0..11, empty boards, one of 17s) with the fixture's first boards mixed in (codes up to 17)."""
    b = random_boards(n, seed)
    g = load_golden("policy.npz")["boards"]
    k = min(n // 4, len(g))
    b[8:8 + k] = g[:k]
    return b


@functools.lru_cache(maxsize=None)
def ragged_case():
    """The random-init module (dim_ff 64, 2 layers), 4,097 boards and their CPU forwards (shared by the ragged-size, the
    position and the refresh tests; never modified)."""
    model = random_model(2, 64, 2)
    boards = case_boards(4097, 9)
    truth, f32_cpu, rounded = cpu_forwards(model, boards)
    return model.float(), boards, truth, f32_cpu, rounded


def device_copy(model):
    import copy
    return copy.deepcopy(model).float().to(DEV)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_reference_class_on_the_fixture_weights(precision):
    from g2048 import DeviceQNetwork
    g, boards, model = golden_model()
    net = DeviceQNetwork(model.float().to(DEV), precision=precision)
    assert net.dim_ff == 2048 and net.n_layers == 2
    q = net(torch.from_numpy(boards).to(DEV))
    assert q.shape == (2048, 4) and q.dtype == torch.float32
    check(precision, q.cpu().numpy(), g["q_f64"], g["q_f32"], g["q_bf16w"], "reference class, dim_ff 2048")


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_ragged_sizes_and_canaries(precision):
    from g2048 import DeviceQNetwork, ops
    model, all_boards, truth, f32_cpu, rounded = ragged_case()
    net = DeviceQNetwork(device_copy(model), precision=precision)
    assert net.dim_ff == 64 and net.n_layers == 2
    for n in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1, 4097):
        b = torch.from_numpy(all_boards[:n]).to(DEV)
        q = torch.full((n + 67, 4), 7.0, device=DEV)
        actions = torch.full((n + 67,), 9, dtype=torch.uint8, device=DEV)
        ops.qnet_forward(b, net.packed, 64, 2, precision, q=q[:n], actions=actions[:n])
        torch.cuda.synchronize()
        assert torch.all(q[n:] == 7.0) and torch.all(actions[n:] == 9), "rows past n were written (n = %d)" % n
        assert torch.all(actions[:n] < 4)
        check(precision, q[:n].cpu().numpy(), truth[:n], f32_cpu[:n], rounded[:n], "dim_ff 64 n=%d" % n)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_one_layer_dim_ff_32(precision):
    from g2048 import DeviceQNetwork
    model = random_model(12, 32, 1)
    boards = case_boards(1000, 5)
    truth, f32_cpu, rounded = cpu_forwards(model, boards)
    net = DeviceQNetwork(model.float().to(DEV), precision=precision)
    assert net.dim_ff == 32 and net.n_layers == 1
    check(precision, net(torch.from_numpy(boards).to(DEV)).cpu().numpy(), truth, f32_cpu, rounded, "L=1 dim_ff=32")


# The packed path away from powers of two: 96 = three 32-feature slices of the feed-forward pair (an odd count; linear2 with three
# bf16 chunks, fragment index o * c2 + c with c2 = 6 or 3), 160 = five slices with a second and a third layer's offsets into the
# fragments and the f32 section.
PACKED_SHAPES = [(96, 1), (160, 3)]


@functools.lru_cache(maxsize=None)
def packed_shape_case(dim_ff, layers):
    """A random-init module of the shape with every layer's tensors its own (distinct_layers: a fresh module's layers are copies
    of one), 257 boards and their CPU forwards (shared, never modified)."""
    model = random_model(2, dim_ff, layers)
    distinct_layers(model.transformer.layers, 5)
    boards = case_boards(257, 11)
    truth, f32_cpu, rounded = cpu_forwards(model, boards)
    return model.float(), boards, truth, f32_cpu, rounded


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("shape", PACKED_SHAPES, ids=["ff%d-L%d" % s for s in PACKED_SHAPES])
def test_packed_shape_matrix_with_canaries(shape, precision):
    from g2048 import DeviceQNetwork, ops
    dim_ff, layers = shape
    model, all_boards, truth, f32_cpu, rounded = packed_shape_case(dim_ff, layers)
    net = DeviceQNetwork(device_copy(model), precision=precision)
    assert (net.dim_ff, net.n_layers) == shape
    for n in (17, 257):
        b = torch.from_numpy(all_boards[:n]).to(DEV)
        q = torch.full((n + 67, 4), 7.0, device=DEV)
        actions = torch.full((n + 67,), 9, dtype=torch.uint8, device=DEV)
        ops.qnet_forward(b, net.packed, dim_ff, layers, precision, q=q[:n], actions=actions[:n])
        torch.cuda.synchronize()
        assert torch.all(q[n:] == 7.0) and torch.all(actions[n:] == 9), "rows past n were written (n = %d)" % n
        assert torch.all(actions[:n] < 4)
        check(precision, q[:n].cpu().numpy(), truth[:n], f32_cpu[:n], rounded[:n], "dim_ff %d L %d n=%d" % (dim_ff, layers, n))
    if layers == 3:
        for i in (0, 130, 256):                              # alone: another wavefront, block and column than in the large call
            a, q1 = net.act(b[i:i + 1].clone())
            assert torch.equal(q1[0], q[i]) and a[0] == actions[i], "board %d alone differs from row %d of the large call" % (i, i)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_outputs_do_not_depend_on_position_or_batch_size(precision):
    from g2048 import DeviceQNetwork
    model, all_boards, _, _, _ = ragged_case()
    net = DeviceQNetwork(device_copy(model), precision=precision)
    b = torch.from_numpy(all_boards).to(DEV)
    a1, q1 = [t.clone() for t in net.act(b)]
    a2, q2 = net.act(b)
    assert torch.equal(q1, q2) and torch.equal(a1, a2), "two launches differ"
    assert torch.equal(net(b), q1), "Q without actions differs"
    for i in (0, 5, 16, 31, 32, BLOCK - 1, BLOCK, 2000, 4095, 4096):          # alone
        a, q = net.act(b[i:i + 1].clone())
        assert torch.equal(q[0], q1[i]) and a[0] == a1[i], "board %d alone differs from row %d of the large call" % (i, i)
    for start in (3, 1000, 4097 - 17):                       # 17 boards at other offsets within their wavefronts and blocks
        a, q = net.act(b[start:start + 17].clone())
        assert torch.equal(q, q1[start:start + 17]) and torch.equal(a, a1[start:start + 17]), "n = 17 from %d differs" % start


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_actions_are_the_masked_argmax_of_the_launchs_own_q(precision):
    from g2048 import DeviceQNetwork, ops
    model, all_boards, _, _, _ = ragged_case()
    boards = all_boards[:2048].copy()
    boards[100] = np.array([1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1], np.uint8)        # full, no merge: no valid move
    boards[101] = np.array([1, 2, 1, 0, 2, 1, 2, 0, 1, 2, 1, 0, 2, 1, 2, 0], np.uint8)        # only RIGHT moves anything
    boards[102] = np.array([3, 4, 3, 4, 4, 3, 4, 3, 3, 4, 3, 4, 0, 0, 0, 0], np.uint8)        # only DOWN
    b = torch.from_numpy(boards).to(DEV)
    mask = ops.valid_moves(b).cpu().numpy()
    valid = qw.mask_bits(mask)
    assert (valid.sum(1) == 0).sum() >= 2 and (valid.sum(1) == 1).sum() >= 2 and (valid.sum(1) == 4).sum() >= 100
    assert mask[100] == 0 and mask[101] == 4 and mask[102] == 8
    net = DeviceQNetwork(device_copy(model), precision=precision)
    actions, q = net.act(b)
    actions, q = actions.cpu().numpy(), q.cpu().numpy()
    assert actions.dtype == np.uint8 and np.array_equal(actions, qw.masked_argmax(q, valid))
    assert np.all(actions[valid.sum(1) == 0] == 0) and actions[101] == 2 and actions[102] == 3


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_actions_against_the_reference(precision):
    from g2048 import DeviceQNetwork, ops
    g, boards, model = golden_model()
    b = torch.from_numpy(boards).to(DEV)
    valid = qw.mask_bits(ops.valid_moves(b).cpu().numpy())
    assert np.array_equal(g["actions_f64"], qw.masked_argmax(g["q_f64"], valid))     # the device's mask is the oracle's
    actions, _ = DeviceQNetwork(model.float().to(DEV), precision=precision).act(b)
    bound = q_bound(precision, g["q_f64"], g["q_f32"], g["q_bf16w"])
    clear = qw.top_two_gap(g["q_f64"], valid) > 2 * bound
    left_out = 1.0 - clear.mean()
    wrong = actions.cpu().numpy() != g["actions_f64"]
    print("actions %s: %.2f %% of the boards within twice the Q bound %.3g of a tie (cap %.0f %%); differing actions: %d among the clear, "
          "%d among the rest" % (precision, 100 * left_out, bound, 100 * LEFT_OUT_CAP[precision], (wrong & clear).sum(), (wrong & ~clear).sum()))
    assert left_out <= LEFT_OUT_CAP[precision]
    assert not np.any(wrong & clear)


def test_refresh_after_an_in_place_weight_change():
    from g2048 import DeviceQNetwork
    model, all_boards, _, _, _ = ragged_case()
    m = device_copy(model)
    net = DeviceQNetwork(m)
    b = torch.from_numpy(all_boards[:300]).to(DEV)
    before = net(b).clone()
    packed_at = net.packed.data_ptr()
    with torch.no_grad():
        m.fc.bias.add_(0.5)
        m.transformer.layers[1].linear2.weight.mul_(1.25)
    assert torch.equal(net(b), before), "the packed weights changed without refresh()"
    m.train()
    with pytest.raises(ValueError, match="training mode"):
        net.refresh()
    m.eval()
    net.refresh()
    after = net(b).clone()
    assert net.packed.data_ptr() == packed_at, "refresh() did not pack in place"
    assert not torch.equal(after, before) and (after - before).abs().max() > 0.1
    assert torch.equal(after, DeviceQNetwork(m)(b)), "refresh() differs from a fresh conversion"


def test_bad_arguments_launch_nothing():
    from g2048 import DeviceQNetwork, _lib, ops
    L = _lib.lib()
    model, all_boards, _, _, _ = ragged_case()
    net = DeviceQNetwork(device_copy(model))
    b = torch.from_numpy(all_boards[:64]).to(DEV)
    q = torch.full((64, 4), 3.0, device=DEV)
    actions = torch.full((64,), 9, dtype=torch.uint8, device=DEV)
    w = net.packed
    cases = [
        ((b.data_ptr() + 4, w.data_ptr(), q.data_ptr(), actions.data_ptr(), 60, 64, 2, 0, None), b"misaligned"),
        ((b.data_ptr(), w.data_ptr() + 8, q.data_ptr(), None, 64, 64, 2, 0, None), b"misaligned"),
        ((b.data_ptr(), w.data_ptr(), q.data_ptr() + 4, None, 60, 64, 2, 0, None), b"misaligned"),
        ((b.data_ptr(), w.data_ptr(), q.data_ptr(), actions.data_ptr(), 64, 64, 2, 5, None), b"opts"),
        ((b.data_ptr(), w.data_ptr(), q.data_ptr(), actions.data_ptr(), 64, 48, 2, 0, None), b"dim_ff"),
        ((b.data_ptr(), w.data_ptr(), q.data_ptr(), actions.data_ptr(), 64, 64, 0, 0, None), b"n_layers"),
        ((b.data_ptr(), None, q.data_ptr(), None, 64, 64, 2, 0, None), b"null pointer"),
        ((b.data_ptr(), w.data_ptr(), None, actions.data_ptr(), 64, 64, 2, 0, None), b"null pointer"),
    ]
    for args, msg in cases:
        assert L.g2048_qnet_forward(*args) == -1
        assert msg in L.g2048_last_error()
    packed = torch.full((ops.qnet_packed_bytes("f32", 64, 2),), 9, dtype=torch.uint8, device=DEV)
    plain = torch.zeros(ops.qnet_plain_floats(64, 2), device=DEV)
    assert L.g2048_qnet_pack(plain.data_ptr(), 64, 2, 3, packed.data_ptr(), None) == -1 and b"precision" in L.g2048_last_error()
    assert L.g2048_qnet_pack(plain.data_ptr(), 48, 2, 0, packed.data_ptr(), None) == -1 and b"dim_ff" in L.g2048_last_error()
    assert L.g2048_qnet_pack(plain.data_ptr(), 64, 0, 0, packed.data_ptr(), None) == -1 and b"n_layers" in L.g2048_last_error()
    assert L.g2048_qnet_pack(plain.data_ptr(), 64, 2, 0, packed.data_ptr() + 8, None) == -1 and b"misaligned" in L.g2048_last_error()
    assert L.g2048_qnet_pack(None, 64, 2, 0, packed.data_ptr(), None) == -1 and b"null pointer" in L.g2048_last_error()
    torch.cuda.synchronize()
    assert torch.all(q == 3.0) and torch.all(actions == 9) and torch.all(packed == 9), "a refused call wrote output"
    with pytest.raises(TypeError):
        net(b.to(torch.int32))
    with pytest.raises(ValueError):
        ops.qnet_forward(b, w, 64, 2, "f32", q=q[:10])
    with pytest.raises(ValueError):
        ops.qnet_forward(b, w, 2048, 2, "f32")                 # the blob was packed for another shape
    with pytest.raises(ValueError):
        ops.qnet_pack(plain[:-1], 64, 2)
    only_q = ops.qnet_forward(b, w, 64, 2, "f32")              # actions are optional in the C-ABI
    assert torch.equal(only_q, net(b))
