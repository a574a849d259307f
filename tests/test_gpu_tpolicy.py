"""g2048_tpolicy_forward on the MI355X: the reference's transformer class on the fixture's weights (tests/golden/tpolicy.npz),
the bench shape with random weights against the module's own CPU f64 forward at ragged sizes, two shapes that are no power of two
(dim_ff 96 with one layer, 160 with three: the packed blob's odd slice counts and third-layer offsets), position independence and
determinism bit for bit, the RolloutCollector boards hook, in-place refresh under a captured rollout graph, and argument
validation.

Tolerances. f32: test_gpu_policy.TOL["f32"] as it stands. bf16: 4 x the error that rounding the weights alone to bf16 costs
(the same network in f64 with bf16 weights against f64: recorded in the fixture, computed here for the random-weight shapes),
max and mean of the probabilities separately, values relative to max |v|: every matmul rounds one weight and one activation
operand, errors of about equal size, and a misplaced fragment costs 0.1 and more."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_policy import TOL, _collector_state, _start_from, _traj
from test_gpu_rollout import TinyTransformerPolicy, replay_and_check
from test_policy_host import distinct_layers, random_boards
from test_tpolicy_host import bf16_round, golden_model, scale_heads

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16_FACTOR = 4.0


def errors(probs, values, want_p, want_v):
    ep = np.abs(np.asarray(probs, np.float64) - want_p)
    ev = np.abs(np.asarray(values, np.float64) - want_v).max() / np.abs(want_v).max()
    return ep.max(), ep.mean(), ev


def check(precision, probs, values, want_p, want_v, weights_only, what):
    """weights_only: (probs, values) of the f64 network with bf16 weights, the yardstick of the bf16 bound."""
    pmax, pmean, ev = errors(probs, values, want_p, want_v)
    probs = np.asarray(probs, np.float64)
    if precision == "f32":
        bound = (TOL["f32"]["probs"], TOL["f32"]["probs_mean"], TOL["f32"]["values"])
        print("%s f32: probs max %.3g mean %.3g; values max %.3g of max|v| %.4g" % (what, pmax, pmean, ev, np.abs(want_v).max()))
    else:
        w = errors(weights_only[0], weights_only[1], want_p, want_v)
        bound = tuple(BF16_FACTOR * e for e in w)
        print("%s bf16: probs max %.3g (%.2f x weights-only %.3g) mean %.3g (%.2f x %.3g); values max %.3g of max|v| (%.2f x %.3g)" % (
            what, pmax, pmax / w[0], w[0], pmean, pmean / w[1], w[1], ev, ev / w[2], w[2]))
    assert np.all(np.isfinite(probs)) and np.allclose(probs.sum(1), 1.0, atol=1e-5 if precision == "f32" else 1e-4)
    assert pmax <= bound[0] and pmean <= bound[1] and ev <= bound[2], what


def tiny_model(seed, dim_ff=128, num_layers=2):
    """TinyTransformerPolicy (tests/test_gpu_rollout.py) with torch's default init, the heads scaled up, eval mode, on the CPU."""
    torch.manual_seed(seed)
    m = TinyTransformerPolicy(num_layers=num_layers)
    if dim_ff != 128:
        import torch.nn as nn
        layer = nn.TransformerEncoderLayer(d_model=64, nhead=4, dim_feedforward=dim_ff, batch_first=True)
        m.encoder = nn.TransformerEncoder(layer, num_layers=num_layers)
    return scale_heads(m.eval())


def cpu_forwards(model, boards):
    """(f64 truth, f64 with bf16 weights) of the module on uint8 boards, on the CPU, as NumPy pairs."""
    from g2048 import tpolicy
    p = tpolicy.parse(model)
    b = torch.from_numpy(boards)
    out = []
    for rw in (None, bf16_round):
        pr, va = [], []
        for i in range(0, len(boards), 8192):
            a, c = tpolicy.forward_reference(p, b[i:i + 8192], round_weights=rw)
            pr.append(a)
            va.append(c)
        out.append((torch.cat(pr).numpy(), torch.cat(va).numpy()))
    return out


@functools.lru_cache(maxsize=None)
def bench_shape_case():
    """The bench-shape model, 65,537 boards and their CPU forwards (shared by the ragged-size and the position tests)."""
    model = tiny_model(2)
    boards = random_boards(65537, 9)
    with torch.no_grad():                                    # the module's own forward is the function forward_reference computes
        want = model.double()(torch.from_numpy(boards[:512]).double() / 15)
    truth, rounded = cpu_forwards(model, boards)
    assert np.abs(truth[0][:512] - want[0].numpy()).max() <= 1e-12 and np.abs(truth[1][:512] - want[1].numpy()).max() <= 1e-12
    return model.float(), boards, truth, rounded


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_reference_class_on_the_fixture_weights(precision):
    from g2048 import DeviceTransformerPolicy
    g, model = golden_model()
    pol = DeviceTransformerPolicy(model.float().to(DEV), precision=precision)
    assert pol.dim_ff == 2048 and pol.n_layers == 2
    p, v = pol(torch.from_numpy(g["boards"]).to(DEV))
    check(precision, p.cpu().numpy(), v.cpu().numpy(), g["probs_f64"], g["value_f64"], (g["probs_bf16w"], g["value_bf16w"]),
          "reference class, dim_ff 2048")


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_bench_shape_ragged_sizes_and_canaries(precision):
    from g2048 import DeviceTransformerPolicy, ops
    model, all_boards, truth, rounded = bench_shape_case()
    pol = DeviceTransformerPolicy(model.to(DEV), precision=precision)
    assert pol.dim_ff == 128 and pol.n_layers == 2
    for n in (1, 2, 15, 16, 17, 63, 64, 65, 4096, 65537):
        b = torch.from_numpy(all_boards[:n]).to(DEV)
        probs = torch.full((n + 67, 4), 7.0, device=DEV)
        value = torch.full((n + 67, 1), 7.0, device=DEV)
        ops.tpolicy_forward(b, pol.packed, 128, 2, precision, probs=probs[:n], value=value[:n])
        torch.cuda.synchronize()
        assert torch.all(probs[n:] == 7.0) and torch.all(value[n:] == 7.0), "rows past n were written (n = %d)" % n
        check(precision, probs[:n].cpu().numpy(), value[:n].cpu().numpy(), truth[0][:n], truth[1][:n],
              (rounded[0][:n], rounded[1][:n]), "bench shape n=%d" % n)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_one_layer_dim_ff_32(precision):
    from g2048 import DeviceTransformerPolicy
    model = tiny_model(12, dim_ff=32, num_layers=1)
    boards = random_boards(1000, 5)
    truth, rounded = cpu_forwards(model, boards)
    pol = DeviceTransformerPolicy(model.to(DEV), precision=precision)
    assert pol.dim_ff == 32 and pol.n_layers == 1
    p, v = pol(torch.from_numpy(boards).to(DEV))
    check(precision, p.cpu().numpy(), v.cpu().numpy(), truth[0], truth[1], rounded, "L=1 dim_ff=32")


# The packed path away from powers of two: 96 = three 32-feature slices of the feed-forward pair (an odd count; linear2 with three
# bf16 chunks, fragment index o * c2 + c with c2 = 6 or 3), 160 = five slices with a second and a third layer's offsets into the
# fragments and the f32 section.
PACKED_SHAPES = [(96, 1), (160, 3)]


@functools.lru_cache(maxsize=None)
def packed_shape_case(dim_ff, layers):
    """A random-init model of the shape with every layer's tensors its own (distinct_layers: a fresh module's layers are copies
    of one), 257 boards and their CPU forwards (shared, never modified)."""
    model = tiny_model(2, dim_ff=dim_ff, num_layers=layers)
    distinct_layers(model.encoder.layers, 5)
    boards = random_boards(257, 11)
    truth, rounded = cpu_forwards(model, boards)
    return model.float(), boards, truth, rounded


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("shape", PACKED_SHAPES, ids=["ff%d-L%d" % s for s in PACKED_SHAPES])
def test_packed_shape_matrix_with_canaries(shape, precision):
    import copy
    from g2048 import DeviceTransformerPolicy, ops
    dim_ff, layers = shape
    model, all_boards, truth, rounded = packed_shape_case(dim_ff, layers)
    pol = DeviceTransformerPolicy(copy.deepcopy(model).to(DEV), precision=precision)
    assert (pol.dim_ff, pol.n_layers) == shape
    for n in (17, 257):
        b = torch.from_numpy(all_boards[:n]).to(DEV)
        probs = torch.full((n + 67, 4), 7.0, device=DEV)
        value = torch.full((n + 67, 1), 7.0, device=DEV)
        ops.tpolicy_forward(b, pol.packed, dim_ff, layers, precision, probs=probs[:n], value=value[:n])
        torch.cuda.synchronize()
        assert torch.all(probs[n:] == 7.0) and torch.all(value[n:] == 7.0), "rows past n were written (n = %d)" % n
        check(precision, probs[:n].cpu().numpy(), value[:n].cpu().numpy(), truth[0][:n], truth[1][:n],
              (rounded[0][:n], rounded[1][:n]), "dim_ff %d L %d n=%d" % (dim_ff, layers, n))
    if layers == 3:
        for i in (0, 130, 256):                              # alone: another wavefront and block than in the large call
            p, v = pol(b[i:i + 1].clone())
            assert torch.equal(p[0], probs[i]) and torch.equal(v[0], value[i]), "board %d alone differs from row %d of the large call" % (i, i)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_outputs_do_not_depend_on_position_or_batch_size(precision):
    from g2048 import DeviceTransformerPolicy
    model, all_boards, _, _ = bench_shape_case()
    pol = DeviceTransformerPolicy(model.to(DEV), precision=precision)
    b = torch.from_numpy(all_boards).to(DEV)
    p1, v1 = [t.clone() for t in pol(b)]
    p2, v2 = pol(b)
    assert torch.equal(p1, p2) and torch.equal(v1, v2), "two launches differ"
    for i in (0, 5, 16, 4097, 40000, 65535, 65536):          # alone
        p, v = pol(b[i:i + 1].clone())
        assert torch.equal(p[0], p1[i]) and torch.equal(v[0], v1[i]), "board %d alone differs from row %d of the large call" % (i, i)
    for start in (3, 1000, 65537 - 17):                      # 17 boards at other offsets within their blocks
        p, v = pol(b[start:start + 17].clone())
        assert torch.equal(p, p1[start:start + 17]) and torch.equal(v, v1[start:start + 17]), "n = 17 from %d differs" % start


def test_rollout_boards_hook_matches_an_observation_wrapper(oracle):
    from g2048 import DeviceTransformerPolicy, RolloutCollector
    pol = DeviceTransformerPolicy(tiny_model(8).to(DEV))

    class ObsWrapper(torch.nn.Module):           # a plain torch policy: re-packs the float observation, calls the same kernel
        def forward(self, obs):
            return pol(torch.round(obs * 15).to(torch.uint8).contiguous())

    n, T, seed = 4096, 16, 5
    for use_graph in (False, True):
        res = RolloutCollector(n, T, pol, device=DEV, seed=seed, use_graph=use_graph).collect()
        a = _traj(res)
        b = _traj(RolloutCollector(n, T, ObsWrapper(), device=DEV, seed=seed, use_graph=use_graph).collect())
        for k in a:
            assert torch.equal(a[k], b[k]), "%s differs (use_graph=%s)" % (k, use_graph)
        assert a["values"].abs().sum() > 0
    replay_and_check(oracle, res, n, T, seed)


def test_graph_replay_after_refresh_uses_the_new_weights():
    from g2048 import DeviceTransformerPolicy, RolloutCollector
    model = tiny_model(6).to(DEV)
    pol = DeviceTransformerPolicy(model)
    pol_old = DeviceTransformerPolicy(model)     # keeps the weights before the optimizer step (never refreshed)
    n, T, seed = 4096, 16, 77
    rc = RolloutCollector(n, T, pol, device=DEV, seed=seed, use_graph=True)
    rc.collect()
    assert rc._graph is not None, "the collector did not capture its loop"
    state = _collector_state(rc)
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    model.train()
    p, v = model(torch.rand(256, 16, device=DEV))
    loss = -(p[:, 0].log().mean()) + v.pow(2).mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    model.eval()
    pol.refresh()
    replayed = _traj(rc.collect())
    fresh = RolloutCollector(n, T, pol, device=DEV, seed=seed, use_graph=True)
    _start_from(fresh, state)
    want = _traj(fresh.collect())
    assert fresh._graph is not None
    for k in want:
        assert torch.equal(replayed[k], want[k]), "replay after refresh differs from a fresh capture in %s" % k
    old = RolloutCollector(n, T, pol_old, device=DEV, seed=seed, use_graph=True)
    _start_from(old, state)
    before = _traj(old.collect())
    assert torch.equal(before["obs"][0], replayed["obs"][0])           # same starting state ...
    assert not torch.equal(before["log_prob"], replayed["log_prob"])   # ... but the replay ran the new weights
    assert not torch.equal(before["values"], replayed["values"])


def test_bad_arguments_launch_nothing():
    from g2048 import DeviceTransformerPolicy, _lib, ops
    L = _lib.lib()
    pol = DeviceTransformerPolicy(tiny_model(1).to(DEV))
    b = torch.from_numpy(random_boards(64, 2)).to(DEV)
    probs = torch.full((64, 4), 3.0, device=DEV)
    value = torch.full((64, 1), 3.0, device=DEV)
    w = pol.packed
    cases = [
        ((b.data_ptr(), w.data_ptr(), probs.data_ptr(), value.data_ptr(), 64, 128, 2, 5, None), b"opts"),
        ((b.data_ptr(), w.data_ptr(), probs.data_ptr(), value.data_ptr(), 64, 48, 2, 0, None), b"dim_ff"),
        ((b.data_ptr(), w.data_ptr(), probs.data_ptr(), value.data_ptr(), 64, 128, 0, 0, None), b"n_layers"),
        ((b.data_ptr() + 4, w.data_ptr(), probs.data_ptr(), value.data_ptr(), 64, 128, 2, 0, None), b"misaligned"),
        ((b.data_ptr(), w.data_ptr() + 8, probs.data_ptr(), None, 64, 128, 2, 0, None), b"misaligned"),
        ((b.data_ptr(), w.data_ptr(), probs.data_ptr(), value.data_ptr() + 2, 64, 128, 2, 0, None), b"misaligned"),
        ((b.data_ptr(), None, probs.data_ptr(), None, 64, 128, 2, 0, None), b"null pointer"),
        ((b.data_ptr(), w.data_ptr(), None, value.data_ptr(), 64, 128, 2, 0, None), b"null pointer"),
    ]
    for args, msg in cases:
        assert L.g2048_tpolicy_forward(*args) == -1
        assert msg in L.g2048_last_error()
    packed = torch.full((ops.tpolicy_packed_bytes("f32", 128, 2),), 9, dtype=torch.uint8, device=DEV)
    plain = torch.zeros(ops.tpolicy_plain_floats(128, 2), device=DEV)
    assert L.g2048_tpolicy_pack(plain.data_ptr(), 128, 2, 3, packed.data_ptr(), None) == -1 and b"precision" in L.g2048_last_error()
    assert L.g2048_tpolicy_pack(plain.data_ptr(), 48, 2, 0, packed.data_ptr(), None) == -1 and b"dim_ff" in L.g2048_last_error()
    assert L.g2048_tpolicy_pack(plain.data_ptr(), 128, 0, 0, packed.data_ptr(), None) == -1 and b"n_layers" in L.g2048_last_error()
    assert L.g2048_tpolicy_pack(None, 128, 2, 0, packed.data_ptr(), None) == -1 and b"null pointer" in L.g2048_last_error()
    torch.cuda.synchronize()
    assert torch.all(probs == 3.0) and torch.all(value == 3.0) and torch.all(packed == 9), "a refused call wrote output"
    with pytest.raises(TypeError):
        pol(b.to(torch.int32))
    with pytest.raises(ValueError):
        ops.tpolicy_forward(b, w, 128, 2, "f32", probs=probs[:10])
    with pytest.raises(ValueError):
        ops.tpolicy_forward(b, w, 2048, 2, "f32")              # the blob was packed for another shape
    # value is optional in the C-ABI: probabilities alone
    only = ops.tpolicy_forward(b, w, 128, 2, "f32", want_value=False)
    assert torch.equal(only, pol(b)[0])
