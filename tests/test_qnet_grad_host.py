"""CPU-side checks of the Q-network's loss and gradient pass (DeviceQNetwork.loss_and_grad, g2048_qnet_loss_grad): the plain-torch
yardstick loss_grad_reference in float64 against the stock module's own autograd through the lines of train_step and against the
reference class's recorded gradients (tests/golden/qnet_grad.npz), the conditions that make the fixture a pin, the refusals, and
the C-ABI's argument validation and workspace arithmetic without a device. The kernels themselves are checked on the GPU
(tests/test_gpu_qnet_grad.py).

Full boards (tiles up to 131,072) at n >= 2: the parameters upstream of layer 0's nearly one-hot softmax have gradients that
even float64 reproduces to 1e-8 only between two spellings of the same function, and float32 not at all; they are compared on
the early boards (codes 0..3) and at n = 1, and the other parameters everywhere. Early boards leave layer 0's attention uniform;
the GPU tests' peaked-attention cases (mid boards, the conditioned module on full boards) are held here to the regime they claim:
the spread of layer 0's softmax, its logits' range, the codes on the boards and a fair stock float32, from the float64 module alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import qnet_grad_ref as R
from conftest import load_golden
from test_gpu_qnet_batch import FAIR_F32, REGIME_CASES, REGIME_IDS
from test_gpu_qnet_grad import regime_case
from test_policy_host import random_boards
from test_qnet_host import RefSpelling, golden_model, random_model

CASES = ("early_17", "early_256", "full_256")


def tensors(t):
    return tuple(torch.from_numpy(np.asarray(x)) for x in t)


def reference(parsed, codes, a, t, w, dtype=torch.float64):
    from g2048 import qnet
    loss, td, q, grads = qnet.loss_grad_reference(parsed, *tensors((codes, a, t, w)), dtype=dtype)
    assert list(grads) == [x for x in parsed.plain_tensors() if isinstance(x, torch.Tensor)], "not in plain order"
    return float(loss), td.numpy().astype(np.float64), q.numpy().astype(np.float64), [g.numpy().astype(np.float64).reshape(-1) for g in grads.values()]


def test_loss_grad_reference_is_the_stock_modules_own_autograd():
    from g2048 import qnet
    _, policy_boards, fixture_model = golden_model()
    early = (random_boards(300, 5) % 4).astype(np.uint8)
    for name, m in (("random init", random_model(2, 64, 2).double()), ("fixture weights", fixture_model)):
        p = qnet.parse(m)
        for kind, boards in (("early", early), ("full", policy_boards)):
            for n in (1, 17, 256):
                codes = boards[:n]
                a, t, w = R.case_inputs(m, codes)
                loss, td, q, g = R.stock_loss_grad(m, codes, a, t, w)
                loss2, td2, q2, g2 = reference(p, codes, a, t, w)
                r = R.ratios(g2, g)
                every = kind == "early" or n == 1
                print("%s, %s boards, n=%d: upstream %.3g, other %.3g of max|g|" % (name, kind, n, r[:R.N_UPSTREAM].max(), r[R.N_UPSTREAM:].max()))
                assert (r if every else r[R.N_UPSTREAM:]).max() <= 1e-9 and np.all(np.isfinite(np.concatenate(g2)))
                assert abs(loss2 - loss) <= 1e-12 * abs(loss) and np.abs(td2 - td).max() <= 1e-12 * td.max() and np.abs(q2 - q).max() <= 1e-9 * np.abs(q).max()
    # three layers and a dim_ff with a main group and a tail step: the yardstick of the GPU tests' shape matrix
    m = random_model(2, 160, 3).double()
    codes = (random_boards(33, 11) % 4).astype(np.uint8)
    a, t, w = R.case_inputs(m, codes)
    loss, td, q, g = R.stock_loss_grad(m, codes, a, t, w)
    loss2, td2, q2, g2 = reference(qnet.parse(m), codes, a, t, w)
    r = R.ratios(g2, g)
    print("random init, dim_ff 160, 3 layers, early boards, n=33: %.3g of max|g| over %d tensors" % (r.max(), len(r)))
    assert len(g) == 6 + 3 * 12 + 2 and r.max() <= 1e-9 and np.all(np.isfinite(np.concatenate(g2)))
    assert abs(loss2 - loss) <= 1e-12 * abs(loss) and np.abs(td2 - td).max() <= 1e-12 * td.max() and np.abs(q2 - q).max() <= 1e-9 * np.abs(q).max()
    assert all(x.grad is None for x in fixture_model.parameters()), "the yardstick must not touch the module's .grad"


def fixture_case(g, case):
    _, policy_boards, model = golden_model()
    n = int(case.split("_")[1])
    codes = g["early_boards"][:n] if case.startswith("early") else policy_boards[:n]
    a, _, w = R.recipe(n)
    return model, codes, a, g[case + "_targets"], w


def test_loss_grad_reference_reproduces_the_fixture():
    from g2048 import qnet
    g = load_golden("qnet_grad.npz")
    assert tuple(g["cases"]) == CASES and g["upstream"].tolist() == [1] * R.N_UPSTREAM + [0] * (len(g["upstream"]) - R.N_UPSTREAM)
    pos = g["positions"]
    for case in CASES:
        model, codes, a, t, w = fixture_case(g, case)
        assert [k for k, _ in model.named_parameters()] == g["tensor_names"].tolist()
        loss, td, q, grads = reference(qnet.parse(model), codes, a, t, w)
        assert abs(loss - float(g[case + "_loss_f64"])) <= 1e-12 * loss and np.abs(td - g[case + "_td_f64"]).max() <= 1e-12 * td.max()
        assert np.abs(q - g[case + "_q_f64"]).max() <= 1e-9 * np.abs(q).max()
        gmax = g[case + "_gmax_f64"]
        err = np.array([np.abs(x[p] - want).max() for x, p, want in zip(grads, pos, g[case + "_g_f64"])]) / gmax
        norm = np.abs(np.array([np.linalg.norm(x) for x in grads]) / g[case + "_norm_f64"] - 1)
        checked = slice(None) if case.startswith("early") else slice(R.N_UPSTREAM, None)
        print("%s: entries %.3g of max|g|, norms %.3g (upstream of the layer-0 softmax: %.3g, %.3g)"
              % (case, err[checked].max(), norm[checked].max(), err[:R.N_UPSTREAM].max(), norm[:R.N_UPSTREAM].max()))
        assert err[checked].max() <= 1e-9 and norm[checked].max() <= 1e-9


def test_fixture_pins_both_huber_branches_every_action_and_a_fair_float32():
    g = load_golden("qnet_grad.npz")
    up = g["upstream"].astype(bool)
    for case in CASES:
        n = int(case.split("_")[1])
        a, offset, w = R.recipe(n)
        q, t = g[case + "_q_f64"], g[case + "_targets"]
        assert t.dtype == np.float32 and np.array_equal(t, (q[np.arange(n), a] + offset).astype(np.float32))
        d = q[np.arange(n), a] - t.astype(np.float64)
        td = np.where(np.abs(d) < 1, 0.5 * d * d, np.abs(d) - 0.5)
        assert np.abs(td - g[case + "_td_f64"]).max() <= 1e-12
        assert abs(float(g[case + "_loss_f64"]) - float((w.astype(np.float64) * td).mean())) <= 1e-12
        quad = (np.abs(d) < 1).mean()
        assert 0.25 <= quad <= 0.75, "a Huber branch holds less than 25 %% of the rows (%s)" % case
        assert np.bincount(a, minlength=4).min() >= 0.1 * n
        err = g[case + "_err_f32"]
        assert np.all(g[case + "_gmax_f64"] > 0)
        if case.startswith("early"):
            assert 0 < err.max() <= 1e-5, "stock float32 is no fair yardstick on %s: %.3g" % (case, err.max())
            sampled = np.abs(g[case + "_g_f32"].astype(np.float64) - g[case + "_g_f64"]).max(axis=1) / g[case + "_gmax_f64"]
            assert np.all(sampled <= err + 1e-12)
        else:
            assert err[~up].max() <= 1e-5
            print("%s: stock float32 autograd upstream of the layer-0 softmax is off by %.3g x max|g| (not a float32 quantity)" % (case, err[up].max()))


@pytest.mark.parametrize("case", REGIME_CASES, ids=REGIME_IDS)
def test_peaked_attention_cases_are_in_the_regime_they_claim(case):
    """The conditions on the inputs of the GPU tests' peaked-attention cases, from the float64 module alone: layer 0's softmax
    spread over a few keys, neither uniform (1 / n) nor one-hot, and stock float32 autograd a fair yardstick for every tensor."""
    regime, dim_ff, layers, n = case
    boards, _, _, _, g64, g32, m64 = regime_case(*case)
    logits, P = R.layer0_attention(m64, boards)
    assert P.shape == (8, n, n) and np.abs(P.sum(-1) - 1).max() <= 1e-12
    top = P.max(-1)
    mean_top, one_hot, yard = top.mean(), (top > 0.999).mean(), R.ratios(g32[3], g64[3]).max()
    largest = np.abs(logits).max()
    print("%s, dim_ff %d L %d n=%d: layer-0 logits %.3g .. %.3g, mean max-P %.3g (1/n = %.3g), one-hot rows %.3g, codes up to %d, "
          "yardstick %.3g" % (case + (logits.min(), logits.max(), mean_top, 1 / n, one_hot, boards.max(), yard)))
    assert 0 < yard <= FAIR_F32, "stock float32 autograd is no fair yardstick on this case: %.3g" % yard
    if regime in ("mid", "distinct"):
        layers1 = list(m64.transformer.layers[1:])
        same = all(torch.equal(x, y) for a, b in zip(layers1, layers1[1:]) for x, y in zip(a.parameters(), b.parameters()))
        assert same == (regime == "mid"), "a fresh module's layers are copies of one; the 'distinct' module's must not be"
        assert boards.max() == 7
        assert mean_top >= 0.15 and one_hot <= 0.01
    else:
        assert one_hot <= 0.05
        # the largest logit in magnitude. It is negative (-111; the largest positive one is 37): a row spans more than float32 exp's
        # range, so a shift by anything below the row's maximum overflows, but exp of the unshifted logits does not; a softmax
        # without its max subtraction is caught by the full boards under the stock module (logits 1e9), not by these cases
        assert largest > 88.8, "every layer-0 logit is within float32 exp's range: %.3g" % largest
        assert boards.max() == 17 and (boards >= 12).sum() >= 16
        assert all(np.abs(g).max() > 0 for g in g64[3][:R.N_UPSTREAM])


class Stub:
    """DeviceQNetwork's own checks, reached without a device."""

    def __new__(cls, parsed, precision):
        from g2048 import DeviceQNetwork

        class S(DeviceQNetwork):
            def __init__(self, parsed, precision):
                self.parsed, self.precision = parsed, precision
        return S(parsed, precision)


def test_loss_and_grad_refusals_name_their_reason():
    from g2048 import ops, qnet
    torch.manual_seed(4)
    b = torch.zeros((4, 16), dtype=torch.uint8)
    a, t, w = torch.zeros(4, dtype=torch.int64), torch.zeros(4), torch.ones(4)
    ok = qnet.parse(RefSpelling(64, 2).eval())
    p4 = qnet.parse(RefSpelling(64, 1, nhead=4).eval())
    pbf = qnet.parse(RefSpelling(64, 2, batch_first=True).eval())
    with pytest.raises(ValueError, match="bf16.*refused.*1e9"):
        Stub(ok, "bf16").loss_and_grad(b, a, t, w)
    for call in (lambda p: Stub(p, "f32").loss_and_grad(b, a, t, w), lambda p: qnet.loss_grad_reference(p, b, a, t, w)):
        with pytest.raises(ValueError, match="nhead 4, expected 8"):
            call(p4)
        with pytest.raises(ValueError, match="batch_first=True"):
            call(pbf)
    for call in (lambda *x: Stub(ok, "f32").loss_and_grad(b, *x), lambda *x: qnet.loss_grad_reference(ok, b, *x)):
        with pytest.raises(TypeError, match="actions must be torch.int64"):
            call(a.to(torch.int32), t, w)
        with pytest.raises(TypeError, match="targets must be torch.float32"):
            call(a, t.double(), w)
        with pytest.raises(TypeError, match="weights must be torch.float32"):
            call(a, t, w.to(torch.float16))
        with pytest.raises(ValueError, match=r"actions must have shape \(4,\)"):
            call(a[:3], t, w)
        with pytest.raises(ValueError, match=r"targets must have shape \(4,\)"):
            call(a, t.reshape(4, 1), w)
        with pytest.raises(ValueError, match=r"weights must have shape \(4,\)"):
            call(a, t, torch.ones(5))
        with pytest.raises(TypeError, match="weights must be a torch.Tensor"):
            call(a, t, [1.0] * 4)
    import __graft_entry__ as ge
    ge.build()
    with pytest.raises(ValueError, match="1 .. 4096 boards.*not truncated"):
        ops.qnet_grad_workspace_bytes(4097, 64, 2)
    with pytest.raises(ValueError, match="1 .. 4096"):
        ops.qnet_grad_workspace_bytes(0, 64, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.qnet_loss_grad(b, torch.zeros(ops.qnet_plain_floats(64, 2)), a, t, w, 64, 2)


def test_grad_entry_points_validate_without_device():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    L = _lib.lib()
    assert L.g2048_abi_version() == 5
    hdr = open(__import__("os").path.join(__import__("conftest").REPO, "include", "g2048.h")).read()
    assert "g2048_qnet_loss_grad" in hdr and "g2048_qnet_grad_workspace" in hdr
    W = L.g2048_qnet_grad_workspace
    for ff, layers in ((32, 1), (64, 2), (2048, 2), (4096, 3), (96, 1), (160, 3), (224, 2), (416, 1)):
        last = 0
        for n in (1, 15, 16, 17, 255, 256, 257, 1025, 4096):
            nb = W(n, ff, layers)
            assert nb > 0 and nb >= last and nb % 16 == 0
            # at least what the backward reads again: per board the conv outputs, per layer input, qkv, attention, two pre-norm
            # sums and the hidden layer, and the last layer's output
            assert nb >= 4 * n * (1024 + 800 + layers * (128 + 384 + 128 + 256 + ff) + 128)
            last = nb
    assert W(256, 2048, 2) < 16 << 20
    for bad in ((0, 64, 2), (4097, 64, 2), (16, 48, 2), (16, 0, 2), (16, -32, 2), (16, 64, 0), (16, 64, 65), (16, 64, -1)):
        assert W(*bad) == 0, bad
    buf = (C.c_uint8 * 256)()
    p = (C.addressof(buf) + 15) & ~15
    F = L.g2048_qnet_loss_grad

    def call(n=8, ff=64, layers=2, **ptr):
        names = ("boards", "plain", "actions", "targets", "weights", "grad", "td", "loss", "q", "workspace")
        v = {k: ptr.get(k, p) for k in names}
        return F(v["boards"], v["plain"], v["actions"], v["targets"], v["weights"], n, ff, layers, v["grad"], v["td"], v["loss"], v["q"],
                 v["workspace"], None)

    assert F(None, None, None, None, None, 0, 64, 2, None, None, None, None, None, None) == 0          # n == 0: nothing to do
    for name in ("boards", "plain", "actions", "targets", "weights", "grad", "td", "loss", "q", "workspace"):
        assert call(**{name: None}) == -1 and b"g2048_qnet_loss_grad: null pointer" in L.g2048_last_error(), name
    for name, off in (("boards", 4), ("plain", 8), ("grad", 8), ("q", 4), ("workspace", 8), ("actions", 4), ("targets", 2), ("weights", 1),
                      ("td", 2), ("loss", 3)):
        assert call(**{name: p + off}) == -1 and b"misaligned" in L.g2048_last_error(), name
    assert call(n=4097) == -1 and b"G2048_QNET_BATCH_MAX" in L.g2048_last_error() and b"not truncated" in L.g2048_last_error()
    assert call(ff=48) == -1 and b"dim_ff" in L.g2048_last_error()
    assert call(layers=0) == -1 and b"n_layers" in L.g2048_last_error()
