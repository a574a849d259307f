"""CPU side of the Q-network's training-mode dropout: the mask rule's restatement, the masked stock module against a plain-ops
restatement, the argument checks of the training library's entry points (no device is touched), DeviceQNetwork's `dropout`
argument, and the regime condition of every case of tests/test_gpu_qnet_dropout.py -- the float32 masked module's own error
against the float64 one lies in (0, 1e-5], the bound tests/test_gpu_qnet_grad.py applies to its yardstick -- with the seed the
cases use being the first from 0 upwards that satisfies it."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import qnet_dropout_ref as D
import qnet_grad_ref as R
from test_qnet_host import RefSpelling, random_model


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    return _lib


def test_keep_rate_of_the_restatement():
    for site, n, dim_ff in ((0, 257, 64), (1, 257, 64), (2, 257, 2048), (3, 1025, 64)):
        for p in (0.1, 0.5):
            keep = D.keep_mask(5, 9, 1, site, p, n, dim_ff)
            assert keep.shape == D.site_shape(site, n, dim_ff) and keep.dtype == np.bool_
            sigma = (p * (1 - p) / keep.size) ** 0.5
            assert abs(keep.mean() - (1 - p)) < 5 * sigma, (site, p, keep.mean())
    assert D.keep_mask(5, 9, 1, 2, 0.0, 17, 64).all()                                  # T = 0: every draw is kept


def test_masks_differ_across_seed_call_layer_and_site_and_windows_are_slices():
    base = D.keep_mask(1, 2, 0, 1, 0.5, 33, 64)
    for other in (D.keep_mask(2, 2, 0, 1, 0.5, 33, 64), D.keep_mask(1, 3, 0, 1, 0.5, 33, 64), D.keep_mask(1, 2 + (1 << 32), 0, 1, 0.5, 33, 64),
                  D.keep_mask(1, 2, 1, 1, 0.5, 33, 64), D.keep_mask(1, 2, 0, 3, 0.5, 33, 64)):
        assert other.shape == base.shape and 0.3 < (other != base).mean() < 0.7
    flat = [D.keep_mask(1, 2, 0, s, 0.5, 33, 64).reshape(-1)[:33 * 64] for s in range(4)]
    assert all(0.3 < (flat[a] != flat[b]).mean() < 0.7 for a in range(4) for b in range(a))
    whole = D.keep_mask(1, 2, 2, 0, 0.1, 33, 64)
    assert np.array_equal(D.keep_mask(1, 2, 2, 0, 0.1, 33, 64, rows=(250, 14)), whole[250:])
    assert np.array_equal(D.keep_mask(1, 2, 2, 0, 0.1, 33, 64, rows=(0, 5)), whole[:5])


def test_the_float32_multiplier_is_torchs():
    """torch's dropout is input * (keep / (1 - p)) with the division in the input's dtype; the project multiplies by
    float32(1 / (1 - p)) formed in double. Bit for bit the same at every probability the cases use."""
    x = torch.randn(4096, generator=torch.Generator().manual_seed(1))
    for p in (0.1, 0.5, 0.3, 0.2):
        keep = torch.from_numpy(D.keep_mask(3, 1, 0, 1, p, 32, 64).reshape(-1))
        assert torch.equal(x * (keep.float() / (1 - p)), x * (keep.float() * float(D.scale32(p)))), p
        assert torch.equal(x * keep.float().div_(1 - p), x * D.multiplier(3, 1, 0, 1, p, 32, 64, torch.float32).reshape(-1)), p


@pytest.mark.parametrize("p4", (D.P4, D.UNEQUAL), ids=("p0.1", "unequal"))
def test_the_patched_stock_module_is_the_plain_ops_restatement(p4):
    for shape, n in (((2, 64, 2), 17), ((12, 32, 1), 33)):
        model, boards = D.case_model("early", shape)
        m64 = D.training_copy(model, p4, torch.float64)
        got, want = D.masked_forward(m64, p4, 11, D.HIGH_INDEX, boards[:n]), D.plain_forward(m64, p4, 11, D.HIGH_INDEX, boards[:n])
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), np.abs(got - want).max()
        other = D.masked_forward(m64, p4, 11, D.HIGH_INDEX + 1, boards[:n])
        assert np.abs(other - want).max() > 1e-3 * np.abs(want).max(), "another call index must give other masks"
        with torch.no_grad():
            plain = copy.deepcopy(model).double().eval()(R.tile_values(boards[:n], torch.float64)).numpy()
        assert np.abs(plain - want).max() > 1e-3 * np.abs(want).max(), "the masks must change the function"
    assert torch.nn.functional.dropout.__module__ == "torch.nn.functional", "feeding() must restore what it replaced"


def _aligned_base():
    buf = (C.c_uint8 * 4096)()
    return buf, (C.addressof(buf) + 63) & ~63


def test_argument_checks_of_the_training_entry_points(built):
    """Every refusal happens before any device call, with a message in the training library's own error string."""
    T = built.train_lib()
    assert T.g2048_train_abi_version() == built.TRAIN_ABI_VERSION == 1
    err = lambda: T.g2048_train_last_error().decode()
    buf, b = _aligned_base()
    p4 = lambda *v: (C.c_double * 4)(*v)
    ok = p4(0.1, 0.1, 0.1, 0.1)
    fwd = lambda **kw: T.g2048_qnet_forward_batch_dropout(*[kw.get(k, d) for k, d in (("boards", b), ("plain", b), ("q", b), ("n", 4), ("ff", 64),
                                                           ("layers", 2), ("p", ok), ("seed", 0), ("call", 0), ("ws", b), ("stream", None))])
    grad = lambda **kw: T.g2048_qnet_loss_grad_dropout(*[kw.get(k, d) for k, d in (("boards", b), ("plain", b), ("a", b), ("t", b), ("w", b), ("n", 4),
                                                        ("ff", 64), ("layers", 2), ("p", ok), ("seed", 0), ("call", 0), ("grad", b), ("td", b),
                                                        ("loss", b), ("q", b), ("ws", b), ("stream", None))])
    mask = lambda **kw: T.g2048_qnet_dropout_mask(*[kw.get(k, d) for k, d in (("seed", 0), ("call", 0), ("layer", 0), ("site", 0), ("p", 0.1), ("n", 4),
                                                   ("ff", 64), ("first", 0), ("rows", 4), ("out", b), ("stream", None))])
    for f, name in ((fwd, "g2048_qnet_forward_batch_dropout"), (grad, "g2048_qnet_loss_grad_dropout")):
        assert f(n=0) == 0 and f(n=0, boards=None, p=None) == 0                                        # n = 0: nothing to do
        for key in ("boards", "plain", "q", "ws", "p") + (("a", "t", "w", "grad", "td", "loss") if f is grad else ()):
            assert f(**{key: None}) == -1 and err() == name + ": null pointer", key
        assert f(boards=b + 1) == -1 and "misaligned" in err()
        assert f(n=built.QNET_BATCH_MAX + 1) == -1 and "G2048_QNET_BATCH_MAX" in err() and err().startswith(name)
        for bad in (dict(ff=48), dict(ff=0), dict(layers=0), dict(layers=65)):
            assert f(**bad) == -1 and "dim_ff" in err(), bad
        for bad in (p4(0.1, 1.0, 0, 0), p4(-0.1, 0, 0, 0), p4(0, 0, float("nan"), 0), p4(0, 0, 0, float("inf"))):
            assert f(p=bad) == -1 and "0 <= p < 1" in err(), list(bad)
    assert mask(n=0) == 0 and mask(rows=0) == 0 and mask(n=0, out=None) == 0
    assert mask(out=None) == -1 and "null pointer" in err()
    assert mask(n=built.QNET_BATCH_MAX + 1) == -1 and "G2048_QNET_BATCH_MAX" in err()
    assert mask(ff=48) == -1 and "dim_ff" in err()
    for bad in (dict(layer=-1), dict(layer=64), dict(site=-1), dict(site=4)):
        assert mask(**bad) == -1 and ("layer" in err() if "layer" in bad else "site" in err()), bad
    for bad in (1.0, -0.5, float("nan")):
        assert mask(p=bad) == -1 and "0 <= p < 1" in err()
    assert mask(first=30, rows=3) == -1 and "past the site's matrix" in err()                          # site 0 at n = 4: 32 rows
    assert mask(first=33, rows=1) == -1 and mask(site=1, first=2, rows=3) == -1 and mask(site=2, first=0, rows=5) == -1
    assert mask(first=2 ** 63, rows=2 ** 63) == -1, "a window whose end wraps round must be refused"
    assert T.g2048_qnet_train_workspace(0, 64, 2) == 0 and T.g2048_qnet_train_workspace(built.QNET_BATCH_MAX + 1, 64, 2) == 0
    assert T.g2048_qnet_train_workspace(4, 48, 2) == 0 and T.g2048_qnet_train_workspace(4, 64, 0) == 0
    for n in (1, 17, 4096):
        assert T.g2048_qnet_train_workspace(n, 64, 2) == built.lib().g2048_qnet_grad_workspace(n, 64, 2) + (n + 15) // 16 * 16 * 128 * 4
    assert built.lib().g2048_last_error() != T.g2048_train_last_error() or not err(), "the two libraries keep their own error strings"


def test_ops_refuse_bad_dropout_arguments_without_a_device():
    from g2048 import ops
    assert ops.qnet_dropout_p(None) is None and ops.qnet_dropout_p(0) is None and ops.qnet_dropout_p((0, 0, 0, 0)) is None
    assert ops.qnet_dropout_p(0.1) == (0.1,) * 4 and ops.qnet_dropout_p([0.3, 0, 0.2, 0.1]) == D.UNEQUAL
    for bad in (1.0, -0.1, float("nan"), (0.1, 0.2), (0.1, 0.1, 0.1, 1.5)):
        with pytest.raises(ValueError):
            ops.qnet_dropout_p(bad)
    for kw in (dict(site=4), dict(layer=64), dict(p=1.0), dict(n=4097), dict(first_row=30, rows=3), dict(first_row=-1)):
        with pytest.raises(ValueError):
            ops.qnet_dropout_mask(**{**dict(n=4, layer=0, site=0, p=0.1), **kw})


def test_the_constructors_dropout_argument():
    """The argument is parsed before anything touches a device: a bad one is a ValueError that names the network, a good one
    reaches the device check."""
    from g2048 import DeviceQNetwork, qnet
    model = random_model(2, 64, 2)
    parsed = qnet.parse(model)
    assert qnet.dropout_of(parsed, 0.0) == (0.0,) * 4 and qnet.dropout_of(parsed, 0.25) == (0.25,) * 4
    assert qnet.dropout_of(parsed, D.UNEQUAL) == D.UNEQUAL
    assert qnet.dropout_of(parsed, "module") == (0.1,) * 4                              # nn.TransformerEncoderLayer's default
    other = RefSpelling(64, 2, dropout=0.3).eval()
    assert qnet.dropout_of(qnet.parse(other), "module") == (0.3,) * 4
    other.transformer.layers[0].dropout1.p = 0.2
    other.transformer.layers[1].dropout1.p = 0.2
    other.transformer.layers[1].self_attn.dropout = 0.0
    with pytest.raises(ValueError, match="DeviceQNetwork: dropout=\"module\": encoder layer 1"):
        qnet.dropout_of(qnet.parse(other), "module")
    other.transformer.layers[0].self_attn.dropout = 0.0
    assert qnet.dropout_of(qnet.parse(other), "module") == (0.0, 0.2, 0.3, 0.3)
    for bad in (1.0, -0.1, float("nan"), (0.1, 0.2), "stock", (0.1, 0.1, 0.1, None)):
        with pytest.raises(ValueError, match="DeviceQNetwork"):
            DeviceQNetwork(model, dropout=bad)
    with pytest.raises(RuntimeError, match="ROCm device"):                              # parsed, then: the module is on the CPU
        DeviceQNetwork(model, dropout="module", dropout_seed=7)
    with pytest.raises(ValueError, match="training mode"):                              # still refused, whatever `dropout` says
        DeviceQNetwork(copy.deepcopy(model).train(), dropout=0.1)


def _conditions(seed):
    """{case id: the float32 yardstick} of every GPU case at dropout seed `seed`."""
    out = {}
    for case in D.LOSS_CASES:
        want, f32 = D.loss_case(case, seed)[5:]
        out[D.case_id(case)] = D.yardstick(want, f32)
    for n in D.FORWARD_SIZES:
        (q_on, q_t), (f_on, f_t) = D.forward_case(n, seed)[5]
        out["forward-n%d-online" % n] = np.abs(f_on - q_on).max() / np.abs(q_on).max()
        out["forward-n%d-target" % n] = np.abs(f_t - q_t).max() / np.abs(q_t).max()
    steps64, steps32 = D.closed_round(torch.float64, seed)[1], D.closed_round(torch.float32, seed)[1]
    for k, (s64, s32) in enumerate(zip(steps64, steps32)):
        out["round-step%d" % (k + 1)] = R.ratios(s32["grads"], s64["grads"]).max()
    return out


def test_every_gpu_case_has_a_fair_float32_yardstick_at_the_first_such_seed():
    for seed in range(D.DROPOUT_SEED + 1):
        found = _conditions(seed)
        fair = {k: 0 < v <= D.FAIR_F32 for k, v in found.items()}
        print("dropout seed %d: yardsticks %.3g .. %.3g; unfair: %s" % (seed, min(found.values()), max(found.values()),
                                                                        {k: "%.3g" % found[k] for k, ok in fair.items() if not ok}))
        if seed < D.DROPOUT_SEED:
            assert not all(fair.values()), "seed %d already satisfies every case: DROPOUT_SEED must be the first such seed" % seed
        else:
            assert all(fair.values()), {k: found[k] for k, ok in fair.items() if not ok}
            print("  " + " ".join("%s=%.3g" % kv for kv in found.items()))
    # the closed round's decisions do not hang on a rounding: the online Q's margins exceed what float32 moves them by
    for s64, s32 in zip(D.closed_round(torch.float64)[1], D.closed_round(torch.float32)[1]):
        assert np.array_equal(s64["next_actions"], s32["next_actions"])
