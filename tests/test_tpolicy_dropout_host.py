"""CPU side of the transformer policy's training-mode dropout: the mask rule's restatement against draws worked out with Python
integers, the masked stock module against the plain-ops restatement (g2048.tpolicy.loss_grad_reference with `multipliers`), the
conditions of every case of tests/test_gpu_tpolicy_dropout.py under the masks, the argument checks of the training library's three
device entry points (no device is touched), its workspace query, and DeviceTransformerPolicy's `dropout` argument.

Measured on the CPU: the masked stock float64 module and the plain-ops restatement agree to 9e-16 .. 1.5e-15 of the largest entry
(loss parts, probs, value and every gradient tensor); the assertion leaves a margin of about 100 x."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import tpolicy_dropout_ref as D
import tpolicy_grad_ref as R
from ppo_dropout_ref import rng_keys, threshold
from test_tpolicy_host import RefSpelling

M32 = 0xFFFFFFFF
PLAIN_OPS_GAP = 2e-13                 # about 100 x the 1.5e-15 measured


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    return _lib


def draw(k0, k1, ident, ctr=0):
    """rng_draw (csrc/g2048_board.h) with Python integers."""
    h = (ident & M32) ^ k0
    h ^= h >> 16; h = h * 0x85EBCA6B & M32; h ^= h >> 13; h = h * 0xC2B2AE35 & M32; h ^= h >> 16       # noqa: E702
    h = (h + k1 + (ident >> 32) * 0x9E3779B1 + ctr * 0x85EBCA77) & M32
    h ^= h >> 16; h = h * 0x7FEB352D & M32; h ^= h >> 15; h = h * 0x846CA68B & M32; h ^= h >> 16       # noqa: E702
    return h


def test_the_restatement_against_draws_worked_out_by_hand():
    """A few elements of every site, each from its coordinates: element e of site s of layer L is kept iff
    rng_draw(rng_keys(seed, 13, call), ((4 L + s) << 32) | e, 0) >= floor(p 2^32)."""
    n, ff, seed = 5, 96, 3
    for call in (7, D.HIGH_INDEX):
        k0, k1 = rng_keys(seed, 13, call)
        for layer in (0, 1):
            for p in (0.1, 0.5):
                m0 = D.keep_mask(seed, call, layer, 0, p, n, ff)
                for board, head, query, key in ((0, 0, 0, 0), (2, 3, 5, 11), (4, 3, 15, 15), (1, 2, 9, 4)):
                    e = ((board * 4 + head) * 16 + query) * 16 + key
                    assert m0[(board * 4 + head) * 16 + query, key] == (draw(k0, k1, ((4 * layer + 0) << 32) | e) >= threshold(p))
                for site, width in ((1, 64), (2, ff), (3, 64)):
                    m = D.keep_mask(seed, call, layer, site, p, n, ff)
                    for board, cell, feature in ((0, 0, 0), (3, 7, width - 1), (4, 15, 17), (2, 1, 33)):
                        token = 16 * board + cell
                        assert m[token, feature] == (draw(k0, k1, ((4 * layer + site) << 32) | (token * width + feature)) >= threshold(p))
    assert [D.site_shape(s, n, ff) for s in range(4)] == [(320, 16), (80, 64), (80, 96), (80, 64)]
    assert D.keep_mask(5, 9, 1, 2, 0.0, 17, 64).all()                                  # T = 0: every draw is kept
    whole = D.keep_mask(1, 2, 1, 2, 0.1, 3, 96)
    assert np.array_equal(D.keep_mask(1, 2, 1, 2, 0.1, 3, 96, rows=(40, 8)), whole[40:])
    for site, nn, dim_ff in ((0, 33, 64), (2, 33, 2048)):
        for p in (0.1, 0.5):
            keep = D.keep_mask(5, 9, 1, site, p, nn, dim_ff)
            assert abs(keep.mean() - (1 - p)) < 5 * (p * (1 - p) / keep.size) ** 0.5, (site, p, keep.mean())


@pytest.mark.parametrize("case", [c for c in D.LOSS_CASES if c[0] in (1, 17) or c[:2] == (33, 32)], ids=D.case_id)
def test_the_masked_stock_module_is_the_plain_ops_restatement(case):
    c = D.loss_case(case)
    got = D.plain_loss_grad(c)
    gap = max(R.ratios(got["grads"], c.want["grads"]).max(), R.rel(got["losses"], c.want["losses"]), R.rel(got["probs"], c.want["probs"]),
              R.rel(got["value"], c.want["value"]))
    print("%s: the plain-ops restatement is %.3g of the largest entry from the masked stock float64 module" % (D.case_id(case), gap))
    assert gap <= PLAIN_OPS_GAP and np.all(got["eps"] == 0)
    other = D.masked_loss_grad(c.train64, c.p4, c.seed, c.index + 1, *c.args)
    assert R.rel(other["probs"], c.want["probs"]) > 1e-3, "another call index must give other masks"
    plain = R.stock_loss_grad(copy.deepcopy(c.model32).double().eval(), *c.args)
    assert R.rel(plain["probs"], c.want["probs"]) > 1e-3, "the masks must change the function"
    from g2048 import tpolicy
    parsed = tpolicy.parse(copy.deepcopy(c.model32).double().eval())
    args = [torch.from_numpy(np.asarray(t)) for t in c.args]
    flat = tpolicy.loss_grad_reference(parsed, *args)[3].numpy()
    assert R.ratios(R.split(parsed, flat)[0], plain["grads"]).max() <= PLAIN_OPS_GAP, "without multipliers nothing changes"
    assert torch.nn.functional.dropout.__module__ == "torch.nn.functional", "feeding() must restore what it replaced"


@pytest.mark.parametrize("case", D.LOSS_CASES, ids=D.case_id)
def test_every_case_meets_its_conditions_under_the_masks_at_the_first_such_seed(case):
    c = D.loss_case(case)
    print("%s, dropout seed %d: yardstick %.3g, clipped share %.2f, max|value| %.2f" % (D.case_id(case), c.seed, c.yardstick, c.clipped_share,
                                                                                         c.max_value))
    c.conditions()
    for seed in range(c.seed):
        assert D.Case(case, seed).failed(), "seed %d already meets every condition: the case's seed must be the first such seed" % seed


def test_the_closed_update_has_a_fair_yardstick_per_epoch():
    steps64, steps32 = D.closed_update(torch.float64)[2], D.closed_update(torch.float32)[2]
    for e, (s64, s32) in enumerate(zip(steps64, steps32)):
        yard = R.ratios(s32["grads"], s64["grads"]).max()
        moved = np.abs(s32["params"] - s64["params"]).max() / np.abs(s64["params"]).max()
        print("epoch %d: the float32 masked module's gradients %.3g, its weights after the step %.3g of the largest" % (e, yard, moved))
        assert 0 < yard <= D.FAIR_F32 and moved > 0


def test_argument_checks_happen_before_any_device_call(built):
    """Host addresses that are never dereferenced: every refusal is decided from the arguments alone, and N = 0 returns 0."""
    T = built.ttrain_lib()
    assert T.g2048_ttrain_abi_version() == built.TTRAIN_ABI_VERSION == 1
    err = lambda: T.g2048_ttrain_last_error().decode()      # noqa: E731
    n, ff, layers = 17, 96, 2
    nb = T.g2048_tpolicy_train_workspace(n, ff, layers)
    p = 0x10000                                              # 16-byte aligned, not null
    f = C.c_float
    p4 = lambda *v: (C.c_double * 4)(*v)                     # noqa: E731
    ok = p4(0.1, 0.1, 0.1, 0.1)

    def grad(boards=p, plain=p, actions=p, old=p, adv=p, ret=p, n=n, ff=ff, layers=layers, p4=ok, clip=0.3, vc=0.4, ec=0.05, grad=p, losses=p,
             probs=p, value=p, ws=p, nb=nb):
        return T.g2048_tpolicy_loss_grad_dropout(boards, plain, actions, old, adv, ret, n, ff, layers, p4, 3, D.HIGH_INDEX, f(clip), f(vc), f(ec),
                                                 grad, losses, probs, value, ws, nb, None)

    def fwd(boards=p, plain=p, n=n, ff=ff, layers=layers, p4=ok, probs=p, value=p, ws=p, nb=nb):
        return T.g2048_tpolicy_forward_dropout(boards, plain, n, ff, layers, p4, 3, D.HIGH_INDEX, probs, value, ws, nb, None)

    def mask(layer=0, site=0, prob=0.1, n=4, ff=64, first=0, rows=4, out=p):
        return T.g2048_tpolicy_dropout_mask(3, D.HIGH_INDEX, layer, site, prob, n, ff, first, rows, out, None)

    for call, name, pointers, misaligned in (
            (grad, "g2048_tpolicy_loss_grad_dropout", ("boards", "plain", "actions", "old", "adv", "ret", "grad", "losses", "probs", "value", "ws", "p4"),
             (("boards", 8), ("plain", 4), ("grad", 8), ("probs", 4), ("ws", 8), ("actions", 4), ("old", 2), ("losses", 1), ("value", 2))),
            (fwd, "g2048_tpolicy_forward_dropout", ("boards", "plain", "probs", "value", "ws", "p4"),
             (("boards", 8), ("plain", 4), ("probs", 4), ("ws", 8), ("value", 2)))):
        assert call(n=0) == 0 and call(n=0, boards=None, ws=None, nb=0, p4=None) == 0, "N = 0 returns G2048_OK and launches nothing"
        for key in pointers:
            assert call(**{key: None}) == -1 and err() == name + ": null pointer", key
        assert call(n=1025, nb=1 << 40) == -1 and "1024" in err() and err().startswith(name)
        for bad in (dict(ff=48), dict(ff=0), dict(layers=0), dict(layers=65)):
            assert call(**bad) == -1 and "dim_ff" in err(), bad
        assert call(nb=nb - 1) == -1 and "workspace" in err() and str(nb) in err() and "g2048_tpolicy_train_workspace" in err()
        assert call(nb=built.tlearn_lib().g2048_tpolicy_grad_workspace(n, ff, layers)) == -1, "the learner library's workspace is too small"
        for key, off in misaligned:
            assert call(**{key: p + off}) == -1 and "misaligned" in err(), key
        for bad in (p4(0.1, 1.0, 0, 0), p4(-0.1, 0, 0, 0), p4(0, 0, float("nan"), 0), p4(0, 0, 0, float("inf"))):
            assert call(p4=bad) == -1 and "0 <= p < 1" in err(), list(bad)
    for key in ("clip", "vc", "ec"):
        assert grad(**{key: -0.1}) == -1 and grad(**{key: float("nan")}) == -1 and grad(**{key: float("inf")}) == -1, key
        assert "finite" in err()
    assert mask(n=0) == 0 and mask(rows=0) == 0 and mask(n=0, out=None) == 0
    assert mask(out=None) == -1 and "null pointer" in err()
    assert mask(n=1025) == -1 and "1024" in err()
    assert mask(ff=48) == -1 and "dim_ff" in err()
    for bad in (dict(layer=-1), dict(layer=64), dict(site=-1), dict(site=4)):
        assert mask(**bad) == -1 and ("layer" in err() if "layer" in bad else "site" in err()), bad
    for bad in (1.0, -0.5, float("nan")):
        assert mask(prob=bad) == -1 and "0 <= p < 1" in err()
    assert mask(first=254, rows=3) == -1 and "past the site's matrix" in err()                         # site 0 at n = 4: 256 rows
    assert mask(first=257, rows=1) == -1 and mask(site=1, first=62, rows=3) == -1 and mask(site=2, first=0, rows=65) == -1
    assert mask(first=2 ** 63, rows=2 ** 63) == -1, "a window whose end wraps round must be refused"
    assert built.tlearn_lib().g2048_tlearn_last_error() != T.g2048_ttrain_last_error() or not err(), "each library keeps its own error string"


def test_workspace_query_refuses_grows_and_keeps_16_byte_multiples(built):
    ws, base = built.ttrain_lib().g2048_tpolicy_train_workspace, built.tlearn_lib().g2048_tpolicy_grad_workspace
    assert ws(0, 2048, 2) == 0 and ws(1025, 2048, 2) == 0 and ws(64, 48, 2) == 0 and ws(64, 0, 2) == 0 and ws(64, 2048, 0) == 0
    assert ws(64, 2048, 65) == 0 and ws(64, 65568, 2) == 0
    assert 0 < ws(1, 32, 1) < ws(2, 32, 1) < ws(17, 32, 1) < ws(1024, 32, 1)
    assert ws(64, 32, 2) < ws(64, 64, 2) < ws(64, 2048, 2) and ws(64, 2048, 1) < ws(64, 2048, 2)
    for n in (1, 3, 17, 1024):
        for ff in (32, 96, 2048):
            for l in (1, 3):
                assert ws(n, ff, l) % 16 == 0 and ws(n, ff, l) == base(n, ff, l) + 16 * n * 64 * 4, "one [16 n][64] float array more"
    from g2048 import ops
    with pytest.raises(ValueError, match="1024"):
        ops.tpolicy_train_workspace_bytes(1025, 2048, 2)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.tpolicy_train_workspace_bytes(64, 48, 2)
    for kw in (dict(site=4), dict(layer=64), dict(p=1.0), dict(n=1025), dict(first_row=254, rows=3), dict(first_row=-1)):
        with pytest.raises(ValueError):
            ops.tpolicy_dropout_mask(**{**dict(n=4, layer=0, site=0, p=0.1), **kw})


def test_the_constructors_dropout_argument_and_the_dropout_state():
    """The argument is parsed before anything touches a device: a bad one is a ValueError that names the network, a good one
    reaches the device check."""
    from g2048 import DeviceTransformerPolicy, _encoder_net as E, qnet, tpolicy
    model = R.stock_module(96, 2)
    parsed = tpolicy.parse(model)
    of = lambda p, d: E.dropout_of(tpolicy.NAME, p, d)      # noqa: E731
    assert of(parsed, 0.0) == (0.0,) * 4 and of(parsed, 0.25) == (0.25,) * 4 and of(parsed, D.UNEQUAL) == D.UNEQUAL
    assert of(parsed, "module") == (0.1,) * 4, "the reference module builds its layers with torch's default dropout"
    other = copy.deepcopy(model)
    other.transformer_encoder.layers[1].dropout1.p = 0.2
    with pytest.raises(ValueError, match="DeviceTransformerPolicy: dropout=\"module\": encoder layer 1"):
        of(tpolicy.parse(other), "module")
    other.transformer_encoder.layers[0].dropout1.p = 0.2
    assert of(tpolicy.parse(other), "module") == (0.1, 0.2, 0.1, 0.1)
    for bad in (1.0, -0.1, float("nan"), (0.1, 0.2, 0.3), "x", (0.1, 0.1, 0.1, None)):
        with pytest.raises(ValueError, match="DeviceTransformerPolicy"):
            DeviceTransformerPolicy(model, dropout=bad)
    with pytest.raises(RuntimeError, match="ROCm device"):                              # parsed, then: the module is on the CPU
        DeviceTransformerPolicy(model, dropout="module", dropout_seed=7)
    with pytest.raises(ValueError, match="training mode"):                              # still refused, whatever `dropout` says
        DeviceTransformerPolicy(copy.deepcopy(model).train(), dropout=0.1)
    assert qnet.dropout_of.__doc__ and callable(E.dropout_of), "the Q-network binds the shared function"
    # the state: no device is needed for the three methods
    net = DeviceTransformerPolicy.__new__(DeviceTransformerPolicy)
    net.dropout_seed, net.dropout_index = 5, 0
    assert net.dropout_state() == (5, 0) and net._next_index() == 0 and net.dropout_state() == (5, 1)
    net.set_dropout_state((2 ** 64 + 9, D.HIGH_INDEX))
    assert net.dropout_state() == (9, D.HIGH_INDEX)
    twin = DeviceTransformerPolicy.__new__(DeviceTransformerPolicy)
    twin.set_dropout_state(net.dropout_state())
    assert twin.dropout_state() == net.dropout_state()
    with pytest.raises(ValueError, match="negative"):
        net.set_dropout_state((1, -1))
