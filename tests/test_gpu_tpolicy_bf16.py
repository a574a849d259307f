"""The transformer policy's bf16 gradient pass on the MI355X (csrc/g2048_tpolicy_bf16.hip, csrc/g2048_tpolicy_bf16.h,
include/g2048_tbf16.h; DeviceTransformerPolicy(grad_precision="bf16")).

1  The three products on their own, tight: each entry point of the header's testing section against float64 matmuls of the SAME
   rounded inputs (both sides round identical bits, so no value can land on another bf16 neighbour). The yardstick is torch CPU
   float32 on those rounded inputs, the bound the project's 8 x that, relative to the tensor's largest element; a bf16 output must
   be a bf16 neighbour of some value within that bound of the float64 result. Inputs on bf16 ties and a float32 ulp either side
   pin round-to-nearest-even.
2  The whole pass against the rounded float64 oracle (g2048.tpolicy.loss_grad_reference(ff_bf16=True)): every gradient tensor, the
   loss parts, probs and value within CAP = 0.25 of the case's intrinsic cost (tests/tpolicy_bf16_ref.py has the reasoning;
   tests/test_tpolicy_bf16_host.py asserts every case's conditions on the CPU).
3  Dropout: the masks of ops.tpolicy_dropout_mask, the same bound; null p4 and zeros; a fully dropped hidden unit.
4  The rules: two calls, guard bands, a poisoned workspace, the refusals, the workspace formula.
5  The interface.
Every measured figure is printed; docs/LOG.md R37 has one MI355X run's."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import guard
import tpolicy_bf16_ref as B
import tpolicy_grad_ref as R
from test_gpu_tpolicy_grad import to_dev

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
bits = guard.bits
FF = (32, 96, 160, 2048)
ROWS = (1, 15, 16, 17)
SPLIT_ROWS = ROWS + (511, 512, 513, 1025)


# ---------------------------------------------------------------------------------------------------- 1: the products --
def lib():
    from g2048 import _lib
    return _lib.tbf16_lib(), _lib


def dev(a, bf16=False):
    """A host float array on the device as float32, or as bf16 (exact: the callers round first)."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
    return t.to(torch.bfloat16) if bf16 else t


def ptr(t):
    return None if t is None else t.data_ptr()


def call(fn, *args):
    handle, L = lib()
    rc = getattr(handle, fn)(*args, L.stream_ptr(torch.device(DEV)))
    assert rc == 0, handle.g2048_tbf16_last_error().decode()
    torch.cuda.synchronize()


def host(t):
    return t.float().cpu().numpy().astype(np.float64)


def judge(what, got, want64, want32, is_bf16, floor=0.0):
    """got within 8 x float32's own error of the float64 result, relative to its largest element; a bf16 result within that of a
    value whose bf16 neighbour it is. floor: the least the yardstick counts as (the column sums, below)."""
    top = np.abs(want64).max()
    yard = max(np.abs(want32 - want64).max() / top, floor)
    tol = R.F32_FACTOR * yard * top
    err = np.abs(got - want64)
    slack = B.bf16_spacing(np.abs(want64) + tol) if is_bf16 else 0.0
    worst = (err - slack).max() / top
    print("%s: %.3g of the largest (after the bf16 spacing: %.3g) = %.2f x the CPU-f32 error %.3g" % (
        what, err.max() / top, max(worst, 0.0), max(worst, 0.0) / yard if yard else float("inf"), yard))
    assert np.all(np.isfinite(got)), what
    assert yard > 0 or err.max() == 0, "%s: float32 is exact here and the device is not" % what
    assert np.all(err <= tol + slack), "%s: %.3g of the largest against a bound of %.3g" % (what, worst, R.F32_FACTOR * yard)


def f32_of(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def inputs(rng, shape, tied=False, scale=1.0):
    return B.ties(shape, rng) if tied else (scale * rng.standard_normal(shape)).astype(np.float32)


def linear_once(rng, n, K, M, kind, relu, with_res, tied=False):
    x_bf16, y_bf16 = kind
    x, w = inputs(rng, (n, K), tied), inputs(rng, (M, K), tied, 0.2)
    if x_bf16:
        x = B.rnd64(x).astype(np.float32)
    bias = inputs(rng, (M,))
    res = inputs(rng, (n, M)) if with_res else None
    xr, wr = B.rnd64(x), B.rnd64(w)
    want64 = xr @ wr.T + bias + (res if with_res else 0.0)
    want32 = (f32_of(xr) @ f32_of(wr).T + f32_of(bias) + (f32_of(res) if with_res else 0.0)).numpy().astype(np.float64)
    if relu:
        want64, want32 = np.maximum(want64, 0), np.maximum(want32, 0)
    xd, wd, bd, rd = dev(x, x_bf16), dev(w), dev(bias), dev(res)
    y = torch.full((n + 2, M), float("nan"), dtype=torch.bfloat16 if y_bf16 else torch.float32, device=DEV)
    ws = torch.empty(2 * M * K, dtype=torch.uint8, device=DEV)
    call("g2048_tbf16_test_linear", ptr(xd), int(x_bf16), ptr(wd), ptr(bd), ptr(rd), ptr(y), int(y_bf16), int(relu), n, K, M, ptr(ws), ws.numel())
    assert bool(torch.isnan(y[n:].float()).all()), "rows past n were written"
    judge("linear n=%d K=%d M=%d x%s y%s relu=%d res=%d%s" % (n, K, M, "bf" if x_bf16 else "f", "bf" if y_bf16 else "f", relu, with_res,
                                                              " ties" if tied else ""), host(y[:n]), want64, want32, y_bf16)


def dx_once(rng, n, M, K, kind, with_res, with_mask, tied=False):
    dy_bf16, dx_bf16 = kind
    dy, w = inputs(rng, (n, M), tied), inputs(rng, (M, K), tied, 0.2)
    if dy_bf16:
        dy = B.rnd64(dy).astype(np.float32)
    res = inputs(rng, (n, K)) if with_res else None
    mask = None
    if with_mask:
        mask = B.rnd64(np.maximum(inputs(rng, (n, K)), 0)).astype(np.float32)          # a hidden layer after its ReLU: about half zeros
        if n > 1:
            mask[n // 2] = 0.0                                                           # and one row of zeros
    yr, wr = B.rnd64(dy), B.rnd64(w)
    want64 = yr @ wr + (res if with_res else 0.0)
    want32 = (f32_of(yr) @ f32_of(wr) + (f32_of(res) if with_res else 0.0)).numpy().astype(np.float64)
    if with_mask:
        want64, want32 = np.where(mask > 0, want64, 0.0), np.where(mask > 0, want32, 0.0)
    yd, wd, rd, md = dev(dy, dy_bf16), dev(w), dev(res), dev(mask, True)
    out = torch.full((n + 2, K), float("nan"), dtype=torch.bfloat16 if dx_bf16 else torch.float32, device=DEV)
    ws = torch.empty(2 * M * K, dtype=torch.uint8, device=DEV)
    call("g2048_tbf16_test_dx", ptr(yd), int(dy_bf16), ptr(wd), ptr(rd), ptr(md), ptr(out), int(dx_bf16), n, M, K, ptr(ws), ws.numel())
    assert bool(torch.isnan(out[n:].float()).all()), "rows past n were written"
    got = host(out[:n])
    if with_mask:
        assert np.all(got[mask <= 0] == 0), "a masked element is not zero"
    judge("dx n=%d M=%d K=%d dy%s dx%s res=%d mask=%d%s" % (n, M, K, "bf" if dy_bf16 else "f", "bf" if dx_bf16 else "f", with_res, with_mask,
                                                            " ties" if tied else ""), got, want64, want32, dx_bf16)


def dw_once(rng, n, M, K, kind, tied=False):
    dy_bf16, x_bf16 = kind
    dy, x = inputs(rng, (n, M), tied), inputs(rng, (n, K), tied)
    if dy_bf16:
        dy = B.rnd64(dy).astype(np.float32)
    if x_bf16:
        x = B.rnd64(x).astype(np.float32)
    yr, xr = B.rnd64(dy), B.rnd64(x)
    want64, want32 = yr.T @ xr, (f32_of(yr).T @ f32_of(xr)).numpy().astype(np.float64)
    b64 = dy.astype(np.float64).sum(0)                                   # dY as stored: the float32 values, or the bf16 ones
    b32 = f32_of(dy).sum(0).numpy().astype(np.float64)
    chunks = (n + 511) // 512
    yd, xd = dev(dy, dy_bf16), dev(x, x_bf16)
    dw = torch.full((M + 1, K), float("nan"), device=DEV)
    db = torch.full((M + 4,), float("nan"), device=DEV)
    ws = torch.full((chunks * (M * K + M),), float("nan"), device=DEV)
    call("g2048_tbf16_test_dw", ptr(yd), int(dy_bf16), ptr(xd), int(x_bf16), ptr(dw), ptr(db), n, M, K, ptr(ws), 4 * ws.numel())
    assert bool(torch.isnan(dw[M:]).all()) and bool(torch.isnan(db[M:]).all()), "elements past the gradient were written"
    what = "dw n=%d M=%d K=%d dy%s x%s%s" % (n, M, K, "bf" if dy_bf16 else "f", "bf" if x_bf16 else "f", " ties" if tied else "")
    judge(what, host(dw[:M]), want64, want32, False)
    # the column sums add bf16 values, or few float32 ones: torch's float32 sum is then often exact, and its error no measure. The
    # yardstick counts as one float32 ulp of the largest sum at least; any order of float32 additions is off by that much.
    judge(what + " db", host(db[:M]), b64, b32, False, floor=float(np.finfo(np.float32).eps))


@pytest.mark.parametrize("ff", FF)
def test_linear_product_against_float64_on_the_same_rounded_inputs(ff):
    rng = np.random.default_rng(100 + ff)
    for n in ROWS:
        # the pass's two: linear1 (f32 -> bf16, ReLU) and linear2 (bf16 -> f32, residual); and each switch the other way
        linear_once(rng, n, 64, ff, (0, 1), True, False)
        linear_once(rng, n, ff, 64, (1, 0), False, True)
        linear_once(rng, n, 64, ff, (0, 0), False, True)
        linear_once(rng, n, ff, 64, (0, 1), True, True)
    linear_once(rng, 17, 64, ff, (0, 1), True, False, tied=True)
    linear_once(rng, 17, ff, 64, (0, 0), False, False, tied=True)


@pytest.mark.parametrize("ff", FF)
def test_data_gradient_against_float64_on_the_same_rounded_inputs(ff):
    rng = np.random.default_rng(200 + ff)
    for n in ROWS:
        # the pass's two: through linear2 (f32 dY, M = 64 -> bf16 dh [n][ff], masked) and through linear1 (bf16 dh -> f32, residual)
        dx_once(rng, n, 64, ff, (0, 1), False, True)
        dx_once(rng, n, ff, 64, (1, 0), True, False)
        dx_once(rng, n, 64, ff, (0, 0), True, True)
        dx_once(rng, n, ff, 64, (0, 0), False, False)
    dx_once(rng, 17, 64, ff, (0, 0), False, False, tied=True)
    dx_once(rng, 17, ff, 64, (0, 0), False, False, tied=True)


@pytest.mark.parametrize("ff", FF)
def test_weight_gradient_against_float64_on_the_same_rounded_inputs(ff):
    rng = np.random.default_rng(300 + ff)
    for n in SPLIT_ROWS:
        dw_once(rng, n, 64, ff, (0, 1))          # dW2: f32 dY, the bf16 hidden layer
        dw_once(rng, n, ff, 64, (1, 0))          # dW1: the bf16 dh, f32 x1
    for n in (17, 513):
        dw_once(rng, n, 64, ff, (0, 0))
        dw_once(rng, n, ff, 64, (0, 0), tied=True)


# ------------------------------------------------------------------------------------------------- 2: the whole pass --
def bf16_net(c, precision="f32"):
    from g2048 import DeviceTransformerPolicy
    p4 = 0.0 if c.p4 is None else c.p4
    net = DeviceTransformerPolicy(copy.deepcopy(c.model32).to(DEV).eval(), precision, dropout=p4, dropout_seed=c.seed, grad_precision="bf16")
    net.set_dropout_state((c.seed, c.index))
    return net


def outputs(net, result):
    losses, probs, value = result
    grads, eps = R.split(net.parsed, net.grad.cpu().numpy())
    assert np.all(eps == 0) and len(eps) == 2 * net.n_layers, "a LayerNorm-eps slot of grad is not 0"
    f64 = lambda t: t.cpu().numpy().astype(np.float64)       # noqa: E731
    return dict(losses=f64(losses), probs=f64(probs), value=f64(value), grads=grads)


def check(got, c, what):
    """Every gradient tensor, the loss parts, probs and value within the cap of the rounded float64 oracle."""
    r = R.ratios(got["grads"], c.want["grads"])
    worst = int(np.argmax(r))
    rest = B.others(got, c.want)
    print("%s: gradients %.3g of max|g| (tensor %d) = %.4f of the intrinsic cost %.4g (cap %.2f; CPU flip noise %.3g = %.4f); losses %.3g, "
          "probs %.3g, value %.3g" % (what, r[worst], worst, r[worst] / c.intrinsic, c.intrinsic, B.CAP, c.flip, c.flip / c.intrinsic,
                                      rest["losses"], rest["probs"], rest["value"]))
    assert all(np.all(np.isfinite(g)) for g in got["grads"]) and np.all(np.isfinite(got["losses"])), what
    assert all(np.abs(g).max() > 0 for g in got["grads"]), "%s: a gradient tensor is zero" % what
    assert r.max() <= c.cap, "%s: tensor %d is %.3f of the intrinsic cost" % (what, worst, r[worst] / c.intrinsic)
    for k, v in rest.items():
        assert v <= c.cap, "%s: %s is %.3f of the intrinsic cost" % (what, k, v / c.intrinsic)


@pytest.mark.parametrize("shape", B.SHAPES, ids=["n%d-ff%d-L%d" % s for s in B.SHAPES])
def test_the_pass_against_the_rounded_float64_oracle(shape):
    """Measured on an MI355X (docs/LOG.md R37.2), worst gradient tensor as a fraction of the case's intrinsic cost, cap 0.25:
    (1, 32, 1) 0.0001, (2, 32, 2) 0.0000, (15, 64, 2) 0.0059, (16, 64, 2) 0.0031, (17, 96, 2) 0.0009, (33, 160, 1) 0.0003,
    (64, 2048, 2) 0.0010, (31 | 32 | 33, 32, 2) 0.0004 | 0.0020 | 0.0005, (1024, 32, 2) 0.0055; float32 torch's flip noise on the same
    cases is 0.0000 - 0.0060. Losses, probs and value at most 3.9e-4 of their largest."""
    c = B.case(shape + (None,))
    c.conditions()
    net = bf16_net(c)
    got = outputs(net, net.loss_and_grad(*to_dev(*c.args)))
    check(got, c, B.case_id(c.case))
    assert got["probs"].shape == (c.n, 4) and got["value"].shape == (c.n, 1)
    # the unrounded function is NOT what the pass computes: it is about the intrinsic cost away from it
    away = float(R.ratios(got["grads"], c.unrounded["grads"]).max())
    assert away > 2 * c.cap, "the pass is within %.3g of the unrounded function" % away


# ----------------------------------------------------------------------------------------------------------- 3: dropout --
@pytest.mark.parametrize("case", B.DROPOUT_CASES, ids=B.case_id)
def test_the_pass_with_dropout_against_the_rounded_oracle_under_the_masks(case):
    """Measured on an MI355X, as a fraction of the intrinsic cost (cap 0.25): p = 0.1 on all four sites 0.0107 at (17, 96, 2) and
    0.0026 at (33, 160, 1); on site 2 alone 0.0035 and 0.0005."""
    c = B.case(case)
    c.conditions()
    net = bf16_net(c)
    got = outputs(net, net.loss_and_grad(*to_dev(*c.args)))
    check(got, c, B.case_id(case))
    assert net.dropout_state() == (c.seed, c.index + 1)


def raw_call(net, args, p4, ws, seed=0, index=0, n_layers=None, dim_ff=None, n=None, ws_bytes=None):
    """g2048_tpolicy_loss_grad_bf16 itself: (status, message, grad, losses, probs, value)."""
    handle, L = lib()
    boards, actions, old, adv, ret = args
    rows = boards.shape[0] if n is None else n
    grad = torch.full_like(net.grad, 7.0)
    losses, probs, value = torch.full((4,), 7.0, device=DEV), torch.full((max(rows, 1), 4), 7.0, device=DEV), torch.full((max(rows, 1), 1), 7.0, device=DEV)
    rc = handle.g2048_tpolicy_loss_grad_bf16(boards.data_ptr(), net.plain.data_ptr(), actions.data_ptr(), old.data_ptr(), adv.data_ptr(),
                                             ret.data_ptr(), rows, net.dim_ff if dim_ff is None else dim_ff,
                                             net.n_layers if n_layers is None else n_layers, None if p4 is None else (C.c_double * 4)(*p4), seed,
                                             index, 0.3, 0.4, 0.05, grad.data_ptr(), losses.data_ptr(), probs.data_ptr(), value.data_ptr(),
                                             ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, L.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, handle.g2048_tbf16_last_error().decode(), grad, losses, probs, value


def test_null_p4_and_zeros_give_the_same_bits():
    from g2048 import ops
    c = B.case((17, 96, 2, None))
    net = bf16_net(c)
    args = to_dev(*c.args)
    ws = torch.empty(ops.tpolicy_bf16_workspace_bytes(c.n, c.dim_ff, c.layers), dtype=torch.uint8, device=DEV)
    null = raw_call(net, args, None, ws)
    zeros = raw_call(net, args, (0.0, 0.0, 0.0, 0.0), ws, seed=5, index=9)
    assert null[0] == zeros[0] == 0, (null[1], zeros[1])
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(null[2:], zeros[2:]))
    through = net.loss_and_grad(*args)
    assert torch.equal(bits(net.grad), bits(null[2])) and torch.equal(bits(through[0]), bits(null[3]))
    rc, said = raw_call(net, args, (0.0, 1.0, 0.0, 0.0), ws)[:2]
    assert rc == -1 and "p[1] must be finite, 0 <= p < 1" in said


def test_a_hidden_unit_dropped_on_every_token_has_a_zero_column_in_linear2s_weight_gradient():
    """One board, 16 tokens, p = 0.9 on site 2 alone: dW2[:, j] is the sum over the tokens of dY[t] h[t][j] m[t][j], so a unit whose
    keep bits (ops.tpolicy_dropout_mask) are 0 on all sixteen tokens has an exactly zero column, and so has its row of dW1 and its
    element of db1; of the units that are kept somewhere, some column is not zero."""
    from g2048 import DeviceTransformerPolicy, ops
    c = B.case((1, 32, 1, None))
    ff, p, seed, index = 96, 0.9, 11, 3
    net = DeviceTransformerPolicy(R.stock_module(ff, 1).to(DEV).eval(), dropout=(0.0, 0.0, p, 0.0), dropout_seed=seed, grad_precision="bf16")
    net.set_dropout_state((seed, index))
    net.loss_and_grad(*to_dev(*c.args))
    keep = ops.tpolicy_dropout_mask(1, 0, 2, p, dim_ff=ff, seed=seed, call_index=index).cpu().numpy().astype(bool)
    assert keep.shape == (16, ff)
    gone = ~keep.any(0)
    assert 3 <= gone.sum() <= ff - 3, "the construction needs units of both kinds (%d dropped everywhere)" % gone.sum()
    lay, at, o = net.parsed.layers[0], {}, 0
    for t in net.parsed.plain_tensors():
        if isinstance(t, torch.Tensor):
            at[id(t)] = o
            o += t.numel()
        else:
            o += 1
    g = net.grad.cpu().numpy()
    part = lambda t: g[at[id(t)]:at[id(t)] + t.numel()].reshape(tuple(t.shape))       # noqa: E731
    dw2, dw1, db1 = part(lay.linear2.weight), part(lay.linear1.weight), part(lay.linear1.bias)
    assert np.all(dw2[:, gone] == 0) and np.all(dw1[gone] == 0) and np.all(db1[gone] == 0)
    assert np.any(dw2[:, ~gone] != 0) and np.any(dw1[~gone] != 0)


# ------------------------------------------------------------------------------------------------------------- 4: rules --
def test_two_calls_give_the_same_bits():
    for case in ((33, 160, 1, None), (33, 160, 1, B.P4)):
        c = B.case(case)
        net = bf16_net(c)
        args = to_dev(*c.args)
        first = [t.clone() for t in net.loss_and_grad(*args)] + [net.grad.clone()]
        net.set_dropout_state((c.seed, c.index))
        again = list(net.loss_and_grad(*args)) + [net.grad]
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(first, again)), "two calls differ"


@pytest.mark.parametrize("case", ((17, 96, 2, B.P4), (1024, 32, 2, None)), ids=B.case_id)
def test_guard_bands_round_everything_the_entry_point_writes(case):
    """The two-run protocol of tests/guard.py round grad, the four outputs and the workspace, poison in the inputs' bands, both runs
    bit-equal; then a third run on a workspace of NaNs (0xFF bytes are a NaN in float32 and in bf16) with the same bits: no
    workspace element is read before the call wrote it."""
    from g2048 import ops
    c = B.case(case)
    net = bf16_net(c)
    n, floats = c.n, net.plain.numel()
    nb = ops.tpolicy_bf16_workspace_bytes(n, net.dim_ff, net.n_layers)
    kw = dict(dropout=c.p4, seed=c.seed, call_index=c.index, grad_precision="bf16")

    def run(s):
        boards = s.inp("boards", c.boards, align=16)
        plain = s.inp("plain", net.plain, align=16)
        actions = s.inp("actions", c.actions)
        old, adv, ret = s.inp("old_log_probs", c.old), s.inp("advantages", c.adv), s.inp("returns", c.ret)
        grad = s.out("grad", floats, (), torch.float32, align=16)
        losses = s.out("losses", 4, (), torch.float32)
        probs = s.out("probs", n, (4,), torch.float32, align=16)
        value = s.out("value", n, (1,), torch.float32)
        ws = s.out("workspace", nb, (), torch.uint8, align=16)
        ops.tpolicy_loss_grad(boards, plain, actions, old, adv, ret, net.dim_ff, net.n_layers, grad=grad, losses=losses, probs=probs,
                              value=value, workspace=ws, **kw)
        return dict(grad=grad, losses=losses, probs=probs, value=value)

    out = guard.twice(DEV, run)
    grads, eps = R.split(net.parsed, out["grad"].numpy())
    assert np.all(eps == 0)
    f64 = lambda t: t.numpy().astype(np.float64)       # noqa: E731
    check(dict(losses=f64(out["losses"]), probs=f64(out["probs"]), value=f64(out["value"]), grads=grads), c, "guarded, " + B.case_id(case))
    poisoned = torch.full((nb,), 0xFF, dtype=torch.uint8, device=DEV)
    losses, probs, value, grad = ops.tpolicy_loss_grad(to_dev(c.boards)[0], net.plain, *to_dev(c.actions, c.old, c.adv, c.ret), net.dim_ff,
                                                       net.n_layers, workspace=poisoned, **kw)
    for name, t in (("grad", grad), ("losses", losses), ("probs", probs), ("value", value)):
        assert torch.equal(bits(t), bits(out[name])), "%s differs on a workspace of NaNs" % name


def test_refusals_name_the_limit_and_launch_nothing():
    from g2048 import ops
    c = B.case((17, 96, 2, None))
    net = bf16_net(c)
    args = to_dev(*c.args)
    nb = ops.tpolicy_bf16_workspace_bytes(c.n, c.dim_ff, c.layers)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    big = tuple(torch.zeros((1025,) + tuple(t.shape[1:]), dtype=t.dtype, device=DEV) for t in args)
    for what, kw, a, message in (("n = 1025", dict(), big, "G2048_TLEARN_BATCH_MAX = 1024"),
                                 ("dim_ff 48", dict(dim_ff=48), args, "dim_ff must be a multiple of 32"),
                                 ("a workspace one byte short", dict(ws_bytes=nb - 1), args, "g2048_tpolicy_bf16_workspace(n, dim_ff, n_layers) is %d" % nb)):
        rc, said, grad, losses, probs, value = raw_call(net, a, None, ws, **kw)
        assert rc == -1 and said.startswith("g2048_tpolicy_loss_grad_bf16: ") and message in said, (what, rc, said)
        assert all(bool((t == 7.0).all()) for t in (grad, losses, probs, value)), "%s: a refused call wrote" % what
    # n = 0: the library's size query refuses it, and the host layer says so with the limits; a call with no rows launches nothing
    handle, _ = lib()
    assert handle.g2048_tpolicy_bf16_workspace(0, 96, 2) == 0 == handle.g2048_tpolicy_bf16_workspace(1025, 96, 2)
    assert handle.g2048_tpolicy_bf16_workspace(17, 48, 2) == 0
    for n in (0, 1025):
        with pytest.raises(ValueError, match="1 .. 1024"):
            ops.tpolicy_bf16_workspace_bytes(n, 96, 2)
    before = net.grad.clone()
    with pytest.raises(ValueError, match="1024"):
        net.loss_and_grad(*big)
    empty = net.loss_and_grad(*(t[:0] for t in args))
    assert empty[1].shape == (0, 4) and torch.equal(bits(net.grad), bits(before)), "N = 0 launches nothing"


@pytest.mark.parametrize("shape", ((1, 32, 1), (17, 96, 2), (33, 160, 1), (64, 2048, 2), (1024, 128, 2), (1024, 2048, 2)))
def test_the_workspace_is_the_headers_formula(shape):
    from g2048 import ops
    n, ff, layers = shape
    got = ops.tpolicy_bf16_workspace_bytes(n, ff, layers)
    assert got == ops.tpolicy_train_workspace_bytes(n, ff, layers) - 2 * (4 - 2) * 16 * n * ff + layers * 4 * 64 * ff * 2 and got % 16 == 0
    if ff >= 128:
        assert got < ops.tpolicy_grad_workspace_bytes(n, ff, layers)


# ------------------------------------------------------------------------------------------------------- 5: interface --
def update_inputs():
    import tpolicy_dropout_ref as D
    base, inputs = D.update_inputs()
    return base, to_dev(*inputs)


def state(net):
    return [net.plain, net.grad, net.exp_avg, net.exp_avg_sq]


def test_f32_is_the_call_without_the_argument_bit_for_bit():
    from g2048 import DeviceTransformerPolicy
    base, inputs = update_inputs()
    for dropout in (0.0, 0.1):
        nets = [DeviceTransformerPolicy(copy.deepcopy(base.model32).to(DEV).eval(), dropout=dropout, dropout_seed=3, **kw)
                for kw in (dict(), dict(grad_precision="f32"))]
        assert [n.grad_precision for n in nets] == ["f32", "f32"]
        results = []
        for net in nets:
            out = [t.clone() for t in net.loss_and_grad(*to_dev(*base.args))] + [net.grad.clone()]
            losses, norms = net.update(*inputs, epochs=2)
            results.append(out + [losses.clone(), norms.clone()] + [t.clone() for t in state(net)])
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(*results)), "grad_precision='f32' moved a bit (dropout %g)" % dropout


@pytest.mark.parametrize("dropout", (0.0, 0.1))
def test_update_is_the_chain_of_its_parts_in_bf16(dropout):
    from g2048 import DeviceTransformerPolicy
    base, inputs = update_inputs()
    boards, actions, old, rewards, nxt, dones = inputs
    make = lambda precision="f32": DeviceTransformerPolicy(copy.deepcopy(base.model32).to(DEV).eval(), precision, dropout=dropout,       # noqa: E731
                                                            dropout_seed=3, grad_precision="bf16")
    net, twin, blob = make(), make(), make("bf16")
    ret, adv = (t.clone() for t in twin.advantages(boards, nxt, rewards, dones, 0.995))
    kept = []
    for e in range(2):
        losses, _, _ = twin.loss_and_grad(boards, actions, old, adv, ret)
        norm = twin.adam_step(losses)
        kept.append((losses.clone(), norm.clone()))
    for other in (net, blob):
        losses, norms = other.update(*inputs, epochs=2)
        torch.cuda.synchronize()
        for name, a, b in zip(("plain", "grad", "exp_avg", "exp_avg_sq"), state(other), state(twin)):
            assert torch.equal(bits(a), bits(b)), "update() and its parts leave other bits in %s (acting blob %s)" % (name, other.precision)
        assert all(torch.equal(bits(losses[e]), bits(k[0])) and torch.equal(bits(norms[e]), bits(k[1])) for e, k in enumerate(kept))
        assert other.dropout_index == twin.dropout_index == (4 if dropout else 2) and other.opt_counters.tolist() == [2, 0, 0]
    # and the f32 pass's update is another function: the two modes are not the same call
    plain = DeviceTransformerPolicy(copy.deepcopy(base.model32).to(DEV).eval(), dropout=dropout, dropout_seed=3)
    plain.update(*inputs, epochs=2)
    assert not torch.equal(bits(plain.grad), bits(net.grad))


def test_attached_gradients_see_the_bf16_pass_and_a_bad_value_is_refused():
    from g2048 import DeviceTransformerPolicy, ops
    c = B.case((17, 96, 2, None))
    net = bf16_net(c)
    net.attach_grads()
    net.loss_and_grad(*to_dev(*c.args))
    flat = torch.cat([p.grad.reshape(-1) for p in net.model.parameters()]).cpu().numpy().astype(np.float64)
    got = np.concatenate(R.split(net.parsed, net.grad.cpu().numpy())[0])
    assert all(p.grad.data_ptr() >= net.grad.data_ptr() for p in net.model.parameters()) and np.abs(flat).max() > 0
    assert np.array_equal(np.sort(flat), np.sort(got)), "the attached .grad views do not hold the pass's gradients"
    assert float(R.ratios(R.split(net.parsed, net.grad.cpu().numpy())[0], c.want["grads"]).max()) <= c.cap
    for bad in ("f16", "fp32", None, 1):
        with pytest.raises(ValueError, match="'f32' or 'bf16'"):
            DeviceTransformerPolicy(copy.deepcopy(c.model32).to(DEV).eval(), grad_precision=bad)
        with pytest.raises(ValueError, match="'f32' or 'bf16'"):
            ops.tpolicy_loss_grad(*to_dev(*c.args)[:1], net.plain, *to_dev(*c.args)[1:], net.dim_ff, net.n_layers, grad_precision=bad)
