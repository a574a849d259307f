"""The bf16 gradient pass of the transformer policy, what the CPU can say (include/g2048_tbf16.h, csrc/libg2048_tbf16_hip.so, the
second row of g2048._build.EXTRA_ROWS): the torch restatement g2048.tpolicy.loss_grad_reference(ff_bf16=...), the conditions of
every case tests/test_gpu_tpolicy_bf16.py runs (tests/tpolicy_bf16_ref.py), and the library's boundary as
tests/test_tpolicy_collect_abi_host.py checks it for its row."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import tpolicy_bf16_ref as B
import tpolicy_grad_ref as R
from conftest import PKG, REPO
from test_abi_and_host import declared_symbols
from test_libraries_abi_host import HOST, SIDE, SIZE, bound, exported

KEY, HEADER, SOURCES = "TBF16_", "g2048_tbf16.h", ["g2048_tpolicy_bf16.hip"]
PRODUCT, VARIABLE = "libg2048_tbf16_hip.so", "G2048_TBF16_LIB"
GPU = "tests/test_gpu_tpolicy_bf16.py"
GUARDED_BY = {
    "g2048_tbf16_last_error": (None, HOST),
    "g2048_tbf16_abi_version": (None, HOST),
    "g2048_tpolicy_bf16_workspace": (None, SIZE),
    "g2048_tpolicy_loss_grad_bf16": GPU + "::test_guard_bands_round_everything_the_entry_point_writes",
    "g2048_tbf16_test_linear": GPU + "::test_linear_product_against_float64_on_the_same_rounded_inputs",
    "g2048_tbf16_test_dx": GPU + "::test_data_gradient_against_float64_on_the_same_rounded_inputs",
    "g2048_tbf16_test_dw": GPU + "::test_weight_gradient_against_float64_on_the_same_rounded_inputs",
}
# the intrinsic cost of the host cases, float64 against float64 (docs/LOG.md R37)
INTRINSIC = {(1, 32, 1, None): 0.00455, (17, 96, 2, None): 0.1456, (33, 160, 1, B.P4): 0.0273}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------- the restatement --
def reference_bits(c, **kw):
    from g2048 import tpolicy
    boards, actions, old, adv, ret = (torch.from_numpy(np.ascontiguousarray(x)) for x in c.args)
    return tpolicy.loss_grad_reference(B.parsed_of(c.model32), boards, actions, old, adv, ret, multipliers=c.multipliers, **kw)


@pytest.mark.parametrize("case", B.HOST_CASES, ids=B.case_id)
def test_without_the_switch_the_reference_is_what_it_was(case):
    c = B.case(case)
    for dtype in (torch.float64, torch.float32):
        was, now = reference_bits(c, dtype=dtype), reference_bits(c, dtype=dtype, ff_bf16=False)
        assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(was, now))
    rounded = reference_bits(c, ff_bf16=True)
    assert not torch.equal(rounded[3], was[3]) and rounded[3].dtype == torch.float64


@pytest.mark.parametrize("case", B.HOST_CASES, ids=B.case_id)
def test_the_intrinsic_cost_is_per_cents_not_rounding(case):
    """The rounded float64 function against the unrounded one: 0.45 % .. 15 % of the worst gradient tensor's largest element, pinned per
    case to a tenth; the probabilities move by 1e-4 .. 1e-2."""
    c = B.case(case)
    print("%s: intrinsic cost %.4g, probs %.3g, flip noise %.3g" % (B.case_id(case), c.intrinsic, R.rel(c.want["probs"], c.unrounded["probs"]), c.flip))
    assert 0.9 * INTRINSIC[case] <= c.intrinsic <= 1.1 * INTRINSIC[case]
    assert 0.004 <= c.intrinsic <= 0.16
    assert 1e-4 <= R.rel(c.want["probs"], c.unrounded["probs"]) <= 1e-2


def test_exact_operands_make_the_rounded_feed_forward_the_plain_one():
    """The feed-forward pair of one layer with every operand exactly representable in bf16 and every product exact (small integers:
    |x| <= 2, weights in {-1, 0, 1}, so the hidden layer stays below 2^8 and its gradient below 2^7): the rounded pair and the plain
    one give the same float64 output and the same gradients, to the bit. A rounding anywhere else than on an operand would show."""
    from g2048 import tpolicy as T
    gen = torch.Generator().manual_seed(5)
    ints = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=gen).double()       # noqa: E731
    x, w1, b1, w2, b2 = ints(-2, 2, 3, 16, 64), ints(-1, 1, 96, 64), ints(-3, 3, 96), ints(-1, 1, 64, 96), ints(-3, 3, 64)
    weight = ints(-1, 1, 3, 16, 64)
    results = []
    for rounded in (True, False):
        leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
        xl, w1l, b1l, w2l, b2l = leaves
        if rounded:
            y = T._feed_forward_bf16(xl, w1l, b1l, w2l, b2l, lambda t: t)
        else:
            y = torch.relu(xl @ w1l.T + b1l) @ w2l.T + b2l
        results.append([y.detach()] + list(torch.autograd.grad((y * weight).sum(), leaves)))
    assert float(results[0][0].abs().max()) > 0 and all(float(g.abs().max()) > 0 for g in results[0])
    assert all(torch.equal(a, b) for a, b in zip(*results))
    # and rnd itself: to nearest, ties to even, through float32
    t = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -30, 1 + 2.0 ** -8 - 2.0 ** -30, -(1 + 2.0 ** -8)], dtype=torch.float64)
    assert T.rnd(t).tolist() == [1.0, 1 + 2.0 ** -6, 1.0, 1.0, -1.0], "float64 -> float32 first (the 2^-30 is gone), then ties to even"
    assert T.rnd(t).dtype == torch.float64 and torch.equal(T.rnd(T.rnd(t)), T.rnd(t))


@pytest.mark.parametrize("case", ((17, 96, 2, None), (33, 160, 1, B.P4)), ids=B.case_id)
def test_with_a_rounding_that_rounds_nothing_the_switch_changes_nothing(case, monkeypatch):
    """The wiring round the two custom functions (loss_grad_reference -> post_norm_tail's feed_forward branch: the site-2 and
    site-3 multipliers, the biases, the residual, the whole network either side): with rnd replaced by the identity, ff_bf16=True is
    the unrounded function to float64 rounding. LayerNorm outputs are not representable in bf16, so no choice of weights makes the
    whole network's products exact; the test above does that for the pair alone, this one holds everything round the pair."""
    from g2048 import tpolicy
    c = B.case(case)
    monkeypatch.setattr(tpolicy, "rnd", lambda t: t)
    same = B.reference(c.model32, c.args, torch.float64, True, c.multipliers)
    assert B.worst(same, c.unrounded) <= 1e-12 and max(B.others(same, c.unrounded).values()) <= 1e-12
    assert c.intrinsic > 1e-3, "and with the real rounding it is not"


@pytest.mark.parametrize("case", B.ALL_CASES, ids=B.case_id)
def test_every_gpu_case_meets_its_conditions(case):
    """The ReLU margin on the ROUNDED function, Case.conditions' rules, and 8 x flip noise under the cap: asserted, not assumed."""
    c = B.case(case)
    c.conditions()
    rest = B.others(c.rounded32, c.want)
    print("%s: board seed %d, dropout seed %d: intrinsic cost %.4g, flip noise %.3g (8 x = %.4f of the intrinsic cost, cap %.2f), ReLU margin "
          "%.3g, clipped share %.2f; losses %.3g probs %.3g value %.3g" % (B.case_id(case), c.board_seed, c.seed, c.intrinsic, c.flip,
                                                                             R.F32_FACTOR * c.flip / c.intrinsic, B.CAP, c.relu_margin,
                                                                             c.clipped_share, rest["losses"], rest["probs"], rest["value"]))
    assert B.CAP <= 0.5 and R.F32_FACTOR * c.flip <= c.cap


def test_the_seed_table_is_what_the_search_finds():
    for case in ((15, 64, 2, None), (16, 64, 2, None)):
        assert B.find_seeds(case)[:2] == B.SEEDS[case][:2]
    assert B.Case((16, 64, 2, None), board_seed=16).failed(), "board seed 16 is the case whose float32 run changes a head ReLU's sign"


# ------------------------------------------------------------------------------------------------------- the boundary --
def test_library_exports_its_header_and_its_binding_table(built):
    path, signatures, version, loaded = bound(built, KEY)
    names = declared_symbols(HEADER)
    assert exported(path) == names, (exported(path), names)
    assert set(names) == set(signatures) == set(GUARDED_BY) and len(names) == 7
    hdr = open(os.path.join(REPO, "include", HEADER)).read()
    in_header = int(re.search(r"#define G2048_TBF16_ABI_VERSION (\d+)", hdr).group(1))
    assert in_header == 1 == version == built.TBF16_ABI_VERSION == loaded.g2048_tbf16_abi_version()
    assert os.path.basename(path) == PRODUCT and os.path.dirname(path) == os.path.dirname(built.library_path())


def test_the_library_shares_no_entry_point_with_another(built):
    from g2048 import _build
    others = set()
    for key in _build.ALL_ROWS:
        if key != KEY:
            table = exported(_build.path_of(key))
            assert table, key
            others |= set(table)
    assert set(exported(built.library_path())) == set(built.SIGNATURES), "the main library's export table moved"
    for name in sorted(SIDE):
        assert set(exported(_build.path_of(SIDE[name]["key"]))) == set(getattr(built, SIDE[name]["key"] + "SIGNATURES"))
    assert not set(built.TBF16_SIGNATURES) & others
    assert set(built.EXTRA_ROWS) == set(_build.EXTRA_ROWS) and KEY in _build.EXTRA_ROWS and KEY not in _build.ROWS
    assert type(built.EXTRA_ROWS[KEY]) is built.Library and built.EXTRA_ROWS[KEY].key == KEY and built.EXTRA_ROWS[KEY].stem == "g2048_tbf16"


def test_the_build_counts_the_library(built):
    from g2048 import _build
    real = _build.TBF16_LIB
    assert os.path.basename(real) == PRODUCT and _build.TBF16_SOURCES == SOURCES
    assert _build.EXTRA_ROWS[KEY] == (PRODUCT, VARIABLE, SOURCES, [HEADER])
    elsewhere = sum((r[2] for k, r in _build.ALL_ROWS.items() if k != KEY), [])
    assert not set(SOURCES) & set(elsewhere)
    assert any(h.endswith(HEADER) for h in _build.PUBLIC_HEADERS) and _build.path_of(KEY) == real
    assert not _build.needs_build()
    try:
        _build.TBF16_LIB = os.path.join(os.path.dirname(real), "absent_tbf16.so")
        assert _build.needs_build(), "needs_build() does not look at the bf16 learner library"
    finally:
        _build.TBF16_LIB = real
    assert not _build.needs_build()


def test_the_loader_is_loud_and_takes_only_the_product_name(built, tmp_path):
    path = built.tbf16_library_path()
    code = ("import os, sys; sys.path.insert(0, %r); from g2048 import _build, _lib\n"
            "if os.environ.get('ROW_POINTS_AT'): _build.TBF16_LIB = os.environ['ROW_POINTS_AT']\n"
            "try:\n    print('LOADED', _lib.tbf16_lib().g2048_tbf16_abi_version())\n"
            "except RuntimeError as e:\n    print('REFUSED', e)\n" % PKG)
    clean = {k: v for k, v in os.environ.items() if k != VARIABLE}
    run = lambda **env: subprocess.run([sys.executable, "-c", code], env=dict(clean, **env), capture_output=True, text=True)  # noqa: E731
    out = run(**{VARIABLE: str(tmp_path / "absent.so")})
    assert "REFUSED" in out.stdout and "is missing" in out.stdout and "no CPU fallback" in out.stdout, out
    assert "no bf16 gradient pass of the transformer policy without it" in out.stdout, out
    copy = shutil.copy(path, str(tmp_path / "libab.so"))
    out = run(ROW_POINTS_AT=copy)
    assert "REFUSED g2048: refusing to load %s: only csrc/%s is the " % (copy, PRODUCT) in out.stdout and "bf16 learner library" in out.stdout, out
    assert "LOADED" not in out.stdout
    out = run(**{VARIABLE: copy})
    assert "LOADED 1" in out.stdout and "loading the A/B build %s (%s is set)" % (copy, VARIABLE) in out.stderr, out


def test_every_entry_point_has_its_bounds_test_or_a_reason():
    for entry, where in GUARDED_BY.items():
        if isinstance(where, tuple):
            assert where[0] is None and len(where[1].strip()) > 10, entry
            continue
        path, _, test = where.partition("::")
        source = open(os.path.join(REPO, path)).read()
        assert re.search(r"^def %s\(" % re.escape(test), source, re.M), "%s: %s has no test %s" % (entry, path, test)
        assert "pytest.mark.gpu" in source


def test_arguments_are_checked_without_a_device(built):
    """Every check comes before any device call, so host memory serves; a refused call writes nothing."""
    lib = built.tbf16_lib()
    block = (C.c_uint8 * (64 * 12 + 16))()
    base = (C.addressof(block) + 15) & ~15
    at = [base + 64 * i for i in range(11)]
    p4 = (C.c_double * 4)(0.1, 0.1, 0.1, 0.1)

    def call(n=8, dim_ff=32, layers=1, p=p4, ws_bytes=1 << 40, clip=0.3, **ptrs):
        a = dict(boards=at[0], plain=at[1], actions=at[2], old=at[3], adv=at[4], ret=at[5], grad=at[6], losses=at[7], probs=at[8], value=at[9],
                 ws=at[10])
        a.update(ptrs)
        rc = lib.g2048_tpolicy_loss_grad_bf16(a["boards"], a["plain"], a["actions"], a["old"], a["adv"], a["ret"], n, dim_ff, layers, p, 1, 2, clip, 0.4,
                                              0.05, a["grad"], a["losses"], a["probs"], a["value"], a["ws"], ws_bytes, None)
        return rc, lib.g2048_tbf16_last_error().decode()

    for what, kw, message in (("a null grad", dict(grad=None), "null pointer"), ("a misaligned plain", dict(plain=at[1] + 4), "misaligned pointer"),
                              ("n past the limit", dict(n=1025), "G2048_TLEARN_BATCH_MAX = 1024"), ("dim_ff 48", dict(dim_ff=48), "multiple of 32"),
                              ("no layer", dict(layers=0), "n_layers 1 .. 64"), ("a negative clip", dict(clip=-1.0), "finite and not negative"),
                              ("no workspace to speak of", dict(ws_bytes=64), "g2048_tpolicy_bf16_workspace(n, dim_ff, n_layers) is"),
                              ("p = 1", dict(p=(C.c_double * 4)(0.0, 0.0, 1.0, 0.0)), "p[2] must be finite, 0 <= p < 1"),
                              ("p a NaN", dict(p=(C.c_double * 4)(float("nan"), 0.0, 0.0, 0.0)), "p[0] must be finite")):
        rc, said = call(**kw)
        assert rc == -1 and said.startswith("g2048_tpolicy_loss_grad_bf16: ") and message in said, (what, rc, said)
    assert call(n=0, grad=None, dim_ff=7)[0] == 0, "n == 0 returns OK before anything is looked at"
    assert bytes(block) == bytes(len(block)), "a refused call wrote to the arrays it was given"
    assert lib.g2048_tpolicy_bf16_workspace(0, 32, 1) == lib.g2048_tpolicy_bf16_workspace(1025, 32, 1) == lib.g2048_tpolicy_bf16_workspace(8, 48, 1) == 0
    # the header's formula, on the host: the training library's bytes, h and dh at half, plus every layer's packed weights
    train = built.ttrain_lib().g2048_tpolicy_train_workspace
    for n, ff, layers in ((1, 32, 1), (17, 96, 2), (1024, 2048, 2)):
        assert lib.g2048_tpolicy_bf16_workspace(n, ff, layers) == train(n, ff, layers) - 2 * 2 * 16 * n * ff + layers * 4 * 64 * ff * 2
    # the products' own checks
    for fn, args in (("g2048_tbf16_test_linear", (at[0], 0, at[1], None, None, at[2], 0, 0, 4, 48, 64, at[3], 1 << 30)),
                     ("g2048_tbf16_test_linear", (at[0], 1, at[1], None, None, at[2], 1, 0, 4, 64, 64, at[3], 1 << 30)),
                     ("g2048_tbf16_test_dx", (at[0], 0, at[1], None, None, at[2], 0, 4, 64, 24, at[3], 1 << 30)),
                     ("g2048_tbf16_test_dw", (at[0], 0, at[1], 0, at[2], at[3], 16385, 64, 64, at[4], 1 << 30)),
                     ("g2048_tbf16_test_dw", (at[0], 0, at[1], 0, at[2], at[3], 513, 64, 64, at[4], 2 * (64 * 64 + 64) * 4 - 1))):
        assert getattr(lib, fn)(*args, None) == -1 and lib.g2048_tbf16_last_error().decode().startswith(fn + ": ")
    assert bytes(block) == bytes(len(block))


def test_host_layer_refuses_a_bad_grad_precision_before_anything_else():
    from g2048 import DeviceTransformerPolicy, ops
    model = R.stock_module(32, 1)
    for bad in ("f16", None, "BF16"):
        with pytest.raises(ValueError, match="'f32' or 'bf16'"):
            DeviceTransformerPolicy(model, grad_precision=bad)
        with pytest.raises(ValueError, match="'f32' or 'bf16'"):
            ops.tpolicy_loss_grad(*([torch.zeros(1)] * 6), 32, 1, grad_precision=bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        DeviceTransformerPolicy(model, grad_precision="bf16")           # the module lives on the CPU
    assert ops.GRAD_PRECISIONS == ("f32", "bf16")
