"""The learner library's boundary (csrc/libg2048_tlearn_hip.so, include/g2048_tlearn.h), the counterpart of
tests/test_train_abi_host.py for the third library: its export table, its header, its binding table and the inventory of bounds
tests below name the same entry points, no name is shared with the other two libraries, whose tables are still exactly their own,
the loader is loud, and every argument check of g2048_tpolicy_loss_grad happens before any device call (there is no device here)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import PKG, REPO
from test_abi_and_host import declared_symbols
from test_train_abi_host import exported

GPU = "tests/test_gpu_tpolicy_grad.py"
HOST = "a host function: it writes no device memory"

# per entry point: the GPU test that puts guard bands round what it writes, or (None, the reason it needs none)
GUARDED_BY = {
    "g2048_tlearn_last_error": (None, HOST),
    "g2048_tlearn_abi_version": (None, HOST),
    "g2048_tpolicy_grad_workspace": (None, "a size query on the host: it writes no device memory"),
    "g2048_tpolicy_loss_grad": GPU + "::test_guard_bands_round_everything_the_entry_point_writes",
}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    return _lib


def test_learner_library_exports_its_header_and_its_binding_table(built):
    names = declared_symbols("g2048_tlearn.h")
    assert exported(built.tlearn_library_path()) == names, (exported(built.tlearn_library_path()), names)
    assert set(names) == set(built.TLEARN_SIGNATURES) == set(GUARDED_BY)
    hdr = open(os.path.join(REPO, "include", "g2048_tlearn.h")).read()
    version = int(re.search(r"#define G2048_TLEARN_ABI_VERSION (\d+)", hdr).group(1))
    assert version == 1 == built.TLEARN_ABI_VERSION == built.tlearn_lib().g2048_tlearn_abi_version()
    assert int(re.search(r"#define G2048_TLEARN_BATCH_MAX (\d+)", hdr).group(1)) == 1024 == built.TLEARN_BATCH_MAX
    assert os.path.basename(built.tlearn_library_path()) == "libg2048_tlearn_hip.so"
    assert os.path.dirname(built.tlearn_library_path()) == os.path.dirname(built.library_path())


def test_the_three_libraries_share_no_entry_point_and_the_other_two_keep_their_tables(built):
    main, train = exported(built.library_path()), exported(built.train_library_path())
    assert main == declared_symbols() and set(main) == set(built.SIGNATURES), "the main library's export table moved"
    assert train == declared_symbols("g2048_train.h") and set(train) == set(built.TRAIN_SIGNATURES) and len(train) == 6
    assert not set(built.TLEARN_SIGNATURES) & (set(main) | set(train))
    assert built.lib().g2048_abi_version() == built.ABI_VERSION == 5
    assert built.train_lib().g2048_train_abi_version() == built.TRAIN_ABI_VERSION == 1


def test_the_build_counts_the_third_library(built):
    from g2048 import _build
    assert os.path.basename(_build.TLEARN_LIB) == "libg2048_tlearn_hip.so" and _build.TLEARN_SOURCES == ["g2048_tpolicy_grad.hip"]
    assert any(h.endswith("g2048_tlearn.h") for h in _build.PUBLIC_HEADERS)
    assert not _build.needs_build()
    real = _build.TLEARN_LIB
    try:
        _build.TLEARN_LIB = os.path.join(os.path.dirname(real), "absent_tlearn.so")
        assert _build.needs_build(), "needs_build() does not look at the learner library"
    finally:
        _build.TLEARN_LIB = real


def test_every_learner_entry_point_has_its_bounds_test_or_a_reason():
    for name, where in GUARDED_BY.items():
        if isinstance(where, tuple):
            none, reason = where
            assert none is None and isinstance(reason, str) and len(reason.strip()) > 10 and "\n" not in reason, name
            continue
        path, _, test = where.partition("::")
        source = open(os.path.join(REPO, path)).read()
        assert re.search(r"^def %s\(" % re.escape(test), source, re.M), "%s: %s has no test %s" % (name, path, test)
        assert "pytest.mark.gpu" in source, "%s: %s is no GPU test file" % (name, path)


def test_the_loader_is_loud_and_takes_only_the_product_name(built, tmp_path):
    """A missing library raises; a library under another name is loaded only through G2048_TLEARN_LIB, and says so."""
    import shutil
    import sys
    code = ("import sys; sys.path.insert(0, %r); from g2048 import _lib\n"
            "try:\n    print('LOADED', _lib.tlearn_lib().g2048_tlearn_abi_version())\n"
            "except RuntimeError as e:\n    print('REFUSED', 'missing' in str(e))\n" % PKG)
    run = lambda env: subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)      # noqa: E731
    out = run(dict(os.environ, G2048_TLEARN_LIB=str(tmp_path / "absent.so")))
    assert "REFUSED True" in out.stdout, out
    copy = shutil.copy(built.tlearn_library_path(), str(tmp_path / "libab.so"))
    out = run(dict(os.environ, G2048_TLEARN_LIB=copy))
    assert "LOADED 1" in out.stdout and "loading the A/B build" in out.stderr, out
    # without the variable a foreign name is refused: the path is fixed at import, so the refusal is read off the loader's source
    src = open(os.path.join(PKG, "g2048", "_lib.py")).read()
    assert 'os.path.basename(path) != "libg2048_tlearn_hip.so"' in src


def test_workspace_query_refuses_shapes_and_grows(built):
    ws = built.tlearn_lib().g2048_tpolicy_grad_workspace
    assert ws(0, 2048, 2) == 0 and ws(1025, 2048, 2) == 0 and ws(64, 48, 2) == 0 and ws(64, 0, 2) == 0 and ws(64, 2048, 0) == 0
    assert ws(64, 2048, 65) == 0 and ws(64, 65568, 2) == 0
    assert 0 < ws(1, 32, 1) < ws(2, 32, 1) < ws(17, 32, 1) < ws(1024, 32, 1)
    assert ws(64, 32, 2) < ws(64, 64, 2) < ws(64, 2048, 2) and ws(64, 2048, 1) < ws(64, 2048, 2)
    assert all(ws(n, ff, l) % 16 == 0 for n in (1, 3, 17, 1024) for ff in (32, 96, 2048) for l in (1, 3))
    assert ws(1024, 2048, 2) == 396800000, "the figure DESIGN.md states for N = 1,024, dim_ff 2,048, 2 layers"


def test_argument_checks_happen_before_any_device_call(built):
    """Host addresses that are never dereferenced: every refusal is decided from the arguments alone, and N = 0 returns 0."""
    T = built.tlearn_lib()
    err = lambda: T.g2048_tlearn_last_error().decode()      # noqa: E731
    n, ff, layers = 17, 96, 2
    nb = T.g2048_tpolicy_grad_workspace(n, ff, layers)
    p = 0x10000                                              # 16-byte aligned, not null
    f = C.c_float

    def call(boards=p, plain=p, actions=p, old=p, adv=p, ret=p, n=n, ff=ff, layers=layers, clip=0.3, vc=0.4, ec=0.05, grad=p, losses=p,
             probs=p, value=p, ws=p, nb=nb):
        return T.g2048_tpolicy_loss_grad(boards, plain, actions, old, adv, ret, n, ff, layers, f(clip), f(vc), f(ec), grad, losses, probs,
                                         value, ws, nb, None)

    assert call(n=0) == 0, "N = 0 returns G2048_OK and launches nothing"
    assert call(n=0, boards=None, ws=None, nb=0) == 0
    for name in ("boards", "plain", "actions", "old", "adv", "ret", "grad", "losses", "probs", "value", "ws"):
        assert call(**{name: None}) == -1 and "null pointer" in err(), name
    assert call(n=1025, nb=1 << 40) == -1 and "1024" in err()
    assert call(ff=48) == -1 and "multiple of 32" in err()
    assert call(layers=0) == -1 and "n_layers" in err()
    assert call(nb=nb - 1) == -1 and "workspace" in err() and str(nb) in err()
    for name, off in (("boards", 8), ("plain", 4), ("grad", 8), ("probs", 4), ("ws", 8), ("actions", 4), ("old", 2), ("losses", 1), ("value", 2)):
        assert call(**{name: p + off}) == -1 and "misaligned" in err(), name
    for name in ("clip", "vc", "ec"):
        assert call(**{name: -0.1}) == -1 and call(**{name: float("nan")}) == -1 and call(**{name: float("inf")}) == -1, name
        assert "finite" in err()


def test_python_refuses_before_the_library(built):
    from g2048 import ops
    with pytest.raises(ValueError, match="1024"):
        ops.tpolicy_grad_workspace_bytes(1025, 2048, 2)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.tpolicy_grad_workspace_bytes(64, 48, 2)
    assert ops.tpolicy_grad_workspace_bytes(1024, 2048, 2) == 396800000
