"""The step library's boundary (csrc/libg2048_tstep_hip.so, include/g2048_tstep.h), the counterpart of
tests/test_tlearn_abi_host.py for the fourth library: its export table, its header, its binding table and the inventory of bounds
tests below name the same entry points, no name is shared with the other three libraries, whose tables are still exactly their own,
the loader is loud, and every argument check of g2048_tpolicy_adam_step happens before any device call (there is no device here)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import PKG, REPO
from test_abi_and_host import declared_symbols
from test_train_abi_host import exported

GPU = "tests/test_gpu_tpolicy_step.py"
HOST = "a host function: it writes no device memory"

# per entry point: the GPU test that puts guard bands round what it writes, or (None, the reason it needs none)
GUARDED_BY = {
    "g2048_tstep_last_error": (None, HOST),
    "g2048_tstep_abi_version": (None, HOST),
    "g2048_tpolicy_step_workspace": (None, "a size query on the host: it writes no device memory"),
    "g2048_tpolicy_adam_step": GPU + "::test_guard_bands_round_everything_the_entry_point_writes",
}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    return _lib


def test_step_library_exports_its_header_and_its_binding_table(built):
    names = declared_symbols("g2048_tstep.h")
    assert exported(built.tstep_library_path()) == names, (exported(built.tstep_library_path()), names)
    assert set(names) == set(built.TSTEP_SIGNATURES) == set(GUARDED_BY) and len(names) == 4
    hdr = open(os.path.join(REPO, "include", "g2048_tstep.h")).read()
    version = int(re.search(r"#define G2048_TSTEP_ABI_VERSION (\d+)", hdr).group(1))
    assert version == 1 == built.TSTEP_ABI_VERSION == built.tstep_lib().g2048_tstep_abi_version()
    assert os.path.basename(built.tstep_library_path()) == "libg2048_tstep_hip.so"
    assert os.path.dirname(built.tstep_library_path()) == os.path.dirname(built.library_path())


def test_the_four_libraries_share_no_entry_point_and_the_other_three_keep_their_tables(built):
    main, train, tlearn = exported(built.library_path()), exported(built.train_library_path()), exported(built.tlearn_library_path())
    assert main == declared_symbols() and set(main) == set(built.SIGNATURES), "the main library's export table moved"
    assert train == declared_symbols("g2048_train.h") and set(train) == set(built.TRAIN_SIGNATURES) and len(train) == 6
    assert tlearn == declared_symbols("g2048_tlearn.h") and set(tlearn) == set(built.TLEARN_SIGNATURES) and len(tlearn) == 4
    assert not set(built.TSTEP_SIGNATURES) & (set(main) | set(train) | set(tlearn))
    assert built.lib().g2048_abi_version() == built.ABI_VERSION == 5
    assert built.train_lib().g2048_train_abi_version() == built.TRAIN_ABI_VERSION == 1
    assert built.tlearn_lib().g2048_tlearn_abi_version() == built.TLEARN_ABI_VERSION == 1


def test_the_build_counts_the_fourth_library(built):
    from g2048 import _build
    assert os.path.basename(_build.TSTEP_LIB) == "libg2048_tstep_hip.so" and _build.TSTEP_SOURCES == ["g2048_tpolicy_step.hip"]
    assert _build.TLEARN_SOURCES == ["g2048_tpolicy_grad.hip"] and "g2048_tpolicy_step.hip" not in _build.SOURCES + _build.TRAIN_SOURCES
    assert any(h.endswith("g2048_tstep.h") for h in _build.PUBLIC_HEADERS)
    assert not _build.needs_build()
    real = _build.TSTEP_LIB
    try:
        _build.TSTEP_LIB = os.path.join(os.path.dirname(real), "absent_tstep.so")
        assert _build.needs_build(), "needs_build() does not look at the step library"
    finally:
        _build.TSTEP_LIB = real


def test_every_step_entry_point_has_its_bounds_test_or_a_reason():
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
    """A missing library raises; a library under another name is loaded only through G2048_TSTEP_LIB, and says so."""
    import shutil
    import sys
    code = ("import sys; sys.path.insert(0, %r); from g2048 import _lib\n"
            "try:\n    print('LOADED', _lib.tstep_lib().g2048_tstep_abi_version())\n"
            "except RuntimeError as e:\n    print('REFUSED', 'missing' in str(e))\n" % PKG)
    run = lambda env: subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)      # noqa: E731
    out = run(dict(os.environ, G2048_TSTEP_LIB=str(tmp_path / "absent.so")))
    assert "REFUSED True" in out.stdout, out
    copy = shutil.copy(built.tstep_library_path(), str(tmp_path / "libab.so"))
    out = run(dict(os.environ, G2048_TSTEP_LIB=copy))
    assert "LOADED 1" in out.stdout and "loading the A/B build" in out.stderr, out
    # without the variable a foreign name is refused: the path is fixed at import, so the refusal is read off the loader's source
    src = open(os.path.join(PKG, "g2048", "_lib.py")).read()
    assert 'os.path.basename(path) != "libg2048_tstep_hip.so"' in src


def test_workspace_query_refuses_shapes_and_is_a_multiple_of_16(built):
    ws = built.tstep_lib().g2048_tpolicy_step_workspace
    assert ws(48, 2) == 0 and ws(0, 2) == 0 and ws(2048, 0) == 0 and ws(2048, 65) == 0 and ws(65568, 2) == 0 and ws(-32, 2) == 0
    shapes = [(ff, l) for ff in (32, 96, 2048, 4096, 65536) for l in (1, 2, 3, 64)]
    assert all(ws(ff, l) > 0 and ws(ff, l) % 16 == 0 for ff, l in shapes)
    assert max(ws(ff, l) for ff, l in shapes) <= 1024 * 8 + 16, "at most 1,024 partial sums and one 16-byte record"
    # a partial per 1,024 floats up to 1,024 partials: 158, 194 and 686 of them; at 1,230,601 floats a chunk is 2,048 floats: 601
    assert [ws(32, 1), ws(96, 2), ws(2048, 2), ws(4096, 2)] == [158 * 8 + 16, 194 * 8 + 16, 686 * 8 + 16, 601 * 8 + 8 + 16]


def test_argument_checks_happen_before_any_device_call(built):
    """Host addresses that are never dereferenced: every refusal is decided from the arguments alone, each call below with exactly
    one defect."""
    T = built.tstep_lib()
    err = lambda: T.g2048_tstep_last_error().decode()      # noqa: E731
    ff, layers = 96, 2
    nb = T.g2048_tpolicy_step_workspace(ff, layers)
    p = 0x10000                                              # 16-byte aligned, not null
    f = C.c_float
    nan, inf = float("nan"), float("inf")

    def call(plain=p, grad=p, m=p, v=p, ff=ff, layers=layers, loss=p, counters=p, lr=3e-4, b1=0.9, b2=0.999, eps=1e-8, max_norm=0.5,
             norm=p, ws=p, nb=nb):
        return T.g2048_tpolicy_adam_step(plain, grad, m, v, ff, layers, loss, counters, f(lr), f(b1), f(b2), f(eps), f(max_norm), norm, ws,
                                         nb, None)

    for name in ("plain", "grad", "m", "v", "counters", "norm", "ws"):
        assert call(**{name: None}) == -1 and "g2048_tpolicy_adam_step: null pointer" in err(), name
    for name in ("plain", "grad", "m", "v", "ws"):
        for off in (4, 8):
            assert call(**{name: p + off}) == -1 and "misaligned" in err(), (name, off)
    assert call(counters=p + 4) == -1 and "misaligned" in err()
    assert call(norm=p + 2) == -1 and "misaligned" in err()
    assert call(loss=p + 2) == -1 and "misaligned" in err()
    assert call(ff=48) == -1 and "multiple of 32" in err()
    assert call(ff=65568) == -1 and "multiple of 32" in err()
    assert call(layers=0) == -1 and "n_layers" in err()
    assert call(layers=65) == -1 and "n_layers" in err()
    for key in ("lr", "b1", "b2", "eps"):
        for bad in (nan, inf, -inf, -1e-3):
            assert call(**{key: bad}) == -1 and "finite and not negative" in err(), (key, bad)
    for key in ("b1", "b2"):
        for bad in (1.0, 1.5):
            assert call(**{key: bad}) == -1 and "must be below 1" in err(), (key, bad)
    for bad in (nan, 0.0, -0.5, -inf):
        assert call(max_norm=bad) == -1 and "max_norm must be above 0" in err(), bad
    assert call(nb=nb - 1) == -1 and "workspace" in err() and str(nb) in err()
    assert call(nb=0) == -1 and str(nb) in err()


def test_python_refuses_before_the_library(built):
    from g2048 import ops
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.tpolicy_step_workspace_bytes(48, 2)
    with pytest.raises(ValueError, match="1 .. 64 layers"):
        ops.tpolicy_step_workspace_bytes(2048, 0)
    assert ops.tpolicy_step_workspace_bytes(2048, 2) == 686 * 8 + 16
