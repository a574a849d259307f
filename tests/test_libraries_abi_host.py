"""The boundary of the three libraries beside the main one (csrc/libg2048_train_hip.so, libg2048_tlearn_hip.so, libg2048_tstep_hip.so),
the counterpart of tests/test_abi_and_host.py::test_export_table_equals_the_two_headers and tests/test_bounds_inventory.py, once for
all of them: a library's export table, its header, its binding table and its inventory of bounds tests below name the same entry
points, no name is shared between any two of the four libraries, the build counts every one of them, and the loader of each of
the four is loud and takes only the product's file name. What only one library has is in tests/test_tlearn_abi_host.py and
tests/test_tstep_abi_host.py."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import PKG, REPO
from test_abi_and_host import declared_symbols

HOST = "a host function: it writes no device memory"
SIZE = "a size query on the host: it writes no device memory"
DROPOUT, TGRAD, TSTEP = "tests/test_gpu_qnet_dropout.py", "tests/test_gpu_tpolicy_grad.py", "tests/test_gpu_tpolicy_step.py"

# per library: its row of g2048._build.LIBRARIES and g2048._lib.LIBRARIES, its header, its ABI version, its sources, and per entry
# point the GPU test that puts guard bands round what it writes, or (None, the reason it needs none)
SIDE = {
    "train": dict(key="TRAIN_", header="g2048_train.h", version=1, sources=["g2048_qnet_train.hip"], guarded_by={
        "g2048_train_last_error": (None, HOST),
        "g2048_train_abi_version": (None, HOST),
        "g2048_qnet_train_workspace": (None, SIZE),
        "g2048_qnet_forward_batch_dropout": DROPOUT + "::test_training_forwards_and_targets_against_the_masked_modules",
        "g2048_qnet_loss_grad_dropout": DROPOUT + "::test_loss_and_gradients_against_the_masked_float64_module",
        "g2048_qnet_dropout_mask": DROPOUT + "::test_masks_equal_the_restatement",
    }),
    "tlearn": dict(key="TLEARN_", header="g2048_tlearn.h", version=1, sources=["g2048_tpolicy_grad.hip"], guarded_by={
        "g2048_tlearn_last_error": (None, HOST),
        "g2048_tlearn_abi_version": (None, HOST),
        "g2048_tpolicy_grad_workspace": (None, SIZE),
        "g2048_tpolicy_loss_grad": TGRAD + "::test_guard_bands_round_everything_the_entry_point_writes",
    }),
    "tstep": dict(key="TSTEP_", header="g2048_tstep.h", version=1, sources=["g2048_tpolicy_step.hip"], guarded_by={
        "g2048_tstep_last_error": (None, HOST),
        "g2048_tstep_abi_version": (None, HOST),
        "g2048_tpolicy_step_workspace": (None, SIZE),
        "g2048_tpolicy_adam_step": TSTEP + "::test_guard_bands_round_everything_the_entry_point_writes",
    }),
}
ENTRY_POINTS = {"train": 6, "tlearn": 4, "tstep": 4}
side = pytest.mark.parametrize("name", sorted(SIDE))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    return _lib


def exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def bound(_lib, key):
    """(path, binding table, binding's ABI version, loaded library) of row `key`, through the module's own names."""
    low = key.lower()
    return (getattr(_lib, low + "library_path")(), getattr(_lib, key + "SIGNATURES"), getattr(_lib, key + "ABI_VERSION"),
            getattr(_lib, low + "lib")())


@side
def test_library_exports_its_header_and_its_binding_table(built, name):
    row = SIDE[name]
    path, signatures, version, loaded = bound(built, row["key"])
    names = declared_symbols(row["header"])
    assert exported(path) == names, (exported(path), names)
    assert set(names) == set(signatures) == set(row["guarded_by"]) and len(names) == ENTRY_POINTS[name]
    hdr = open(os.path.join(REPO, "include", row["header"])).read()
    in_header = int(re.search(r"#define G2048_%sABI_VERSION (\d+)" % row["key"], hdr).group(1))
    assert in_header == row["version"] == 1 == version == getattr(loaded, "g2048_%s_abi_version" % name)()
    assert os.path.basename(path) == "libg2048_%s_hip.so" % name
    assert os.path.dirname(path) == os.path.dirname(built.library_path())


@side
def test_the_library_shares_no_entry_point_and_the_others_keep_their_tables(built, name):
    main = exported(built.library_path())
    assert main == declared_symbols() and set(main) == set(built.SIGNATURES), "the main library's export table moved"
    assert built.lib().g2048_abi_version() == built.ABI_VERSION == 5
    others = set(main)
    for other in sorted(set(SIDE) - {name}):
        path, signatures, version, loaded = bound(built, SIDE[other]["key"])
        table = exported(path)
        assert table == declared_symbols(SIDE[other]["header"]) and set(table) == set(signatures) and len(table) == ENTRY_POINTS[other]
        assert getattr(loaded, "g2048_%s_abi_version" % other)() == version == 1
        others |= set(table)
    assert not set(bound(built, SIDE[name]["key"])[1]) & others


@side
def test_the_build_counts_the_library(built, name):
    from g2048 import _build
    row = SIDE[name]
    attr = row["key"] + "LIB"
    real = getattr(_build, attr)
    assert os.path.basename(real) == "libg2048_%s_hip.so" % name and getattr(_build, row["key"] + "SOURCES") == row["sources"]
    elsewhere = sum((r[2] for k, r in _build.LIBRARIES.items() if k != row["key"]), [])
    assert not set(row["sources"]) & set(elsewhere) and _build.SOURCES == _build.LIBRARIES[""][2]
    assert any(h.endswith(row["header"]) for h in _build.PUBLIC_HEADERS)
    assert not _build.needs_build()
    products = [_build.path_of(k) for k in _build.LIBRARIES]
    before = [os.path.getmtime(p) for p in products]
    try:
        setattr(_build, attr, os.path.join(os.path.dirname(real), "absent_%s.so" % name))
        assert _build.needs_build(), "needs_build() does not look at the %s library" % name
    finally:
        setattr(_build, attr, real)
    assert [os.path.getmtime(p) for p in products] == before and not _build.needs_build()


@side
def test_every_entry_point_has_its_bounds_test_or_a_reason(name):
    for entry, where in SIDE[name]["guarded_by"].items():
        if isinstance(where, tuple):
            none, reason = where
            assert none is None and isinstance(reason, str) and len(reason.strip()) > 10 and "\n" not in reason, entry
            continue
        path, _, test = where.partition("::")
        source = open(os.path.join(REPO, path)).read()
        assert re.search(r"^def %s\(" % re.escape(test), source, re.M), "%s: %s has no test %s" % (entry, path, test)
        assert "pytest.mark.gpu" in source, "%s: %s is no GPU test file" % (entry, path)


@pytest.mark.parametrize("key,role", [("", "product library"), ("TRAIN_", "training library"), ("TLEARN_", "learner library"),
                                      ("TSTEP_", "step library")])
def test_the_loader_is_loud_and_takes_only_the_product_name(built, tmp_path, key, role):
    """A missing library raises; a copy of the product under another name is refused when the table's row points at it, and is
    loaded only through the row's environment variable, which it says. Each in a fresh process: a library loads once."""
    from g2048 import _build
    product, variable = _build.LIBRARIES[key][:2]
    path, _, version, _ = bound(built, key)
    code = ("import os, sys; sys.path.insert(0, %r); from g2048 import _build, _lib\n"
            "if os.environ.get('ROW_POINTS_AT'): _build.%sLIB = os.environ['ROW_POINTS_AT']\n"
            "try:\n    print('LOADED', _lib.%slib().%s_abi_version())\n"
            "except RuntimeError as e:\n    print('REFUSED', e)\n" % (PKG, key, key.lower(), built.LIBRARIES[key].stem))
    clean = {k: v for k, v in os.environ.items() if k != variable}
    run = lambda **env: subprocess.run([sys.executable, "-c", code], env=dict(clean, **env), capture_output=True, text=True)  # noqa: E731
    out = run(**{variable: str(tmp_path / "absent.so")})
    assert "REFUSED" in out.stdout and "is missing" in out.stdout and "no CPU fallback" in out.stdout, out
    copy = shutil.copy(path, str(tmp_path / "libab.so"))
    out = run(ROW_POINTS_AT=copy)
    assert "REFUSED g2048: refusing to load %s: only csrc/%s is the " % (copy, product) in out.stdout and role in out.stdout, out
    assert "LOADED" not in out.stdout and "A/B build" not in out.stderr, out
    out = run(**{variable: copy})
    assert "LOADED %d" % version in out.stdout and "loading the A/B build %s (%s is set)" % (copy, variable) in out.stderr, out
