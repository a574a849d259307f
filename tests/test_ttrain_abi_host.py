"""The boundary of the fifth library (csrc/libg2048_ttrain_hip.so, include/g2048_ttrain.h: the transformer policy's training-mode
passes), what tests/test_libraries_abi_host.py checks for the other three beside the main one: its export table, its header, its
binding table and the inventory of bounds tests below name the same entry points, no name is shared with the other four libraries
(whose tables are unchanged), the build counts it, and its loader is loud and takes only the product's file name. Its argument
checks and workspace arithmetic are in tests/test_tpolicy_dropout_host.py."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import PKG, REPO
from test_abi_and_host import declared_symbols
from test_libraries_abi_host import ENTRY_POINTS, HOST, SIDE, SIZE, bound, exported

KEY, HEADER, SOURCES, PRODUCT = "TTRAIN_", "g2048_ttrain.h", ["g2048_tpolicy_train.hip"], "libg2048_ttrain_hip.so"
GPU = "tests/test_gpu_tpolicy_dropout.py"
# per entry point the GPU test that puts guard bands round what it writes, or (None, the reason it needs none)
GUARDED_BY = {
    "g2048_ttrain_last_error": (None, HOST),
    "g2048_ttrain_abi_version": (None, HOST),
    "g2048_tpolicy_train_workspace": (None, SIZE),
    "g2048_tpolicy_loss_grad_dropout": GPU + "::test_guard_bands_round_everything_the_two_passes_write",
    "g2048_tpolicy_forward_dropout": GPU + "::test_guard_bands_round_everything_the_two_passes_write",
    "g2048_tpolicy_dropout_mask": GPU + "::test_masks_equal_the_restatement",
}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    return _lib


def test_library_exports_its_header_and_its_binding_table(built):
    path, signatures, version, loaded = bound(built, KEY)
    names = declared_symbols(HEADER)
    assert exported(path) == names, (exported(path), names)
    assert set(names) == set(signatures) == set(GUARDED_BY) and len(names) == 6
    hdr = open(os.path.join(REPO, "include", HEADER)).read()
    in_header = int(re.search(r"#define G2048_TTRAIN_ABI_VERSION (\d+)", hdr).group(1))
    assert in_header == 1 == version == built.TTRAIN_ABI_VERSION == loaded.g2048_ttrain_abi_version()
    assert os.path.basename(path) == PRODUCT and os.path.dirname(path) == os.path.dirname(built.library_path())


def test_the_library_shares_no_entry_point_and_the_others_keep_their_tables(built):
    main = exported(built.library_path())
    assert main == declared_symbols() and set(main) == set(built.SIGNATURES), "the main library's export table moved"
    assert built.lib().g2048_abi_version() == built.ABI_VERSION == 5
    others = set(main)
    for other in sorted(SIDE):
        path, signatures, version, loaded = bound(built, SIDE[other]["key"])
        table = exported(path)
        assert table == declared_symbols(SIDE[other]["header"]) and set(table) == set(signatures) and len(table) == ENTRY_POINTS[other]
        assert getattr(loaded, "g2048_%s_abi_version" % other)() == version == 1
        others |= set(table)
    assert not set(built.TTRAIN_SIGNATURES) & others
    assert set(built.LIBRARIES) == {""} | {row["key"] for row in SIDE.values()} | {KEY}, "five libraries, a Library each"


def test_the_build_counts_the_library(built):
    from g2048 import _build
    real = _build.TTRAIN_LIB
    assert os.path.basename(real) == PRODUCT and _build.TTRAIN_SOURCES == SOURCES
    assert _build.LIBRARIES[KEY][:2] == (PRODUCT, "G2048_TTRAIN_LIB")
    elsewhere = sum((r[2] for k, r in _build.LIBRARIES.items() if k != KEY), [])
    assert not set(SOURCES) & set(elsewhere) and _build.SOURCES == _build.LIBRARIES[""][2]
    assert any(h.endswith(HEADER) for h in _build.PUBLIC_HEADERS)
    assert not _build.needs_build()
    products = [_build.path_of(k) for k in _build.LIBRARIES]
    assert len(products) == 5
    before = [os.path.getmtime(p) for p in products]
    try:
        _build.TTRAIN_LIB = os.path.join(os.path.dirname(real), "absent_ttrain.so")
        assert _build.needs_build(), "needs_build() does not look at the ttrain library"
    finally:
        _build.TTRAIN_LIB = real
    assert [os.path.getmtime(p) for p in products] == before and not _build.needs_build()
    flags = " ".join(_build.FLAGS)
    assert "-ffp-contract=off" in flags and "g2048_exports.map" in flags, "the same flags and the same version script as the others"


def test_every_entry_point_has_its_bounds_test_or_a_reason():
    for entry, where in GUARDED_BY.items():
        if isinstance(where, tuple):
            none, reason = where
            assert none is None and isinstance(reason, str) and len(reason.strip()) > 10 and "\n" not in reason, entry
            continue
        path, _, test = where.partition("::")
        source = open(os.path.join(REPO, path)).read()
        assert re.search(r"^def %s\(" % re.escape(test), source, re.M), "%s: %s has no test %s" % (entry, path, test)
        assert "pytest.mark.gpu" in source, "%s: %s is no GPU test file" % (entry, path)


def test_the_loader_is_loud_and_takes_only_the_product_name(built, tmp_path):
    """A missing library raises; a copy of the product under another name is refused when the table's row points at it, and is
    loaded only through the row's environment variable, which it says. Each in a fresh process: a library loads once."""
    variable = "G2048_TTRAIN_LIB"
    path = built.ttrain_library_path()
    code = ("import os, sys; sys.path.insert(0, %r); from g2048 import _build, _lib\n"
            "if os.environ.get('ROW_POINTS_AT'): _build.TTRAIN_LIB = os.environ['ROW_POINTS_AT']\n"
            "try:\n    print('LOADED', _lib.ttrain_lib().g2048_ttrain_abi_version())\n"
            "except RuntimeError as e:\n    print('REFUSED', e)\n" % PKG)
    clean = {k: v for k, v in os.environ.items() if k != variable}
    run = lambda **env: subprocess.run([sys.executable, "-c", code], env=dict(clean, **env), capture_output=True, text=True)  # noqa: E731
    out = run(**{variable: str(tmp_path / "absent.so")})
    assert "REFUSED" in out.stdout and "is missing" in out.stdout and "no CPU fallback" in out.stdout, out
    copy = shutil.copy(path, str(tmp_path / "libab.so"))
    out = run(ROW_POINTS_AT=copy)
    assert "REFUSED g2048: refusing to load %s: only csrc/%s is the " % (copy, PRODUCT) in out.stdout and "policy training library" in out.stdout, out
    assert "LOADED" not in out.stdout and "A/B build" not in out.stderr, out
    out = run(**{variable: copy})
    assert "LOADED 1" in out.stdout and "loading the A/B build %s (%s is set)" % (copy, variable) in out.stderr, out
