"""The training library's boundary (csrc/libg2048_train_hip.so, include/g2048_train.h), the counterpart of
tests/test_abi_and_host.py::test_export_table_equals_the_two_headers and tests/test_bounds_inventory.py for the second library:
its export table, its header, its binding table and the inventory of bounds tests below name the same entry points, and the main
library's export table is still exactly its own two headers'."""
import os
import re
import subprocess

import pytest

from conftest import PKG, REPO
from test_abi_and_host import declared_symbols

GPU = "tests/test_gpu_qnet_dropout.py"
HOST = "a host function: it writes no device memory"

# per entry point: the GPU test that puts canaries round what it writes, or (None, the reason it needs none)
GUARDED_BY = {
    "g2048_train_last_error": (None, HOST),
    "g2048_train_abi_version": (None, HOST),
    "g2048_qnet_train_workspace": (None, "a size query on the host: it writes no device memory"),
    "g2048_qnet_forward_batch_dropout": GPU + "::test_training_forwards_and_targets_against_the_masked_modules",
    "g2048_qnet_loss_grad_dropout": GPU + "::test_loss_and_gradients_against_the_masked_float64_module",
    "g2048_qnet_dropout_mask": GPU + "::test_masks_equal_the_restatement",
}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    return _lib


def exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_training_library_exports_its_header_and_its_binding_table(built):
    names = declared_symbols("g2048_train.h")
    assert exported(built.train_library_path()) == names, (exported(built.train_library_path()), names)
    assert set(names) == set(built.TRAIN_SIGNATURES) == set(GUARDED_BY)
    hdr = open(os.path.join(REPO, "include", "g2048_train.h")).read()
    version = int(re.search(r"#define G2048_TRAIN_ABI_VERSION (\d+)", hdr).group(1))
    assert version == 1 == built.TRAIN_ABI_VERSION == built.train_lib().g2048_train_abi_version()
    assert os.path.basename(built.train_library_path()) == "libg2048_train_hip.so"
    assert os.path.dirname(built.train_library_path()) == os.path.dirname(built.library_path())


def test_the_two_libraries_share_no_entry_point_and_the_main_one_keeps_its_table(built):
    main = exported(built.library_path())
    assert main == declared_symbols() and set(main) == set(built.SIGNATURES), "the main library's export table moved"
    assert not set(main) & set(built.TRAIN_SIGNATURES)
    assert built.lib().g2048_abi_version() == built.ABI_VERSION == 5


def test_every_training_entry_point_has_its_bounds_test_or_a_reason():
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
    """A missing library raises; a library under another name is loaded only through G2048_TRAIN_LIB, and says so."""
    import shutil
    import sys
    code = ("import sys; sys.path.insert(0, %r); from g2048 import _lib\n"
            "try:\n    print('LOADED', _lib.train_lib().g2048_train_abi_version())\n"
            "except RuntimeError as e:\n    print('REFUSED', 'missing' in str(e))\n" % PKG)
    run = lambda env: subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    out = run(dict(os.environ, G2048_TRAIN_LIB=str(tmp_path / "absent.so")))
    assert "REFUSED True" in out.stdout, out
    copy = shutil.copy(built.train_library_path(), str(tmp_path / "libab.so"))
    out = run(dict(os.environ, G2048_TRAIN_LIB=copy))
    assert "LOADED 1" in out.stdout and "loading the A/B build" in out.stderr, out
