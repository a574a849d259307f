"""The boundary of the experience collector's library (csrc/libg2048_collect_hip.so, include/g2048_collect.h), the one row of the
SECOND library table (g2048._build.EXTENSIONS, g2048._lib.EXTENSIONS): what tests/test_ttrain_abi_host.py checks for the fifth
library. Its export table, its header, its binding table and the inventory of bounds tests below name the same entry points, no
name is shared with the five libraries (whose tables, counts and versions are unchanged), the build counts it, its loader is loud
and takes only the product's file name, and g2048_qnet_collect checks every argument before any device call."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import PKG, REPO
from test_abi_and_host import declared_symbols
from test_libraries_abi_host import ENTRY_POINTS, HOST, SIDE, SIZE, bound, exported

KEY, HEADER, SOURCES, PRODUCT = "COLLECT_", "g2048_collect.h", ["g2048_qnet_collect.hip"], "libg2048_collect_hip.so"
GPU = "tests/test_gpu_qnet_collect.py"
# per entry point the GPU test that puts guard bands round what it writes, or (None, the reason it needs none)
GUARDED_BY = {
    "g2048_collect_last_error": (None, HOST),
    "g2048_collect_abi_version": (None, HOST),
    "g2048_qnet_collect_workspace": (None, SIZE),
    "g2048_qnet_collect": GPU + "::test_guard_bands_round_everything_the_call_writes",
}
FIVE = {"": 5, "TRAIN_": 1, "TLEARN_": 1, "TSTEP_": 1, "TTRAIN_": 1}          # the five libraries' ABI versions


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
    assert set(names) == set(signatures) == set(GUARDED_BY) and len(names) == 4
    hdr = open(os.path.join(REPO, "include", HEADER)).read()
    in_header = int(re.search(r"#define G2048_COLLECT_ABI_VERSION (\d+)", hdr).group(1))
    assert in_header == 1 == version == built.COLLECT_ABI_VERSION == loaded.g2048_collect_abi_version()
    assert os.path.basename(path) == PRODUCT and os.path.dirname(path) == os.path.dirname(built.library_path())


def test_the_library_shares_no_entry_point_and_the_five_keep_their_tables(built):
    from g2048 import _build
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
    ttrain = exported(built.ttrain_library_path())
    assert ttrain == declared_symbols("g2048_ttrain.h") and set(ttrain) == set(built.TTRAIN_SIGNATURES) and len(ttrain) == 6
    others |= set(ttrain)
    assert not set(built.COLLECT_SIGNATURES) & others
    # the two tables: five rows and one, the same keys in the build's and the binding's, the same class in both of the binding's
    assert set(built.LIBRARIES) == set(_build.LIBRARIES) == set(FIVE) and set(built.EXTENSIONS) == set(_build.EXTENSIONS) == {KEY}
    assert {k: lib.version for k, lib in built.LIBRARIES.items()} == FIVE
    assert all(type(lib) is built.Library for lib in list(built.LIBRARIES.values()) + list(built.EXTENSIONS.values()))
    assert built.EXTENSIONS[KEY].key == KEY and built.EXTENSIONS[KEY].stem == "g2048_collect"


def test_the_build_counts_the_library(built):
    from g2048 import _build
    real = _build.COLLECT_LIB
    assert os.path.basename(real) == PRODUCT and _build.COLLECT_SOURCES == SOURCES
    assert _build.EXTENSIONS[KEY][:2] == (PRODUCT, "G2048_COLLECT_LIB") and len(_build.EXTENSIONS) == 1 and len(_build.LIBRARIES) == 5
    elsewhere = sum((r[2] for r in _build.LIBRARIES.values()), [])
    assert not set(SOURCES) & set(elsewhere) and _build.SOURCES == _build.LIBRARIES[""][2]
    assert any(h.endswith(HEADER) for h in _build.PUBLIC_HEADERS)
    assert _build.path_of(KEY) == real
    assert not _build.needs_build()
    products = [_build.path_of(k) for k in list(_build.LIBRARIES) + list(_build.EXTENSIONS)]
    assert len(products) == 6 and len(set(products)) == 6
    before = [os.path.getmtime(p) for p in products]
    try:
        _build.COLLECT_LIB = os.path.join(os.path.dirname(real), "absent_collect.so")
        assert _build.needs_build(), "needs_build() does not look at the collect library"
    finally:
        _build.COLLECT_LIB = real
    assert [os.path.getmtime(p) for p in products] == before and not _build.needs_build()
    flags = " ".join(_build.FLAGS)
    assert "-ffp-contract=off" in flags and "g2048_exports.map" in flags, "the same flags and the same version script as the others"


def test_the_collect_switch_builds_the_library_alone(built, tmp_path):
    out = str(tmp_path / "libab_collect.so")
    run = subprocess.run([sys.executable, "-m", "g2048._build", "--collect", "-o", out], cwd=PKG, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.strip().splitlines()[-1] == out and exported(out) == declared_symbols(HEADER)
    assert "g2048_qnet_collect.hip" in run.stdout and "g2048_qnet.hip" not in run.stdout


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
    variable = "G2048_COLLECT_LIB"
    path = built.collect_library_path()
    code = ("import os, sys; sys.path.insert(0, %r); from g2048 import _build, _lib\n"
            "if os.environ.get('ROW_POINTS_AT'): _build.COLLECT_LIB = os.environ['ROW_POINTS_AT']\n"
            "try:\n    print('LOADED', _lib.collect_lib().g2048_collect_abi_version())\n"
            "except RuntimeError as e:\n    print('REFUSED', e)\n" % PKG)
    clean = {k: v for k, v in os.environ.items() if k != variable}
    run = lambda **env: subprocess.run([sys.executable, "-c", code], env=dict(clean, **env), capture_output=True, text=True)  # noqa: E731
    out = run(**{variable: str(tmp_path / "absent.so")})
    assert "REFUSED" in out.stdout and "is missing" in out.stdout and "no CPU fallback" in out.stdout, out
    copy = shutil.copy(path, str(tmp_path / "libab.so"))
    out = run(ROW_POINTS_AT=copy)
    assert "REFUSED g2048: refusing to load %s: only csrc/%s is the " % (copy, PRODUCT) in out.stdout and "collector library" in out.stdout, out
    assert "LOADED" not in out.stdout and "A/B build" not in out.stderr, out
    out = run(**{variable: copy})
    assert "LOADED 1" in out.stdout and "loading the A/B build %s (%s is set)" % (copy, variable) in out.stderr, out


# ---- g2048_qnet_collect's argument checks: all of them before any device call, so host memory serves ------------------------------
GOOD = dict(dim_ff=32, n_layers=1, opts=0, epsilon=0.5, beam_width=0, search_depth=30, threshold=64, seed=1, step_index0=0, env_id_base=0,
            n=8, steps=2, max_episode_steps=0, capacity=64, size=3, head=5)
POINTERS = ("boards", "score", "moves", "packed", "states", "next_states", "actions", "rewards", "dones", "priorities", "flags", "workspace")


def collect(lib, base, **changes):
    """The call with GOOD's arguments and every pointer at its own 16-byte aligned place in the host block at `base`, but for
    `changes` (a pointer's name: its new address). Returns (status, message)."""
    a = dict(GOOD, **{name: base + 64 * i for i, name in enumerate(POINTERS)})
    a.update(changes)
    rc = lib.g2048_qnet_collect(a["boards"], a["score"], a["moves"], a["packed"], a["dim_ff"], a["n_layers"], a["opts"], a["epsilon"],
                                a["beam_width"], a["search_depth"], a["threshold"], a["seed"], a["step_index0"], a["env_id_base"], a["n"],
                                a["steps"], a["max_episode_steps"], a["states"], a["next_states"], a["actions"], a["rewards"], a["dones"],
                                a["priorities"], a["capacity"], a["size"], a["head"], a["flags"], a["workspace"], None)
    return rc, lib.g2048_collect_last_error().decode()


REFUSED = [
    ("a null board pointer", dict(boards=None), "null pointer"),
    ("a null ring array", dict(next_states=None), "null pointer"),
    ("a null workspace", dict(workspace=None), "null pointer"),
    ("steps 0", dict(steps=0), "steps must be at least 1"),
    ("negative steps", dict(steps=-3), "steps must be at least 1"),
    ("more transitions than slots", dict(steps=9), "more transitions than the buffer's capacity (steps x n = 9 x 8, capacity 64)"),
    ("a product that overflows 32 bits", dict(steps=0x7fffffff, n=0x7fffffff, capacity=1 << 40), "more transitions than the buffer's capacity"),
    ("size above capacity", dict(size=65), "size must be at most capacity and head below it"),
    ("head at capacity", dict(head=64), "size must be at most capacity and head below it"),
    ("a negative episode cap", dict(max_episode_steps=-1), "max_episode_steps must be 0 (no cap) or positive"),
    ("epsilon below 0", dict(epsilon=-0.01), "epsilon must lie in [0, 1]"),
    ("epsilon above 1", dict(epsilon=1.5), "epsilon must lie in [0, 1]"),
    ("epsilon NaN", dict(epsilon=float("nan")), "epsilon must lie in [0, 1]"),
    ("a beam wider than 64", dict(beam_width=65), "beam_width must lie in 1 .. 64"),
    ("a negative beam width", dict(beam_width=-1), "beam_width must lie in 1 .. 64"),
    ("depth 1 with the beam on", dict(beam_width=3, search_depth=1), "search_depth 1 asks the network about every candidate"),
    ("depth 0 with the beam on", dict(beam_width=3, search_depth=0), "search_depth must be at least 1"),
    ("threshold 0 with the beam on", dict(beam_width=3, threshold=0), "threshold (a tile value) must be at least 1"),
    ("dim_ff no multiple of 32", dict(dim_ff=48), "dim_ff must be a multiple of 32"),
    ("no layer", dict(n_layers=0), "dim_ff must be a multiple of 32 (32 .. 65536) and n_layers 1 .. 64"),
    ("an unknown precision", dict(opts=2), "unknown opts (precision)"),
]


@pytest.mark.parametrize("what,changes,message", REFUSED, ids=[r[0] for r in REFUSED])
def test_arguments_are_checked_without_a_device(built, what, changes, message):
    lib = built.collect_lib()
    block = (C.c_uint8 * (64 * len(POINTERS) + 16))()
    base = (C.addressof(block) + 15) & ~15
    rc, said = collect(lib, base, **changes)
    assert rc == -1 and said.startswith("g2048_qnet_collect: ") and message in said, (what, rc, said)


@pytest.mark.parametrize("name,off", [("boards", 8), ("packed", 4), ("states", 8), ("next_states", 1), ("score", 2), ("moves", 1),
                                      ("rewards", 2), ("priorities", 3), ("workspace", 1)])
def test_misaligned_pointers_are_refused(built, name, off):
    lib = built.collect_lib()
    block = (C.c_uint8 * (64 * len(POINTERS) + 16))()
    base = (C.addressof(block) + 15) & ~15
    rc, said = collect(lib, base, **{name: base + 64 * POINTERS.index(name) + off})
    assert rc == -1 and "g2048_qnet_collect: misaligned pointer" in said, (name, rc, said)


def test_without_the_beam_its_settings_are_not_read_and_n_0_does_nothing(built):
    lib = built.collect_lib()
    block = (C.c_uint8 * (64 * len(POINTERS) + 16))()
    base = (C.addressof(block) + 15) & ~15
    # n == 0 returns OK before anything is looked at, null pointers included
    assert collect(lib, base, n=0)[0] == 0
    assert collect(lib, base, n=0, boards=None, steps=0, dim_ff=7)[0] == 0
    assert bytes(block) == bytes(len(block)), "n == 0 wrote to the arrays it was given"
    # beam_width 0: depth 1 and threshold 0 pass the beam's checks (the call then stops at the next bad argument)
    rc, said = collect(lib, base, search_depth=1, threshold=0, steps=0)
    assert rc == -1 and "steps must be at least 1" in said
    assert lib.g2048_qnet_collect_workspace(0) >= 4 and lib.g2048_qnet_collect_workspace(1 << 20) >= 4


def test_host_layer_fails_loudly_on_cpu(built):
    import torch
    from g2048 import ops
    ring = [torch.zeros((8, 16), dtype=torch.uint8), torch.zeros((8, 16), dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8),
            torch.zeros(8, dtype=torch.float32), torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.float32)]
    packed = torch.zeros(ops.qnet_packed_bytes("f32", 32, 1), dtype=torch.uint8)
    args = (torch.zeros((4, 16), dtype=torch.uint8), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), packed, 32, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.qnet_collect(*args, *ring, 0, 0, 2)
    for bad in (dict(steps=0), dict(steps=1, epsilon=1.5), dict(steps=1, beam_width=65), dict(steps=1, beam_width=3, search_depth=1),
                dict(steps=1, precision="f16"), dict(steps=1, max_episode_steps=-1)):
        steps = bad.pop("steps")
        with pytest.raises(ValueError):
            ops.qnet_collect(*args, *ring, 0, 0, steps, **bad)
