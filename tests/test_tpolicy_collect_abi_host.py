"""The boundary of the transformer policy's collector library (csrc/libg2048_tpolicy_collect_hip.so,
include/g2048_tpolicy_collect.h), the first row of the FOURTH, open-ended library table (g2048._build.EXTRA_ROWS,
g2048._lib.EXTRA_ROWS): what tests/test_ppo_collect_abi_host.py checks for the seventh library. Its export table, its header, its
binding table and the inventory of bounds tests below name the same entry points, no name is shared with the seven other libraries
(whose tables, counts and versions are unchanged), the build counts it, its loader is loud and takes only the product's file name,
and g2048_tpolicy_collect checks every argument before any device call. Nothing here pins the SIZE of EXTRA_ROWS or ALL_ROWS: the
next library is one more row of that table. Also here, on CPU tensors: the rounding of RolloutCollector.sample(as_boards=True)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import PKG, REPO
from test_abi_and_host import declared_symbols
from test_collect_abi_host import FIVE
from test_libraries_abi_host import ENTRY_POINTS, HOST, SIDE, bound, exported

KEY, HEADER, SOURCES = "TPOLICY_COLLECT_", "g2048_tpolicy_collect.h", ["g2048_tpolicy_collect.hip"]
PRODUCT, VARIABLE = "libg2048_tpolicy_collect_hip.so", "G2048_TPOLICY_COLLECT_LIB"
GPU = "tests/test_gpu_tpolicy_collect.py"
SEVEN = set(FIVE) | {"COLLECT_", "PPO_COLLECT_"}
# per entry point the GPU test that puts guard bands round what it writes, or (None, the reason it needs none)
GUARDED_BY = {
    "g2048_tpolicy_collect_last_error": (None, HOST),
    "g2048_tpolicy_collect_abi_version": (None, HOST),
    "g2048_tpolicy_collect": GPU + "::test_guard_bands_round_everything_the_call_writes",
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
    assert set(names) == set(signatures) == set(GUARDED_BY) and len(names) == 3
    hdr = open(os.path.join(REPO, "include", HEADER)).read()
    in_header = int(re.search(r"#define G2048_TPOLICY_COLLECT_ABI_VERSION (\d+)", hdr).group(1))
    assert in_header == 1 == version == built.TPOLICY_COLLECT_ABI_VERSION == loaded.g2048_tpolicy_collect_abi_version()
    assert os.path.basename(path) == PRODUCT and os.path.dirname(path) == os.path.dirname(built.library_path())
    shift = int(re.search(r"#define G2048_TPOLICY_COLLECT_PRECISION_SHIFT (\d+)", hdr).group(1))
    assert shift == built.TPOLICY_COLLECT_PRECISION_SHIFT == built.PPO_COLLECT_PRECISION_SHIFT == 8, "opts are g2048_ppo_collect's"


def test_the_library_shares_no_entry_point_and_the_seven_keep_their_tables(built):
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
    for key, header, count, stem in (("TTRAIN_", "g2048_ttrain.h", 6, "ttrain"), ("COLLECT_", "g2048_collect.h", 4, "collect"),
                                     ("PPO_COLLECT_", "g2048_ppo_collect.h", 3, "ppo_collect")):
        path, signatures, version, loaded = bound(built, key)
        table = exported(path)
        assert table == declared_symbols(header) and set(table) == set(signatures) and len(table) == count
        assert getattr(loaded, "g2048_%s_abi_version" % stem)() == version == 1
        others |= set(table)
    assert not set(built.TPOLICY_COLLECT_SIGNATURES) & others
    # the three pinned tables are as they were, and ROWS is still their union; the fourth holds this row, bound by the same class
    assert set(built.LIBRARIES) == set(_build.LIBRARIES) == set(FIVE) and set(built.EXTENSIONS) == set(_build.EXTENSIONS) == {"COLLECT_"}
    assert set(built.PPO_EXTENSIONS) == set(_build.PPO_EXTENSIONS) == {"PPO_COLLECT_"}
    assert {k: lib.version for k, lib in built.LIBRARIES.items()} == FIVE
    assert set(_build.ROWS) == SEVEN and KEY not in _build.ROWS
    assert set(built.EXTRA_ROWS) == set(_build.EXTRA_ROWS) and KEY in _build.EXTRA_ROWS
    assert _build.ALL_ROWS == {**_build.ROWS, **_build.EXTRA_ROWS} and not set(_build.ROWS) & set(_build.EXTRA_ROWS)
    assert type(built.EXTRA_ROWS[KEY]) is built.Library
    assert built.EXTRA_ROWS[KEY].key == KEY and built.EXTRA_ROWS[KEY].stem == "g2048_tpolicy_collect"


def test_the_build_counts_the_library(built):
    from g2048 import _build
    real = _build.TPOLICY_COLLECT_LIB
    assert os.path.basename(real) == PRODUCT and _build.TPOLICY_COLLECT_SOURCES == SOURCES
    assert _build.EXTRA_ROWS[KEY] == (PRODUCT, VARIABLE, SOURCES, [HEADER])
    elsewhere = sum((r[2] for k, r in _build.ALL_ROWS.items() if k != KEY), [])
    assert not set(SOURCES) & set(elsewhere) and _build.SOURCES == _build.LIBRARIES[""][2]
    assert any(h.endswith(HEADER) for h in _build.PUBLIC_HEADERS)
    assert _build.path_of(KEY) == real
    assert not _build.needs_build()
    products = [_build.path_of(k) for k in _build.ALL_ROWS]
    assert real in products and len(set(products)) == len(products) and all(os.path.exists(p) for p in products)
    before = [os.path.getmtime(p) for p in products]
    try:
        _build.TPOLICY_COLLECT_LIB = os.path.join(os.path.dirname(real), "absent_tpolicy_collect.so")
        assert _build.needs_build(), "needs_build() does not look at the transformer policy's collector library"
    finally:
        _build.TPOLICY_COLLECT_LIB = real
    assert [os.path.getmtime(p) for p in products] == before and not _build.needs_build()
    flags = " ".join(_build.FLAGS)
    assert "-ffp-contract=off" in flags and "g2048_exports.map" in flags, "the same flags and the same version script as the others"


def test_the_tpolicy_collect_switch_builds_the_library_alone(built, tmp_path):
    out = str(tmp_path / "libab_tpolicy_collect.so")
    run = subprocess.run([sys.executable, "-m", "g2048._build", "--tpolicy-collect", "-o", out], cwd=PKG, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.strip().splitlines()[-1] == out and exported(out) == declared_symbols(HEADER)
    assert "g2048_tpolicy_collect.hip" in run.stdout
    assert not any(s in run.stdout for s in ("g2048_tpolicy.hip", "g2048_ppo_collect.hip", "g2048_qnet_collect.hip"))


def test_the_shared_forward_header_adds_no_conditional():
    text = open(os.path.join(PKG, "csrc", "g2048_tpolicy_forward.h")).read()
    assert "#pragma once" in text and not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", text, re.M)
    for name in ("struct Layout", "kWaves", "kLdsFloats", "project64", "add_norm", "dense_lds", "#define TPOLICY_ENCODER_",
                 "#define TPOLICY_DENSE_", "#define TPOLICY_HEADS_"):
        assert name in text, name
    for user in ("g2048_tpolicy.hip", "g2048_tpolicy_collect.hip"):
        source = open(os.path.join(PKG, "csrc", user)).read()
        assert '#include "g2048_tpolicy_forward.h"' in source and "#define TPOLICY_ENCODER_" not in source, user


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
    path = built.tpolicy_collect_library_path()
    code = ("import os, sys; sys.path.insert(0, %r); from g2048 import _build, _lib\n"
            "if os.environ.get('ROW_POINTS_AT'): _build.TPOLICY_COLLECT_LIB = os.environ['ROW_POINTS_AT']\n"
            "try:\n    print('LOADED', _lib.tpolicy_collect_lib().g2048_tpolicy_collect_abi_version())\n"
            "except RuntimeError as e:\n    print('REFUSED', e)\n" % PKG)
    clean = {k: v for k, v in os.environ.items() if k != VARIABLE}
    run = lambda **env: subprocess.run([sys.executable, "-c", code], env=dict(clean, **env), capture_output=True, text=True)  # noqa: E731
    out = run(**{VARIABLE: str(tmp_path / "absent.so")})
    assert "REFUSED" in out.stdout and "is missing" in out.stdout and "no CPU fallback" in out.stdout, out
    assert "no experience collection of the transformer policy in one launch without it" in out.stdout, out
    copy = shutil.copy(path, str(tmp_path / "libab.so"))
    out = run(ROW_POINTS_AT=copy)
    assert "REFUSED g2048: refusing to load %s: only csrc/%s is the " % (copy, PRODUCT) in out.stdout, out
    assert "transformer policy collector library" in out.stdout, out
    assert "LOADED" not in out.stdout and "A/B build" not in out.stderr, out
    out = run(**{VARIABLE: copy})
    assert "LOADED 1" in out.stdout and "loading the A/B build %s (%s is set)" % (copy, VARIABLE) in out.stderr, out


# ---- g2048_tpolicy_collect's argument checks: all of them before any device call, so host memory serves ---------------------------
F64, AUTO, OBS_SHIFT, BF16 = 0x01, 0x02, 4, 1 << 8
GOOD = dict(dim_ff=32, n_layers=1, seed=1, step_index0=0, env_id_base=0, n=8, steps=2, opts=F64 | (2 << OBS_SHIFT) | BF16)
POINTERS = ("boards", "score", "packed", "actions", "prob", "reward", "flags", "value", "obs", "mask", "next_boards", "state_maxcode",
            "counter")
OPTIONAL = ("value", "obs", "mask", "next_boards", "state_maxcode", "counter")
ENTRY = "g2048_tpolicy_collect: "


def collect(lib, base, **changes):
    """The call with GOOD's arguments and every pointer at its own 16-byte aligned place in the host block at `base`, but for
    `changes` (a pointer's name: its new address). Returns (status, message)."""
    a = dict(GOOD, **{name: base + 64 * i for i, name in enumerate(POINTERS)})
    a.update(changes)
    rc = lib.g2048_tpolicy_collect(a["boards"], a["score"], a["packed"], a["dim_ff"], a["n_layers"], a["actions"], a["prob"], a["reward"],
                                   a["flags"], a["value"], a["obs"], a["mask"], a["next_boards"], a["state_maxcode"], a["seed"],
                                   a["step_index0"], a["counter"], a["env_id_base"], a["n"], a["steps"], a["opts"], None)
    return rc, lib.g2048_tpolicy_collect_last_error().decode()


def host_block():
    block = (C.c_uint8 * (64 * len(POINTERS) + 16))()
    return block, (C.addressof(block) + 15) & ~15


REQUIRED = [n for n in POINTERS if n not in OPTIONAL]
SHAPE = "dim_ff must be a multiple of 32 (32 .. 65536) and n_layers 1 .. 64"
REFUSED = [("a null %s pointer" % name, {name: None}, "null pointer") for name in REQUIRED] + [
    ("steps 0", dict(steps=0), "steps must be at least 1"),
    ("negative steps", dict(steps=-3), "steps must be at least 1"),
    ("an unknown opts bit", dict(opts=0x04), "unknown opts 0x4"),
    ("an opts bit above the precision", dict(opts=1 << 12), "unknown opts 0x1000"),
    ("an obs dtype past bf16", dict(opts=3 << OBS_SHIFT), "unknown observation dtype"),
    ("a precision past bf16", dict(opts=2 << 8), "unknown precision"),
    ("dim_ff no multiple of 32", dict(dim_ff=48), SHAPE),
    ("dim_ff 0", dict(dim_ff=0), SHAPE),
    ("dim_ff past the range", dict(dim_ff=65536 + 32), SHAPE),
    ("no layer", dict(n_layers=0), SHAPE),
    ("65 layers", dict(n_layers=65), SHAPE),
    ("more blocks than a grid has", dict(n=16 * 0x7fffffff + 1), "n too large for one launch"),
]


@pytest.mark.parametrize("what,changes,message", REFUSED, ids=[r[0] for r in REFUSED])
def test_arguments_are_checked_without_a_device(built, what, changes, message):
    lib = built.tpolicy_collect_lib()
    block, base = host_block()
    rc, said = collect(lib, base, **changes)
    assert rc == -1 and said.startswith(ENTRY) and message in said, (what, rc, said)
    assert bytes(block) == bytes(len(block)), "a refused call wrote to the arrays it was given"


@pytest.mark.parametrize("name,off,opts", [("boards", 8, None), ("packed", 4, None), ("obs", 8, None), ("next_boards", 1, None),
                                           ("score", 2, None), ("prob", 1, None), ("value", 2, None), ("reward", 4, None), ("reward", 2, BF16),
                                           ("counter", 4, None)])
def test_misaligned_pointers_are_refused(built, name, off, opts):
    lib = built.tpolicy_collect_lib()
    block, base = host_block()
    changes = {name: base + 64 * POINTERS.index(name) + off}
    if opts is not None:
        changes["opts"] = opts
    rc, said = collect(lib, base, **changes)
    assert rc == -1 and ENTRY + "misaligned pointer" in said, (name, rc, said)
    assert bytes(block) == bytes(len(block))


def test_what_is_aligned_enough_passes_the_alignment_check(built):
    """A float32 reward needs 4 bytes only, and the byte arrays none: the call goes on to the next bad argument."""
    lib = built.tpolicy_collect_lib()
    block, base = host_block()
    at = lambda name, off: base + 64 * POINTERS.index(name) + off       # noqa: E731
    rc, said = collect(lib, base, opts=BF16 | AUTO, reward=at("reward", 4), actions=at("actions", 1), flags=at("flags", 3),
                       mask=at("mask", 1), state_maxcode=at("state_maxcode", 5), steps=0)
    assert rc == -1 and "steps must be at least 1" in said
    # every optional pointer absent, the value array among them: the same
    rc, said = collect(lib, base, steps=0, **{name: None for name in OPTIONAL})
    assert rc == -1 and "steps must be at least 1" in said


def test_n_0_does_nothing(built):
    lib = built.tpolicy_collect_lib()
    block, base = host_block()
    # n == 0 returns OK before anything is looked at, null pointers included
    assert collect(lib, base, n=0)[0] == 0
    assert collect(lib, base, n=0, boards=None, steps=0, opts=0xffff, dim_ff=7, n_layers=0)[0] == 0
    assert bytes(block) == bytes(len(block)), "n == 0 wrote to the arrays it was given"


def test_host_layer_fails_loudly_on_cpu(built):
    import torch
    from g2048 import ops
    boards, scores, blob = torch.zeros((4, 16), dtype=torch.uint8), torch.zeros(4, dtype=torch.int32), torch.zeros(1024, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.tpolicy_collect(boards, scores, blob, 32, 1, 2)
    for bad in (dict(steps=0), dict(steps=-1), dict(steps=1, precision="f16")):
        with pytest.raises(ValueError):
            ops.tpolicy_collect(boards, scores, blob, 32, 1, **bad)


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_as_boards_rounds_every_code_back_exactly(dtype):
    """RolloutCollector.sample(as_boards=True) hands DeviceTransformerPolicy.update() round(15 x) of the normalized observations.
    An observation is float32(code) / float32(15), rounded once more to the collector's obs dtype where that is a 16-bit one;
    codes are at most 17 (a 131072 tile). The worst case, bfloat16 at code 17, misses by 17 * 2^-9 = 0.034 < 1 / 2."""
    import torch
    from g2048.rollout import boards_from_observations
    dtype = getattr(torch, dtype)
    codes = torch.arange(18, dtype=torch.uint8)[:, None].expand(18, 16).contiguous()      # (B,16), row c is sixteen cells of code c
    stored = (codes.float() / torch.tensor(15, dtype=torch.float32)).to(dtype)  # what the collector keeps
    got = boards_from_observations(stored)
    assert got.dtype == torch.uint8 and got.shape == codes.shape and torch.equal(got, codes)
    # ... and of the float32 tensor the minibatch gather returns for it (the 16-bit value widened, not rounded again)
    assert torch.equal(boards_from_observations(stored.float()), codes)
    if dtype != torch.float32:
        assert not torch.equal(stored.float(), codes.float() / 15), "the 16-bit observations are rounded once more"
