"""The boundary of the expectimax agent's library (csrc/libg2048_search_hip.so, include/g2048_search.h), a row of the open-ended
library table (g2048._build.EXTRA_ROWS, g2048._lib.EXTRA_ROWS): its export table, its header, its binding table and the inventory
of bounds tests below name the same entry points, no name and no source is shared with another library, the build counts it, and
both entry points check every argument before any device call. Nothing here pins the size of EXTRA_ROWS."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from conftest import PKG, REPO
from test_abi_and_host import declared_symbols
from test_libraries_abi_host import HOST, bound, exported

KEY, HEADER, SOURCES = "SEARCH_", "g2048_search.h", ["g2048_expectimax.hip"]
PRODUCT, VARIABLE = "libg2048_search_hip.so", "G2048_SEARCH_LIB"
GPU, PLAY = "tests/test_gpu_expectimax.py", "tests/test_gpu_expectimax_play.py"
# per entry point the GPU test that puts guard bands round what it writes, or (None, the reason it needs none)
GUARDED_BY = {
    "g2048_search_last_error": (None, HOST),
    "g2048_search_abi_version": (None, HOST),
    "g2048_expectimax_actions": GPU + "::test_guard_bands_and_two_calls_give_the_same_bits",
    "g2048_play_expectimax_workspace": (None, "a size query on the host: it writes no device memory"),
    "g2048_play_expectimax_games": PLAY + "::test_canaries_and_one_move",
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
    assert set(names) == set(signatures) == set(GUARDED_BY) and len(names) == 5
    hdr = open(os.path.join(REPO, "include", HEADER)).read()
    in_header = int(re.search(r"#define G2048_SEARCH_ABI_VERSION (\d+)", hdr).group(1))
    assert in_header == 1 == version == built.SEARCH_ABI_VERSION == loaded.g2048_search_abi_version()
    deepest = int(re.search(r"#define G2048_EXPECTIMAX_MAX_DEPTH (\d+)", hdr).group(1))
    assert deepest == 3 == built.EXPECTIMAX_MAX_DEPTH
    assert os.path.basename(path) == PRODUCT and os.path.dirname(path) == os.path.dirname(built.library_path())


def test_the_library_shares_no_entry_point_and_no_source(built):
    from g2048 import _build
    others = set()
    for key in _build.ALL_ROWS:
        if key != KEY:
            table = exported(_build.path_of(key))
            assert table, key
            others |= set(table)
    assert not set(built.SEARCH_SIGNATURES) & others
    assert exported(built.library_path()) == declared_symbols() and set(exported(built.library_path())) == set(built.SIGNATURES), \
        "the main library's export table moved"
    assert built.lib().g2048_abi_version() == built.ABI_VERSION == 5
    assert _build.EXTRA_ROWS[KEY] == (PRODUCT, VARIABLE, SOURCES, [HEADER]) and KEY not in _build.ROWS
    elsewhere = sum((r[2] for k, r in _build.ALL_ROWS.items() if k != KEY), [])
    assert not set(SOURCES) & set(elsewhere), "the search library's sources are built into another library too"
    assert _build.SEARCH_SOURCES == SOURCES and os.path.basename(_build.SEARCH_LIB) == PRODUCT
    assert any(h.endswith(HEADER) for h in _build.PUBLIC_HEADERS)
    assert set(built.EXTRA_ROWS) == set(_build.EXTRA_ROWS)
    assert type(built.EXTRA_ROWS[KEY]) is built.Library and built.EXTRA_ROWS[KEY].key == KEY and built.EXTRA_ROWS[KEY].stem == "g2048_search"
    # the kernels' file and the shared header are no other source's business, and the header is host-compilable as it stands
    csrc = os.path.join(PKG, "csrc")
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".h")) and f not in ("g2048_expectimax.hip", "g2048_expectimax.h"):
            assert "g2048_expectimax" not in open(os.path.join(csrc, f)).read(), f
    text = open(os.path.join(csrc, "g2048_expectimax.h")).read()
    assert "#pragma once" in text and not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", text, re.M)
    assert "__syncthreads" not in text and "__shared__" not in text and "hip_runtime" not in text


def test_the_build_counts_the_library(built):
    from g2048 import _build
    real = _build.SEARCH_LIB
    assert _build.path_of(KEY) == real and not _build.needs_build()
    try:
        _build.SEARCH_LIB = os.path.join(os.path.dirname(real), "absent_search.so")
        assert _build.needs_build(), "needs_build() does not look at the search library"
    finally:
        _build.SEARCH_LIB = real
    assert not _build.needs_build()


def test_the_search_switch_builds_the_library_alone(built, tmp_path):
    out = str(tmp_path / "libab_search.so")
    run = subprocess.run([sys.executable, "-m", "g2048._build", "--search", "-o", out], cwd=PKG, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout.strip().splitlines()[-1] == out and exported(out) == declared_symbols(HEADER)
    assert "g2048_expectimax.hip" in run.stdout and "g2048_kernels.hip" not in run.stdout and "-ffp-contract=off" in run.stdout


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


# ---- the argument checks: all of them before any device call, so host memory serves ----------------------------------------------
def host_block(slots):
    block = (C.c_uint8 * (64 * slots + 16))()
    return block, (C.addressof(block) + 15) & ~15


ACT = ("boards", "mask", "actions", "values")
ACT_GOOD = dict(depth=2, early=512, mid=1024, n=8)


def actions_call(lib, base, **changes):
    a = dict(ACT_GOOD, **{name: base + 64 * i for i, name in enumerate(ACT)})
    a.update(changes)
    rc = lib.g2048_expectimax_actions(a["boards"], a["mask"], a["actions"], a["values"], a["depth"], a["early"], a["mid"], a["n"], None)
    return rc, lib.g2048_search_last_error().decode()


ACT_REFUSED = [
    ("depth 0", dict(depth=0), "depth must be 1 .. 3"),
    ("depth 4", dict(depth=4), "depth must be 1 .. 3"),
    ("a negative depth", dict(depth=-2), "depth must be 1 .. 3"),
    ("null boards", dict(boards=None), "null pointer"),
    ("null actions", dict(actions=None), "null pointer"),
    ("a negative threshold", dict(mid=-1), "negative threshold"),
    ("more blocks than a grid has", dict(n=4 * 0x7fffffff + 1), "n too large for one launch"),
]


@pytest.mark.parametrize("what,changes,message", ACT_REFUSED, ids=[r[0] for r in ACT_REFUSED])
def test_expectimax_actions_checks_its_arguments_without_a_device(built, what, changes, message):
    lib = built.search_lib()
    block, base = host_block(len(ACT))
    rc, said = actions_call(lib, base, **changes)
    assert rc == -1 and said.startswith("g2048_expectimax_actions: ") and message in said, (what, rc, said)
    assert bytes(block) == bytes(len(block)), "a refused call wrote to the arrays it was given"


@pytest.mark.parametrize("name,off", [("boards", 8), ("boards", 1), ("values", 4), ("values", 1)])
def test_expectimax_actions_refuses_misaligned_pointers(built, name, off):
    lib = built.search_lib()
    block, base = host_block(len(ACT))
    rc, said = actions_call(lib, base, **{name: base + 64 * ACT.index(name) + off})
    assert rc == -1 and "g2048_expectimax_actions: misaligned pointer" in said, (name, rc, said)
    assert bytes(block) == bytes(len(block))


def test_optional_and_byte_pointers_pass_and_n_0_does_nothing(built):
    lib = built.search_lib()
    block, base = host_block(len(ACT))
    # the byte arrays need no alignment and mask and values may be absent: the call goes on to the next bad argument
    rc, said = actions_call(lib, base, mask=None, values=None, actions=base + 64 * 2 + 3, depth=9)
    assert rc == -1 and "depth must be 1 .. 3" in said
    assert actions_call(lib, base, n=0)[0] == 0
    assert actions_call(lib, base, n=0, boards=None, depth=0)[0] == 0, "n == 0 returns before anything is looked at"
    assert bytes(block) == bytes(len(block))


PLAY_PTRS = ("boards", "score", "moves", "valid", "invalid", "milestones", "reward", "alive", "actions", "workspace")
PLAY_GOOD = dict(depth=1, early=512, mid=1024, max_moves=10, seed=1, base=0, n=4, max_waves=0, ws_bytes=64)


def play_call(lib, base, **changes):
    a = dict(PLAY_GOOD, **{name: base + 64 * i for i, name in enumerate(PLAY_PTRS)})
    a.update(changes)
    rc = lib.g2048_play_expectimax_games(a["boards"], a["score"], a["depth"], a["early"], a["mid"], a["moves"], a["valid"], a["invalid"],
                                         a["milestones"], a["reward"], a["alive"], a["actions"], a["max_moves"], a["seed"], a["base"], a["n"],
                                         a["max_waves"], a["workspace"], a["ws_bytes"], None)
    return rc, lib.g2048_search_last_error().decode()


PLAY_REFUSED = [("a null %s pointer" % p, {p: None}, "null pointer") for p in PLAY_PTRS if p not in ("reward", "actions")] + [
    ("depth 0", dict(depth=0), "depth must be 1 .. 3"),
    ("depth 4", dict(depth=4), "depth must be 1 .. 3"),
    ("a negative threshold", dict(early=-5), "negative threshold"),
    ("no move", dict(max_moves=0), "max_moves must be at least 1"),
    ("a workspace too small", dict(ws_bytes=8), "workspace smaller than g2048_play_expectimax_workspace"),
]


@pytest.mark.parametrize("what,changes,message", PLAY_REFUSED, ids=[r[0] for r in PLAY_REFUSED])
def test_play_expectimax_games_checks_its_arguments_without_a_device(built, what, changes, message):
    lib = built.search_lib()
    block, base = host_block(len(PLAY_PTRS))
    rc, said = play_call(lib, base, **changes)
    assert rc == -1 and said.startswith("g2048_play_expectimax_games: ") and message in said, (what, rc, said)
    assert bytes(block) == bytes(len(block)), "a refused call wrote to the arrays it was given"


def test_play_misalignment_workspace_size_and_n_0(built):
    lib = built.search_lib()
    block, base = host_block(len(PLAY_PTRS))
    for name, off in (("boards", 8), ("milestones", 4), ("score", 2), ("reward", 4), ("workspace", 4)):
        rc, said = play_call(lib, base, **{name: base + 64 * PLAY_PTRS.index(name) + off})
        assert rc == -1 and "g2048_play_expectimax_games: misaligned pointer" in said, (name, rc, said)
    assert lib.g2048_play_expectimax_workspace(1) == lib.g2048_play_expectimax_workspace(1 << 20) == 64
    assert play_call(lib, base, n=0, boards=None, depth=0)[0] == 0
    assert bytes(block) == bytes(len(block))


def test_host_layer_fails_loudly_on_cpu_and_checks_depth_first(built):
    import torch
    import g2048
    from g2048 import ops
    boards, scores = torch.zeros((4, 16), dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.expectimax_actions(boards, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.play_expectimax_games(boards, scores, 2)
    for depth in (0, 4):
        with pytest.raises(ValueError, match="depth must be 1 .. 3"):
            g2048.BatchedExpectimax(depth=depth)
        with pytest.raises(ValueError, match="depth must be 1 .. 3"):
            g2048.evaluate_expectimax(num_games=1, depth=depth)
    from agents.expectimax_agent import ExpectimaxAgent
    with pytest.raises(ValueError):
        ExpectimaxAgent(depth=0)
    agent = ExpectimaxAgent(depth=1)
    assert agent.remember(1, 2, 3) is None and agent.update() is None and agent.action_names[3] == "DOWN"
    search = g2048.BatchedExpectimax()
    assert (search.depth, search.early_game_threshold, search.mid_game_threshold) == (2, 512, 1024)
