"""CPU-side checks of the policy evaluation (g2048_play_policy_games, g2048.evaluate_policy): the C-ABI refuses bad arguments
without touching a device, the Python layer refuses what it cannot run, and the result dict / overall_results.json are
assembled from a per-game table. The games themselves are checked on the GPU (tests/test_gpu_policy_play.py)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from test_policy_host import RefLayout


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    return _lib.lib()


def test_play_policy_games_validates_without_device(lib):
    from g2048 import _lib as L
    assert lib.g2048_play_policy_workspace(0) == lib.g2048_play_policy_workspace(1 << 20) >= 8
    buf = (C.c_uint8 * 1024)()
    a = (C.addressof(buf) + 63) & ~63
    ws = lib.g2048_play_policy_workspace(100)
    masked = L.POLICY_F32 | (L.PLAY_POLICY_MASKED << L.PLAY_POLICY_MODE_SHIFT)

    def call(boards=a, score=a, actor=a, moves=a, valid=a, invalid=a, ms=a, reward=a, alive=a, actions=a, max_moves=10, n=100,
             opts=masked, workspace=a, ws_bytes=ws):
        return lib.g2048_play_policy_games(boards, score, actor, moves, valid, invalid, ms, reward, alive, actions, max_moves, 7, 0,
                                           n, opts, 0, workspace, ws_bytes, None)

    def refused(what, **kw):
        assert call(**kw) == -1 and what in lib.g2048_last_error(), (kw, lib.g2048_last_error())

    assert call(boards=None, score=None, actor=None, n=0) == 0                  # nothing to play
    for k in ("boards", "score", "actor", "moves", "valid", "invalid", "ms", "alive", "workspace"):
        refused(b"null pointer", **{k: None})
    for k, off in (("boards", 8), ("actor", 4), ("ms", 8), ("score", 2), ("moves", 1), ("valid", 2), ("invalid", 2),
                   ("reward", 4), ("workspace", 4)):
        refused(b"misaligned", **{k: a + off})
    refused(b"unknown opts", opts=2)                                            # precision 2
    refused(b"unknown opts", opts=1 << 8)                                       # bits above the mode
    refused(b"unknown mode", opts=3 << L.PLAY_POLICY_MODE_SHIFT)
    refused(b"max_moves", max_moves=0)
    refused(b"max_moves", max_moves=-5)
    refused(b"workspace", ws_bytes=ws - 1)


def test_python_layer_refuses_what_it_cannot_run(lib):
    import g2048
    from g2048 import DevicePolicy, ops
    actor = RefLayout(4).eval()
    with pytest.raises(TypeError, match="DevicePolicy"):
        g2048.evaluate_policy(actor)                       # a bare module, not a DevicePolicy
    with pytest.raises(RuntimeError, match="no CPU path"):
        DevicePolicy(actor)                                # the module lives on the CPU
    cpu = torch.zeros((4, 16), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.play_policy_games(cpu, torch.zeros(4, dtype=torch.int32), torch.zeros(16, dtype=torch.uint8))


def test_policy_result_dict_and_overall_results(tmp_path):
    from g2048 import evaluate as E
    n = 6
    table = np.zeros((n, E.TABLE_COLUMNS), dtype=np.int64)
    table[:, 0] = [300, 1200, 80, 1200, 40, 999]                # scores (a tie: game 1 stays ahead of game 3)
    table[:, 1] = [60, 200, 20, 210, 2000, 150]                 # moves; game 4 hit the cap
    table[:, 2] = table[:, 1] - 3
    table[:, 3] = 3
    table[4, 4] = 1                                             # alive = unfinished
    table[:, 6:14] = -1
    table[1, 6:10] = [30, 70, 120, 190]                         # game 1 reached 512
    table[:, 14:30] = 4
    table[1, 14] = 512
    rewards = np.array([10.25, -3.5, 0.1 + 0.2, 7.0, -1e3, 2.0 ** -30])
    params = {"mode": "masked", "precision": "f32", "max_moves": 2000, "num_games": n, "seed": 11}
    res = E.policy_results_from_table(table, rewards, 0.25, params)
    assert res["best_games"] == [1, 3, 5, 0, 2] and res["best_score"] == 1200 and res["best_game_idx"] == 1
    assert res["unfinished"] == 1 and res["total_moves"] == int(table[:, 1].sum()) and res["total_expansions"] == 0
    assert res["highest_tiles"][1] == 512 and res["milestones"][512] == [190] and res["milestones_by_game"][1][256] == 120
    assert res["parameters"] == params and res["elapsed_s"] == 0.25
    assert res["episode_rewards"] == [float(r) for r in rewards]              # every f64 bit kept
    s = res["summary"]
    assert s["average_episode_reward"] == sum(float(r) for r in rewards) / n and s["games_per_s"] == n / 0.25
    assert s["hit_move_cap"] == 1 and s["best_score"] == 1200
    out = json.load(open(E.save_overall_results(res, str(tmp_path / "overall_results.json"))))
    assert out["parameters"] == params and out["episode_rewards"] == res["episode_rewards"]
    assert out["scores"] == res["scores"] and out["milestones"]["512"] == [190]


def test_beam_overall_results_keep_their_schema(tmp_path):
    """The generalised helpers leave the beam evaluation's dict and file exactly as they were."""
    from g2048 import evaluate as E
    table = np.zeros((3, E.TABLE_COLUMNS), dtype=np.int64)
    table[:, 0] = [5, 7, 6]
    table[:, 6:14] = -1
    res = E.results_from_table(table, 1.0, 20, 30, 7, 5000)
    assert res["parameters"] == {"beam_width": 20, "search_depth": 30, "num_games": 3, "seed": 7, "max_moves": 5000}
    assert "episode_rewards" not in res and "average_episode_reward" not in res["summary"]
    out = json.load(open(E.save_overall_results(res, str(tmp_path / "o.json"))))
    assert list(out) == ["scores", "highest_tiles", "moves", "valid_moves", "invalid_moves", "milestones", "best_games", "parameters"]
    assert out["parameters"] == {"beam_width": 20, "search_depth": 30, "num_games": 3}
