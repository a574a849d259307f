"""Policy evaluation: complete games of a PPO actor, fused (g2048_play_policy_games, one launch) against the unfused loop of
existing launches (policy_forward, valid_moves, sample_actions, step, track_episodes per move for the whole batch).

    python3 tools/policy_eval_rate.py [--fused-only]

Cases: 4,096 and 65,536 games, f32 and bf16, masked mode (train.py's games), max_moves 2000, the reference checkpoint of
tests/golden/policy.npz and random weights (the reference layout, default init). Per case and driver: wall time of the whole
evaluation from the reset to the synchronised end (median of 3 after one warm-up run), games/s, moves/s, mean and longest
game, and the forward FLOP the games needed (92,160 per board-move, layer 4 padded to 16 outputs) over that wall time as a
share of the MFMA peak of the precision (157.3 TF f32, 2.5 PF bf16). Both drivers play the same games (checked here too).
--fused-only: one run of each fused case (for a rocprofv3 --kernel-trace --stats run of the launch).
Output: one text table (profiles/r07_policy_eval_rate.txt keeps a run)."""
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import __graft_entry__ as ge  # noqa: E402

ge.import_package()
from g2048 import DevicePolicy, evaluate_policy  # noqa: E402
from test_policy_host import RefLayout, golden_modules  # noqa: E402

FLOP_PER_BOARD = 2 * (16 * 256 + 256 * 128 + 128 * 64 + 64 * 16)
PEAK = {"f32": 157.3e12, "bf16": 2.5e15}
FUSED_ONLY = "--fused-only" in sys.argv
dev = torch.device("cuda")


def actors():
    torch.manual_seed(0)
    return (("reference", golden_modules()[1].to(dev)), ("random", RefLayout(4).eval().to(dev)))


def run(pol, n, fused):
    r = evaluate_policy(pol, num_games=n, max_moves=2000, mode="masked", seed=0x2048, fused=fused)
    return r, r["elapsed_s"]


print("# evaluate_policy, masked mode, max_moves 2000: fused (one g2048_play_policy_games launch) vs unfused (five launches per"
      " move); wall from reset to synchronised end, median of %d after 1 warm-up" % (1 if FUSED_ONLY else 3))
print("%-9s %-5s %-7s %-8s %10s %12s %12s %8s %7s %9s %9s" % ("weights", "prec", "games", "driver", "wall ms", "games/s",
                                                            "moves/s", "mean len", "longest", "fwd of pk", "vs unfused"))
for name, actor in actors():
    for prec in ("f32", "bf16"):
        pol = DevicePolicy(actor, precision=prec)
        for n in (4096, 65536):
            rows = {}
            for fused in ((True,) if FUSED_ONLY else (False, True)):
                res, _ = run(pol, n, fused)                       # warm-up (code objects, allocations)
                walls = [res["elapsed_s"]] if FUSED_ONLY else []
                for _ in range(0 if FUSED_ONLY else 3):
                    res, dt = run(pol, n, fused)
                    walls.append(dt)
                rows[fused] = (res, statistics.median(walls))
            if not FUSED_ONLY:
                assert rows[True][0]["scores"] == rows[False][0]["scores"] and rows[True][0]["moves"] == rows[False][0]["moves"]
            for fused, (res, wall) in sorted(rows.items()):
                moves = res["total_moves"]
                share = moves * FLOP_PER_BOARD / wall / PEAK[prec]
                gain = ("%8.2fx" % (rows[False][1] / wall)) if (fused and False in rows) else "%9s" % "-"
                print("%-9s %-5s %-7d %-8s %10.2f %12.4g %12.4g %8.1f %7d %8.1f%% %s" % (
                    name, prec, n, "fused" if fused else "unfused", wall * 1e3, n / wall, moves / wall, moves / n,
                    max(res["moves"]), 100 * share, gain))
            sys.stdout.flush()
