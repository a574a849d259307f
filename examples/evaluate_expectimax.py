#!/usr/bin/env python3
"""Evaluate the expectimax agent over many complete games on the GPU.

    python examples/evaluate_expectimax.py --games 4096 --depth 2 [--max-moves 5000] [--seed 8264] [--stepwise]
                                           [--out overall_results.json]

Every game is played to the end in one launch (g2048.evaluate_expectimax); --stepwise plays the same games move by move
(expectimax_actions, step, track_episodes per move). Prints the summary table and optionally writes overall_results.json."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2048-using-reinforcement-learning_amd"))
import g2048  # noqa: E402
from g2048.evaluate import save_overall_results  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--games", type=int, default=4096)
ap.add_argument("--depth", type=int, default=2, choices=(1, 2, 3))
ap.add_argument("--max-moves", type=int, default=5000)
ap.add_argument("--seed", type=int, default=0x2048)
ap.add_argument("--stepwise", action="store_true", help="the move-by-move loop instead of the one launch")
ap.add_argument("--out", default=None)
a = ap.parse_args()

res = g2048.evaluate_expectimax(num_games=a.games, depth=a.depth, max_moves=a.max_moves, seed=a.seed, fused=not a.stepwise)
s = res["summary"]
tiles = res["highest_tiles"]
print("==== EXPECTIMAX EVALUATION SUMMARY (depth %d, %s) ====" % (a.depth, "move by move" if a.stepwise else "one launch"))
print("Highest tile reached: %d" % s["highest_tile"])
print("Best score: %d" % s["best_score"])
print("Average score: %.1f" % s["average_score"])
print("Average highest tile: %.1f" % s["average_highest_tile"])
print("Games reaching >= 1024 / 2048 / 4096: %s" % " / ".join("%.1f%%" % (100.0 * sum(1 for x in tiles if x >= t) / max(len(tiles), 1))
                                                              for t in (1024, 2048, 4096)))
print("Hit the %d-move cap: %d" % (a.max_moves, s["hit_move_cap"]))
print("Highest tile distribution:", json.dumps(s["tile_distribution_pct"]))
print("%d games, %d moves, %.3f s  (%.3g games/s, %.3g moves/s)" % (a.games, res["total_moves"], res["elapsed_s"], s["games_per_s"],
                                                                     s["moves_per_s"]))
if a.out:
    print("wrote", save_overall_results(res, a.out))
