"""The expectimax agent: decisions per second of g2048_expectimax_actions, and the strength of complete games.

    python3 tools/expectimax_rate.py rates [--rounds 5] [--sizes 4096,65536] [--depths 1,2,3]
    python3 tools/expectimax_rate.py strength --depth 2 [--games 4096] [--max-moves 5000]

rates: per board source, batch size and depth, one ops.expectimax_actions call timed by device events: one warm-up, then the
median of --rounds calls (each call between its own pair of events, a synchronise after every call). The cost of a decision
depends strongly on the number of empty cells (a ply multiplies the tree by 2 x #empty x the valid moves), so the empty-cell
histogram of the boards stands next to each figure. Sources: "synth" = g2048_synth_boards (each cell empty with p = 0.30, codes
up to 11); "move300" = the boards of depth-1 expectimax games after 300 moves (games that ended earlier are left out, the rest
repeated to fill the batch).
strength: g2048.evaluate_expectimax(games, depth) in one launch: average score, the share of games whose highest tile reached
1024 / 2048 / 4096, moves, and the wall time from the reset to the synchronised end.
Output: text (profiles/r38_expectimax_rate.txt keeps a run)."""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import __graft_entry__ as ge  # noqa: E402

g2048 = ge.import_package()
from g2048 import ops  # noqa: E402
from g2048.vec import VecGame2048  # noqa: E402

dev = torch.device("cuda")


def histogram(boards):
    empty = (boards == 0).sum(dim=1)
    counts = torch.bincount(empty, minlength=17).cpu().tolist()
    return " ".join("%d:%.0f%%" % (e, 100.0 * c / boards.shape[0]) for e, c in enumerate(counts) if c), float(empty.float().mean())


def move300_boards(n):
    env = VecGame2048(n, device=dev, seed=0x300)
    r = ops.play_expectimax_games(env.boards, env.scores, 1, 300, seed=0x300)
    live = env.boards[r["alive"].bool()]
    assert live.shape[0] > 0, "no game reached move 300"
    return live.repeat((n + live.shape[0] - 1) // live.shape[0], 1)[:n].contiguous(), live.shape[0]


def time_call(boards, depth, rounds):
    actions = torch.empty(boards.shape[0], dtype=torch.uint8, device=dev)
    ops.expectimax_actions(boards, depth, actions=actions)            # warm-up: the code object, the allocation
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        ops.expectimax_actions(boards, depth, actions=actions)
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms), min(ms), max(ms)


def rates(a):
    sizes, depths = [int(x) for x in a.sizes.split(",")], [int(x) for x in a.depths.split(",")]
    print("# ops.expectimax_actions, one launch per call, device events, median of %d after 1 warm-up (min .. max in brackets)" % a.rounds)
    print("%-8s %7s %5s %12s %22s %14s   %s" % ("boards", "n", "depth", "ms / call", "[min .. max]", "decisions/s", "empty cells (count:share), mean"))
    for source in ("synth", "move300"):
        for n in sizes:
            if source == "synth":
                boards, note = ops.synth_boards(n, seed=0x2048, device=dev), ""
            else:
                boards, live = move300_boards(n)
                note = "  (%d of %d games reached move 300)" % (live, n)
            hist, mean = histogram(boards)
            for depth in depths:
                med, lo, hi = time_call(boards, depth, a.rounds)
                print("%-8s %7d %5d %12.3f %22s %14.4g   %s, mean %.2f%s" % (source, n, depth, med, "[%.3f .. %.3f]" % (lo, hi),
                                                                            n / (med * 1e-3), hist, mean, note))
                sys.stdout.flush()


def strength(a):
    res = g2048.evaluate_expectimax(num_games=a.games, depth=a.depth, max_moves=a.max_moves, seed=0x2048)
    s, tiles, n = res["summary"], res["highest_tiles"], max(a.games, 1)
    share = lambda t: 100.0 * sum(1 for x in tiles if x >= t) / n      # noqa: E731
    print("# g2048.evaluate_expectimax(num_games=%d, depth=%d, max_moves=%d, seed=0x2048), one launch, wall from the reset to the "
          "synchronised end" % (a.games, a.depth, a.max_moves))
    print("depth %d: %d games, average score %.1f, best score %d, highest tile %d" % (a.depth, a.games, s["average_score"], s["best_score"],
                                                                                     s["highest_tile"]))
    print("depth %d: reached >= 1024: %.1f%%   >= 2048: %.1f%%   >= 4096: %.1f%%   hit the move cap: %d" % (
        a.depth, share(1024), share(2048), share(4096), s["hit_move_cap"]))
    print("depth %d: %d moves (%.1f a game, longest %d), wall %.2f s, %.4g moves/s" % (
        a.depth, res["total_moves"], res["total_moves"] / n, max(res["moves"]), res["elapsed_s"], s["moves_per_s"]))
    print("depth %d: highest tile distribution (%%): %s" % (a.depth, s["tile_distribution_pct"]))


ap = argparse.ArgumentParser()
sub = ap.add_subparsers(dest="what", required=True)
p = sub.add_parser("rates")
p.add_argument("--rounds", type=int, default=5)
p.add_argument("--sizes", default="4096,65536")
p.add_argument("--depths", default="1,2,3")
p = sub.add_parser("strength")
p.add_argument("--depth", type=int, required=True)
p.add_argument("--games", type=int, default=4096)
p.add_argument("--max-moves", type=int, default=5000)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU; there is no fallback"
{"rates": rates, "strength": strength}[args.what](args)
