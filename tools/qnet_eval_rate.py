"""Q-network evaluation: complete games, fused (g2048_play_qnet_games, one launch) against the unfused loop of the launches
that exist apart from it (qnet_forward with actions, qnet_select_actions when epsilon > 0, step, track_episodes per move for
the whole batch).

    python3 tools/qnet_eval_rate.py [--fused-only] [--rounds N] [--epsilon E] [--beam] [--sizes N,N,...]

Cases: greedy (epsilon 0 unless --epsilon says otherwise), max_moves 2000, f32 and bf16, the reference's shape (dim_ff 2048, two
layers) on the hash-derived weights of tests/qnet_weights.py, at 4,096, 65,536 and 262,144 games; the last is four times what
the chip holds in flight (65,536 slots), so there the refill matters. Per case the two drivers alternate within each of 5 rounds
after one warm-up round; a run is timed on the wall clock from the reset to the synchronised end (the result tensors stay on
the device); median with min - max. Also: mean and longest game, and the forward FLOP the games needed (tools/qnet_rate.py's
count per board-move) over the fused launch's own time (an event pair around it) as a share of the precision's MFMA peak
(157.3 TF f32, 2.5 PF bf16). Both drivers play the same games (checked here too). "sign": is the slowest fused round faster
than the fastest unfused round.
--fused-only: the fused driver alone, one round unless --rounds says otherwise (for a rocprofv3 --kernel-trace --stats run of the
launch, and for A/B builds of the kernel through G2048_LIB).
--beam: the reference's use_beam_search = True (width 15, depth 30, threshold 64). Per case four drivers alternate within a round:
"beam" (one g2048_play_qnet_beam_games launch), "beam-loop" (its unfused loop: qnet_forward, qnet_beam_actions, step,
track_episodes), "fused" (the games without the search, for the cost of the decision per move) and, at the smallest size only,
"depth1" (the stepwise search_depth 1 loop: 33 boards through the network per board-move), for scale. The beam drivers play the
same games (checked); they are other games than those without the search, so compare moves/s and the launch's own time per
move of its longest game ("us/longest"), not wall times.
--sizes: the game counts, in place of 4096,65536,262144.
Output: one text table."""
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
import qnet_weights as qw  # noqa: E402
from g2048 import DeviceQNetwork, ops  # noqa: E402
from g2048.evaluate import _play_policy_stepwise, qnet_stepwise_act  # noqa: E402
from g2048.vec import VecGame2048  # noqa: E402
from test_qnet_host import RefSpelling  # noqa: E402

PEAK = {"f32": 157.3e12, "bf16": 2.5e15}
FUSED_ONLY = "--fused-only" in sys.argv
ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 1 if FUSED_ONLY else 5
EPSILON = float(sys.argv[sys.argv.index("--epsilon") + 1]) if "--epsilon" in sys.argv else 0.0
BEAM = "--beam" in sys.argv
SEED, CAP, DIM_FF, LAYERS = 0x2048, 2000, 2048, 2
SIZES = tuple(int(x) for x in sys.argv[sys.argv.index("--sizes") + 1].split(",")) if "--sizes" in sys.argv else (4096, 65536, 262144)
REFERENCE_BEAM = (15, 30, 64)
dev = torch.device("cuda")


def flop_per_board(dim_ff=DIM_FF, layers=LAYERS):              # tools/qnet_rate.py
    return 2 * (25 * 32 * 4 + 16 * 64 * 128 + 1024 * 128 + layers * (2 * 128 * 128 + 2 * 128 * dim_ff) + 128 * 4)


def hash_model():
    model = RefSpelling(DIM_FF, LAYERS).double()
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict({k: torch.from_numpy(v) for k, v in qw.state_dict(shapes).items()})
    return model.float().eval().to(dev)


def run(net, n, fused):
    """(wall seconds from the reset to the synchronised end, the fused launch's own seconds or None, result tensors)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    env = VecGame2048(n, device=dev, seed=SEED)
    if fused:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = ops.play_qnet_games(env.boards, env.scores, net.packed, net.dim_ff, net.n_layers, net.precision, CAP, EPSILON, SEED, 0)
        e1.record()
    else:
        act = qnet_stepwise_act(net.packed, net.dim_ff, net.n_layers, net.precision, n, dev, EPSILON, SEED, 0)
        r = _play_policy_stepwise(env, net.packed, net.precision, CAP, None, SEED, 0, act=act)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    r.update(boards=env.boards, scores=env.scores)
    return wall, (e0.elapsed_time(e1) * 1e-3 if fused else None), r


def run_beam(net, n, driver):
    """run() for the drivers of --beam: (wall seconds, the launch's own seconds or None, result tensors)"""
    if driver == "fused":
        return run(net, n, True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    env = VecGame2048(n, device=dev, seed=SEED)
    k = None
    if driver == "beam":
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = ops.play_qnet_beam_games(env.boards, env.scores, net.packed, net.dim_ff, net.n_layers, net.precision, CAP, EPSILON,
                                     *REFERENCE_BEAM, SEED, 0)
        e1.record()
    else:
        beam = REFERENCE_BEAM if driver == "beam-loop" else (REFERENCE_BEAM[0], 1, REFERENCE_BEAM[2])
        act = qnet_stepwise_act(net.packed, net.dim_ff, net.n_layers, net.precision, n, dev, EPSILON, SEED, 0, beam)
        r = _play_policy_stepwise(env, net.packed, net.precision, CAP, None, SEED, 0, act=act)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    r.update(boards=env.boards, scores=env.scores)
    return wall, (e0.elapsed_time(e1) * 1e-3 if driver == "beam" else k), r


def beam_table():
    print("# hybrid Q-network (hash weights, dim_ff %d, %d layers), epsilon %g, max_moves %d, use_beam_search = True (width %d, depth %d, "
          "threshold %d): beam = one g2048_play_qnet_beam_games launch; beam-loop = its unfused loop; fused = g2048_play_qnet_games "
          "(no search); depth1 = the stepwise search_depth 1 loop. Wall from reset to synchronised end, median [min - max] of %d "
          "round(s) after 1 warm-up, the drivers alternating within a round" % ((DIM_FF, LAYERS, EPSILON, CAP) + REFERENCE_BEAM + (ROUNDS,)))
    print("%-5s %-6s %-9s %10s %22s %11s %11s %8s %7s %10s %10s" % (
        "prec", "games", "driver", "wall ms", "[min - max] ms", "games/s", "moves/s", "mean len", "longest", "launch ms", "us/longest"))
    model = hash_model()
    for prec in ("f32", "bf16"):
        net = DeviceQNetwork(model, precision=prec)
        for n in SIZES:
            drivers = ("beam",) if FUSED_ONLY else ("beam-loop", "beam", "fused") + (("depth1",) if n == min(SIZES) else ())
            walls, kernel, last = {d: [] for d in drivers}, {d: [] for d in drivers}, {}
            for rnd in range(ROUNDS + 1):
                for d in drivers:
                    if d == "depth1" and rnd > 1:
                        continue                                            # (one timed round: it is there for scale)
                    wall, k, r = run_beam(net, n, d)
                    last[d] = r
                    if rnd >= 1:
                        walls[d].append(wall)
                        kernel[d].append(k)
            if not FUSED_ONLY:
                for key in ("boards", "scores", "moves", "valid_moves", "invalid_moves", "milestone_move", "alive", "reward_sum"):
                    assert torch.equal(last["beam"][key], last["beam-loop"][key]), key
            for d in drivers:
                w, moves = walls[d], last[d]["moves"]
                med, total, longest = statistics.median(w), int(moves.sum().item()), int(moves.max().item())
                # the launch's own time, and that time per move of the longest game: with every game in a slot from the start (up to
                # 65,536 games) the launch lasts as long as its longest game, so this is what one move of a wavefront costs
                k = statistics.median(kernel[d]) if kernel[d][0] is not None else None
                own = "%10.2f %10.1f" % (k * 1e3, k * 1e6 / longest) if k is not None else "%10s %10s" % ("-", "-")
                print("%-5s %-6d %-9s %10.2f %22s %11.4g %11.4g %8.1f %7d %s" % (
                    prec, n, d, med * 1e3, "[%.2f - %.2f]" % (min(w) * 1e3, max(w) * 1e3), n / med, total / med, total / n, longest, own))
            sys.stdout.flush()


if BEAM:
    beam_table()
    sys.exit(0)

print("# hybrid Q-network (hash weights, dim_ff %d, %d layers), epsilon %g, max_moves %d: fused (one g2048_play_qnet_games launch) vs "
      "unfused (%d launches per move); wall from reset to synchronised end, median [min - max] of %d round(s) after 1 warm-up, the "
      "drivers alternating within a round" % (DIM_FF, LAYERS, EPSILON, CAP, 4 if EPSILON > 0 else 3, ROUNDS))
print("%-5s %-6s %-8s %10s %22s %11s %11s %8s %7s %9s %10s %s" % (
    "prec", "games", "driver", "wall ms", "[min - max] ms", "games/s", "moves/s", "mean len", "longest", "fwd of pk", "vs unfused", "sign"))
model = hash_model()
for prec in ("f32", "bf16"):
    net = DeviceQNetwork(model, precision=prec)
    for n in SIZES:
        drivers = (True,) if FUSED_ONLY else (False, True)
        walls, kernel, last = {f: [] for f in drivers}, [], {}
        for rnd in range(ROUNDS + 1):
            for fused in drivers:
                wall, k, r = run(net, n, fused)
                last[fused] = r
                if rnd >= 1:
                    walls[fused].append(wall)
                    if fused:
                        kernel.append(k)
        if not FUSED_ONLY:
            for key in ("boards", "scores", "moves", "valid_moves", "invalid_moves", "milestone_move", "alive", "reward_sum"):
                assert torch.equal(last[True][key], last[False][key]), key
        moves = last[True]["moves"]
        total, longest = int(moves.sum().item()), int(moves.max().item())
        for fused in drivers:
            w = walls[fused]
            med = statistics.median(w)
            share = ("%8.1f%%" % (100 * total * flop_per_board() / statistics.median(kernel) / PEAK[prec])) if fused else "%9s" % "-"
            gain = ("%9.2fx" % (statistics.median(walls[False]) / med)) if (fused and False in walls) else "%10s" % "-"
            sign = ("faster" if max(w) < min(walls[False]) else "NOT faster") if (fused and False in walls) else "-"
            print("%-5s %-6d %-8s %10.2f %22s %11.4g %11.4g %8.1f %7d %s %s %s" % (
                prec, n, "fused" if fused else "unfused", med * 1e3, "[%.2f - %.2f]" % (min(w) * 1e3, max(w) * 1e3),
                n / med, total / med, total / n, longest, share, gain, sign))
        sys.stdout.flush()
