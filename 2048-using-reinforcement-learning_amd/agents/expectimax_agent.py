"""An expectimax player with BeamSearchAgent's surface (agents/beam_search_agent.py): get_action(state, valid_moves) ->
(action, 0.0), no-op remember / update, so a train.py-shaped loop runs on it unchanged. Not in the reference: where the beam
agent samples one spawn per node, this one takes the expectation over all of them (tile 2 with 0.9, tile 4 with 0.1), `depth`
plies deep, with the beam agent's own leaf heuristic. The search runs on the GPU (`g2048_expectimax_actions`, one wavefront per
board); for many games at once use `g2048.BatchedExpectimax` or `g2048.evaluate_expectimax`."""
import numpy as np
import torch

from g2048 import _lib as L
from g2048 import ops


class ExpectimaxAgent:
    def __init__(self, depth=2, device="cuda"):
        if not 1 <= int(depth) <= L.EXPECTIMAX_MAX_DEPTH:
            raise ValueError("ExpectimaxAgent: depth must be 1 .. %d" % L.EXPECTIMAX_MAX_DEPTH)
        self.depth = int(depth)
        self.action_names = {0: "LEFT", 1: "UP", 2: "RIGHT", 3: "DOWN"}
        self.early_game_threshold = 512
        self.mid_game_threshold = 1024
        self.device = torch.device(device)

    def get_action(self, state, valid_moves=None):
        """state: the env's 4x4 tile values. valid_moves: optional four booleans, ANDed with the env's own valid moves. Returns
        (action, 0.0): the second value stands where the learning agents return a log-probability."""
        if self.device.type != "cuda":
            raise RuntimeError("ExpectimaxAgent: needs a ROCm device; there is no CPU path")
        tiles = torch.as_tensor(np.ascontiguousarray(state, dtype=np.int32).reshape(1, 16), device=self.device)
        mask = None
        if valid_moves is not None:
            mask = torch.tensor([sum(int(bool(v)) << a for a, v in enumerate(list(valid_moves)[:4]))], dtype=torch.uint8, device=self.device)
        action = ops.expectimax_actions(ops.pack(tiles), self.depth, mask, False, self.early_game_threshold, self.mid_game_threshold)
        return int(action.item()), 0.0

    def remember(self, *args):
        pass

    def update(self):
        pass
