"""g2048 -- MI355X-native batched 2048 rollout / beam-search engine (host side).

`ops` holds one tensor-level wrapper per C-ABI entry point (include/g2048.h);
`VecGame2048`, `BatchedBeamSearch` and `BatchedExpectimax` are the batched front-ends; the drop-in
look-alikes of the reference's classes live where the reference keeps them:
`environment.game_2048.Game2048Env` and `agents.beam_search_agent.BeamSearchAgent`
(put this package directory on sys.path instead of the reference checkout).
"""
from . import _lib, ops                      # noqa: F401
from .vec import VecGame2048, BatchedBeamSearch, BatchedExpectimax   # noqa: F401
from .evaluate import evaluate_beam_search, evaluate_beam_search_sharded, evaluate_policy, evaluate_qnet, evaluate_expectimax, save_moveset, save_game_data   # noqa: F401
from .rollout import RolloutCollector, masked_sample  # noqa: F401
from .policy import DevicePolicy  # noqa: F401
from .tpolicy import DeviceTransformerPolicy  # noqa: F401
from .qnet import DeviceQNetwork, dqn_targets, cosine_lr, dqn_epsilon  # noqa: F401
from .replay_buffer import DeviceReplayBuffer  # noqa: F401
from .collector import DQNCollector  # noqa: F401
from .ppo import DevicePPOLearner  # noqa: F401

__all__ = ["ops", "VecGame2048", "BatchedBeamSearch", "BatchedExpectimax", "evaluate_beam_search", "evaluate_beam_search_sharded", "evaluate_policy", "evaluate_qnet", "evaluate_expectimax", "save_moveset",
           "save_game_data", "RolloutCollector", "masked_sample", "DevicePolicy", "DeviceTransformerPolicy", "DeviceQNetwork",
           "DeviceReplayBuffer", "DQNCollector", "DevicePPOLearner", "dqn_targets", "cosine_lr", "dqn_epsilon"]
