"""Every entry point of the C-ABI (g2048._lib.SIGNATURES) is listed here with the GPU test that puts sentinels round what it
writes -- guard bands (tests/guard.py) or rows to spare that must survive -- or with the reason why it needs none. A name that
is missing fails this test: the next entry point arrives with its bounds test, or the CPU suite says so."""
import os
import re

from conftest import REPO

ENV, ROLL, PER, BEAM, NETS = ("tests/test_gpu_bounds%s.py" % s for s in ("", "_rollout", "_per", "_beam", "_nets"))
HOST = "a host function: it writes no device memory"
SIZE = "a size query on the host: it writes no device memory"
PLAY = "::test_canaries_and_one_move"

GUARDED_BY = {
    "g2048_last_error": (None, HOST),
    "g2048_abi_version": (None, HOST),
    "g2048_build_flags": (None, HOST),
    "g2048_device_count": (None, HOST),
    "g2048_launch_plan": (None, "host arithmetic into a host array of four words"),
    "g2048_device_plan": (None, "device queries on the host into a host array of six words"),
    "g2048_step_pack": (None, "fills a call block in host memory; the launch is g2048_step_packed's"),
    # the environment
    "g2048_step": "tests/test_gpu_parity.py::test_step_writes_nothing_past_the_last_board",
    "g2048_step_packed": ENV + "::test_step_packed_and_dyn",
    "g2048_step_dyn": ENV + "::test_step_packed_and_dyn",
    "g2048_step_many": ENV + "::test_step_many",
    "g2048_reset": ENV + "::test_reset",
    "g2048_valid_moves": ENV + "::test_valid_moves",
    "g2048_eval": ENV + "::test_evaluate_every_kind_with_and_without_phase",
    "g2048_obs_f32": ENV + "::test_obs",
    "g2048_obs_16": ENV + "::test_obs",
    "g2048_pack_i32": ENV + "::test_pack_and_unpack",
    "g2048_unpack_i32": ENV + "::test_pack_and_unpack",
    "g2048_synth_boards": ENV + "::test_synth_boards_and_actions",
    "g2048_synth_actions": ENV + "::test_synth_boards_and_actions",
    "g2048_metrics": ENV + "::test_metrics_table",
    "g2048_track_episodes": ENV + "::test_track_episodes",
    "g2048_track_episodes_dyn": ENV + "::test_track_episodes",
    "g2048_sample_actions": ENV + "::test_sample_actions",
    "g2048_sample_actions_dyn": ENV + "::test_sample_actions",
    "g2048_simulate_move": ENV + "::test_simulate_move",
    "g2048_simulate_move_sampled": ENV + "::test_simulate_move_sampled",
    "g2048_env_step": ENV + "::test_env_step_record",
    "g2048_replay_games": ENV + "::test_replay_games",
    "g2048_keys_advance": ENV + "::test_keys_advance",
    "g2048_selftest": ENV + "::test_selftest_result_word",
    # the rollout
    "g2048_rollout_step": ROLL + "::test_rollout_step_all_outputs",
    "g2048_minibatch_gather": ROLL + "::test_minibatch_gather",
    "g2048_shaping_scan_workspace": (None, SIZE),
    "g2048_shaping_scan": ROLL + "::test_shaping_chain",
    "g2048_seen_insert": ROLL + "::test_seen_insert_into_the_smallest_table",
    "g2048_seen_rehash": ROLL + "::test_seen_rehash",
    "g2048_shaping_apply": ROLL + "::test_shaping_chain",
    # the prioritized replay
    "g2048_per_update_workspace": (None, SIZE),
    "g2048_per_push": PER + "::test_per_push",
    "g2048_per_sample_workspace": (None, SIZE),
    "g2048_per_sample": PER + "::test_per_sample",
    "g2048_dqn_shape_rewards": PER + "::test_dqn_shape_rewards",
    "g2048_per_update_priorities": PER + "::test_per_update_priorities",
    # the beam search
    "g2048_beam_get_action": BEAM + "::test_beam_get_action",
    "g2048_beam_workspace_bytes": (None, SIZE),
    "g2048_beam_get_action_ws": BEAM + "::test_beam_get_action_with_the_order_scratch",
    "g2048_beam_history_bytes": (None, SIZE),
    "g2048_beam_get_action_hist": BEAM + "::test_beam_get_action_with_the_history",
    "g2048_beam_get_action_dyn": BEAM + "::test_beam_get_action_dyn",
    "g2048_play_games": BEAM + "::test_play_games_with_the_helpers_workspace",
    "g2048_play_games_workspace": (None, SIZE),
    "g2048_play_games_ws": BEAM + "::test_play_games_with_the_helpers_workspace",
    "g2048_play_games_tuned": BEAM + "::test_play_games_with_the_helpers_workspace",
    "g2048_sort_selftest": BEAM + "::test_ranking_network_selftest",
    # the networks
    "g2048_policy_packed_bytes": (None, SIZE),
    "g2048_policy_pack": NETS + "::test_policy_pack",
    "g2048_policy_forward": "tests/test_gpu_policy.py::test_random_weights_ragged_sizes_and_canaries",
    "g2048_tpolicy_packed_bytes": (None, SIZE),
    "g2048_tpolicy_pack": NETS + "::test_encoder_pack",
    "g2048_tpolicy_forward": "tests/test_gpu_tpolicy.py::test_bench_shape_ragged_sizes_and_canaries",
    "g2048_play_policy_workspace": (None, SIZE),
    "g2048_play_policy_games": "tests/test_gpu_policy_play.py" + PLAY,
    "g2048_play_tpolicy_workspace": (None, SIZE),
    "g2048_play_tpolicy_games": "tests/test_gpu_tpolicy_play.py" + PLAY,
    "g2048_qnet_packed_bytes": (None, SIZE),
    "g2048_qnet_pack": NETS + "::test_encoder_pack",
    "g2048_qnet_forward": "tests/test_gpu_qnet.py::test_ragged_sizes_and_canaries",
    "g2048_qnet_select_actions": ENV + "::test_qnet_select_actions",
    "g2048_play_qnet_workspace": (None, SIZE),
    "g2048_play_qnet_games": "tests/test_gpu_qnet_play.py" + PLAY,
    "g2048_qnet_beam_actions": "tests/test_gpu_qnet_beam.py::test_beam_actions_at_depth_30_equal_the_reference",
    "g2048_qnet_beam_expand": ENV + "::test_qnet_beam_expand",
    "g2048_play_qnet_beam_workspace": (None, SIZE),
    "g2048_play_qnet_beam_games": NETS + "::test_qnet_beam_games_canaries_and_one_move",
    "g2048_qnet_batch_workspace": (None, SIZE),
    "g2048_qnet_forward_batch": "tests/test_gpu_qnet_batch.py::test_ragged_sizes_and_canaries",
    "g2048_dqn_targets": ENV + "::test_dqn_targets",
    "g2048_qnet_grad_workspace": (None, SIZE),
    "g2048_qnet_loss_grad": "tests/test_gpu_qnet_grad.py::test_tile_edges_with_canaries",
    "g2048_qnet_step_workspace": (None, SIZE),
    "g2048_qnet_adamw_step": "tests/test_gpu_qnet_step.py::test_three_steps_against_the_yardstick_with_canaries_and_bit_for_bit_twice",
    "g2048_ppo_train_workspace": (None, SIZE),
    "g2048_ppo_forward_train": "tests/test_gpu_ppo_update.py::test_loss_grad_and_forward_train_against_float64",
    "g2048_ppo_advantages": "tests/test_gpu_ppo_update.py::test_advantages_against_float64_torch",
    "g2048_ppo_loss_grad": "tests/test_gpu_ppo_update.py::test_loss_grad_and_forward_train_against_float64",
    "g2048_ppo_forward_train_dropout": "tests/test_gpu_ppo_dropout.py::test_loss_grad_and_forwards_against_float64_with_the_masks",
    "g2048_ppo_loss_grad_dropout": "tests/test_gpu_ppo_dropout.py::test_loss_grad_and_forwards_against_float64_with_the_masks",
    "g2048_ppo_dropout_mask": "tests/test_gpu_ppo_dropout.py::test_masks_equal_the_restatement",
    "g2048_ppo_step_workspace": (None, SIZE),
    "g2048_ppo_adam_step": "tests/test_gpu_ppo_step.py::test_four_steps_against_the_yardstick_with_canaries_and_bit_for_bit_twice",
}


def test_every_entry_point_has_its_bounds_test_or_a_reason():
    from g2048 import _lib
    names = set(_lib.SIGNATURES)
    missing, stale = sorted(names - set(GUARDED_BY)), sorted(set(GUARDED_BY) - names)
    assert not missing, "entry points without a bounds test (add one, then list it in GUARDED_BY): %s" % missing
    assert not stale, "GUARDED_BY lists names that are no entry points: %s" % stale
    for name, where in GUARDED_BY.items():
        if isinstance(where, tuple):
            none, reason = where
            assert none is None and isinstance(reason, str) and len(reason.strip()) > 10 and "\n" not in reason, name
            continue
        path, _, test = where.partition("::")
        full = os.path.join(REPO, path)
        assert os.path.isfile(full), "%s: %s does not exist" % (name, path)
        source = open(full).read()
        assert re.search(r"^def %s\(" % re.escape(test), source, re.M), "%s: %s has no test %s" % (name, path, test)
        assert "pytest.mark.gpu" in source, "%s: %s is no GPU test file" % (name, path)
