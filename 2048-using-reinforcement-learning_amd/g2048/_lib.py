"""ctypes binding of the C-ABI in include/g2048.h (csrc/libg2048_hip.so) and of the four libraries beside it (g2048_train.h,
g2048_tlearn.h, g2048_tstep.h, g2048_ttrain.h): one Library per row of _build.LIBRARIES, each with its own table, error string and version;
and of the extensions libg2048_collect_hip.so (g2048_collect.h), the one row of _build.EXTENSIONS, and libg2048_ppo_collect_hip.so
(g2048_ppo_collect.h), the one row of _build.PPO_EXTENSIONS, bound by the same Library class; and of the rows of _build.EXTRA_ROWS, the
open-ended fourth table: libg2048_tpolicy_collect_hip.so (g2048_tpolicy_collect.h), libg2048_tbf16_hip.so (g2048_tbf16.h) and
libg2048_search_hip.so (g2048_search.h).

There is no fallback: if the library is missing or no HIP device is visible, every
compute call raises. PyTorch is only used for device memory and streams -- tensors
are passed as data_ptr(), work is enqueued on torch's current stream.
"""
import contextlib
import ctypes as C
import os
import sys

import torch

from . import _build

OK = 0
ABI_VERSION = 5
FLAG_DONE, FLAG_VALID, FLAG_MAXCODE_SHIFT = 0x01, 0x02, 3
STEP_REWARD_F64, STEP_AUTO_RESET, STEP_RANDOM_ACTIONS, STEP_NOOP_ACTIONS = 0x01, 0x02, 0x04, 0x08
VALID_ENV, VALID_AGENT = 0, 1
(EVAL_FAST, EVAL_FULL, EVAL_PPO_HEURISTIC, EVAL_MONO_PP, EVAL_MONO_PM, EVAL_MONO_MP, EVAL_MONO_MM, EVAL_PPO_SHAPING, EVAL_PATTERN,
 EVAL_CORNER_BONUS, EVAL_MERGE_POTENTIAL) = range(11)
BEAM_FIXED_DOWN = 0x01
BEAM_RANK_BY_COUNTING = 0x04
PLAY_ONE_PHASE = 0x02
BEAM_MAX_WIDTH = 128
KEYBLOCK_WORDS = 16
STEP_CALL_BYTES = 128
ROLLOUT_OBS_SHIFT, OBS_F32, OBS_F16, OBS_BF16 = 4, 0, 1, 2
SEEN_SLOT_BYTES = 32
ENV_RECORD_BYTES, ENV_OP_STEP, ENV_OP_RESET, ENV_OP_PEEK, ENV_OP_MOVE, ENV_OP_SPAWN, ENV_OP_MOVE_AGENT = 80, 0, 1, 2, 3, 4, 5
ENV_TOKEN_SHIFT = 8
PER_SCAN_TILE = 256
POLICY_F32, POLICY_BF16 = 0, 1
QNET_BATCH_MAX = 4096
QNET_STEP_MAX_PARTIALS = 1024
PPO_BATCH_MAX = 4096
PLAY_POLICY_MASKED, PLAY_POLICY_UNMASKED, PLAY_POLICY_GREEDY, PLAY_POLICY_MODE_SHIFT = 0, 1, 2, 4

_vp, _u64, _sz, _u32, _int = C.c_void_p, C.c_uint64, C.c_size_t, C.c_uint32, C.c_int
SIGNATURES = {
    "g2048_last_error": (C.c_char_p, []),
    "g2048_abi_version": (_int, []),
    "g2048_build_flags": (C.c_uint, []),
    "g2048_device_count": (_int, []),
    "g2048_step": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _sz, _u32, _vp]),
    "g2048_step_pack": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _sz, _u32, _vp]),
    "g2048_step_packed": (_int, [_vp, _u64, _vp]),
    "g2048_step_many": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _u32, _u64, _sz, _u32, _vp]),
    "g2048_reset": (_int, [_vp, _vp, _u64, _u64, _u64, _sz, _vp]),
    "g2048_valid_moves": (_int, [_vp, _vp, _sz, _u32, _vp]),
    "g2048_eval": (_int, [_vp, _int, _vp, _vp, _sz, _vp]),
    "g2048_obs_f32": (_int, [_vp, _vp, _sz, _vp]),
    "g2048_obs_16": (_int, [_vp, _vp, _int, _sz, _vp]),
    "g2048_beam_get_action": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _u64, _u64, _u64, _sz, _u32, _vp]),
    "g2048_beam_workspace_bytes": (_sz, [_sz]),
    "g2048_beam_get_action_ws": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _u64, _u64, _u64, _sz, _u32, _vp, _sz, _vp]),
    "g2048_beam_history_bytes": (_sz, [_sz]),
    "g2048_beam_get_action_hist": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _u64, _u64, _u64, _sz, _u32, _vp, _sz, _u32, _vp]),
    "g2048_track_episodes": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int32, _sz, _vp]),
    "g2048_sample_actions": (_int, [_vp, _vp, _vp, _vp, _u64, _u64, _u64, _sz, _vp]),
    "g2048_simulate_move": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "g2048_simulate_move_sampled": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _u64, _sz, _vp]),
    "g2048_play_games": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _int, _u64, _u64, _sz, _u32, _vp]),
    "g2048_play_games_workspace": (_sz, [_sz]),
    "g2048_play_games_ws": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _int, _u64, _u64, _sz, _u32, _vp,
                                  _sz, _vp]),
    "g2048_play_games_tuned": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _int, _u64, _u64, _sz, _u32,
                                     _vp, _sz, _vp, _vp]),
    "g2048_replay_games": (_int, [_vp, _vp, _vp, _u64, _vp, _sz, _vp, _vp, _vp, _vp, _sz, _u64, _sz, _vp]),
    "g2048_env_step": (_int, [_vp, _vp, _u32, _u32, _vp, _u64, _u64, _u64, _vp]),
    "g2048_minibatch_gather": (_int, [_vp, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _sz, _sz, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _vp]),
    "g2048_launch_plan": (_int, [_int, _int, _sz, _vp]),
    "g2048_device_plan": (_int, [_int, _sz, _vp]),
    "g2048_pack_i32": (_int, [_vp, _vp, _sz, _vp]),
    "g2048_unpack_i32": (_int, [_vp, _vp, _sz, _vp]),
    "g2048_synth_boards": (_int, [_vp, _u64, _u64, _sz, _u32, _u32, _vp]),
    "g2048_synth_actions": (_int, [_vp, _u64, _u64, _u64, _sz, _vp]),
    "g2048_metrics": (_int, [_vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "g2048_keys_advance": (_int, [_vp, _vp, _u64, _vp]),
    "g2048_step_dyn": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _sz, _u32, _vp]),
    "g2048_beam_get_action_dyn": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _int, _int, _int, _vp, _u64, _sz, _u32, _vp]),
    "g2048_sample_actions_dyn": (_int, [_vp, _vp, _vp, _vp, _vp, _u64, _sz, _vp]),
    "g2048_track_episodes_dyn": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "g2048_selftest": (_int, [_vp, _vp]),
    "g2048_sort_selftest": (_int, [_vp, _vp, _sz, _int, _vp]),
    "g2048_rollout_step": (_int, [_vp] * 13 + [_u64, _u64, _vp, _u64, _sz, _u32, _vp]),
    "g2048_shaping_scan_workspace": (_sz, [_sz]),
    "g2048_shaping_scan": (_int, [_vp, _vp, _vp, _vp, _sz, _vp]),
    "g2048_seen_insert": (_int, [_vp, _u64, _vp, _u32, _vp, _vp, _vp, _sz, _vp]),
    "g2048_seen_rehash": (_int, [_vp, _u32, _vp, _u32, _vp, _vp]),
    "g2048_shaping_apply": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _sz, _vp]),
    "g2048_policy_packed_bytes": (_sz, [_int, _int]),
    "g2048_policy_pack": (_int, [_vp, _int, _int, _vp, _vp]),
    "g2048_policy_forward": (_int, [_vp, _vp, _vp, _vp, _vp, _sz, _u32, _vp]),
    "g2048_tpolicy_packed_bytes": (_sz, [_int, _int, _int]),
    "g2048_tpolicy_pack": (_int, [_vp, _int, _int, _int, _vp, _vp]),
    "g2048_tpolicy_forward": (_int, [_vp, _vp, _vp, _vp, _sz, _int, _int, _u32, _vp]),
    "g2048_play_policy_workspace": (_sz, [_sz]),
    "g2048_play_policy_games": (_int, [_vp] * 10 + [_int, _u64, _u64, _sz, _u32, _u32, _vp, _sz, _vp]),
    "g2048_play_tpolicy_workspace": (_sz, [_sz]),
    "g2048_play_tpolicy_games": (_int, [_vp] * 3 + [_int, _int] + [_vp] * 7 + [_int, _u64, _u64, _sz, _u32, _u32, _vp, _sz, _vp]),
    "g2048_qnet_packed_bytes": (_sz, [_int, _int, _int]),
    "g2048_qnet_pack": (_int, [_vp, _int, _int, _int, _vp, _vp]),
    "g2048_qnet_forward": (_int, [_vp, _vp, _vp, _vp, _sz, _int, _int, _u32, _vp]),
    "g2048_qnet_select_actions": (_int, [_vp, _vp, _vp, _vp, C.c_float, _u64, _u64, _u64, _sz, _vp]),
    "g2048_play_qnet_workspace": (_sz, [_sz]),
    "g2048_play_qnet_games": (_int, [_vp] * 3 + [_int, _int] + [_vp] * 7 + [_int, C.c_float, _u64, _u64, _sz, _u32, _u32, _vp, _sz, _vp]),
    "g2048_qnet_beam_actions": (_int, [_vp] * 6 + [_int, _int, _int, C.c_double, C.c_float, _u64, _u64, _u64, _sz, _vp]),
    "g2048_qnet_beam_expand": (_int, [_vp, _vp, _vp, _u64, _u64, _u64, _sz, _vp]),
    "g2048_play_qnet_beam_workspace": (_sz, [_sz]),
    "g2048_play_qnet_beam_games": (_int, [_vp] * 3 + [_int, _int] + [_vp] * 7 +
                                   [_int, C.c_float, _int, _int, _int, _u64, _u64, _sz, _u32, _u32, _vp, _sz, _vp]),
    "g2048_per_update_workspace": (_sz, [_sz]),
    "g2048_per_push": (_int, [_vp] * 6 + [_sz, _sz, _sz] + [_vp] * 4 + [_u32, _vp, _sz, _vp, _vp]),
    "g2048_per_sample_workspace": (_sz, [_sz, _sz]),
    "g2048_per_sample": (_int, [_vp] * 6 + [_sz, _sz, _sz, C.c_float, C.c_float, _sz, _u64, _u64] + [_vp] * 12),
    "g2048_dqn_shape_rewards": (_int, [_vp, _vp, _vp, _sz, _vp, _vp]),
    "g2048_per_update_priorities": (_int, [_vp, _sz, _sz, _sz, _vp, _vp, _sz, _vp, _vp]),
    "g2048_qnet_batch_workspace": (_sz, [_sz, _int]),
    "g2048_qnet_forward_batch": (_int, [_vp, _vp, _vp, _sz, _int, _int, _vp, _vp]),
    "g2048_dqn_targets": (_int, [_vp, _vp, _vp, _vp, C.c_float, _vp, _vp, _sz, _vp]),
    "g2048_qnet_grad_workspace": (_sz, [_sz, _int, _int]),
    "g2048_qnet_loss_grad": (_int, [_vp] * 5 + [_sz, _int, _int] + [_vp] * 6),
    "g2048_qnet_step_workspace": (_sz, [_int, _int]),
    "g2048_qnet_adamw_step": (_int, [_vp] * 4 + [_int, _int] + [C.c_float] * 6 + [_u64, _vp, _vp, _vp]),
    "g2048_ppo_train_workspace": (_sz, [_sz]),
    "g2048_ppo_forward_train": (_int, [_vp, _vp, _vp, _int, _vp, _sz, _vp, _vp]),
    "g2048_ppo_advantages": (_int, [_vp] * 4 + [C.c_float, _vp, _vp, _sz, _vp]),
    "g2048_ppo_loss_grad": (_int, [_vp] * 9 + [C.c_float] * 3 + [_sz] + [_vp] * 5),
    "g2048_ppo_forward_train_dropout": (_int, [_vp, _vp, _vp, _int, _int, C.c_double, _u64, _u64, _vp, _sz, _vp, _vp]),
    "g2048_ppo_loss_grad_dropout": (_int, [_vp] * 9 + [C.c_float] * 3 + [C.c_double] * 2 + [_u64, _u64, _sz] + [_vp] * 5),
    "g2048_ppo_dropout_mask": (_int, [_u64, _u64, _int, _int, C.c_double, _vp, _sz, _vp]),
    "g2048_ppo_step_workspace": (_sz, []),
    "g2048_ppo_adam_step": (_int, [_vp] * 10 + [C.c_float] * 7 + [_vp] * 3),
}


TRAIN_ABI_VERSION = 1
_p4 = C.POINTER(C.c_double)
TRAIN_SIGNATURES = {
    "g2048_train_last_error": (C.c_char_p, []),
    "g2048_train_abi_version": (_int, []),
    "g2048_qnet_train_workspace": (_sz, [_sz, _int, _int]),
    "g2048_qnet_forward_batch_dropout": (_int, [_vp, _vp, _vp, _sz, _int, _int, _p4, _u64, _u64, _vp, _vp]),
    "g2048_qnet_loss_grad_dropout": (_int, [_vp] * 5 + [_sz, _int, _int, _p4, _u64, _u64] + [_vp] * 6),
    "g2048_qnet_dropout_mask": (_int, [_u64, _u64, _int, _int, C.c_double, _sz, _int, _sz, _sz, _vp, _vp]),
}

TLEARN_ABI_VERSION = 1
TLEARN_BATCH_MAX = 1024
_f = C.c_float
TLEARN_SIGNATURES = {
    "g2048_tlearn_last_error": (C.c_char_p, []),
    "g2048_tlearn_abi_version": (_int, []),
    "g2048_tpolicy_grad_workspace": (_sz, [_sz, _int, _int]),
    "g2048_tpolicy_loss_grad": (_int, [_vp] * 6 + [_sz, _int, _int, _f, _f, _f] + [_vp] * 5 + [_sz, _vp]),
}

TSTEP_ABI_VERSION = 1
TSTEP_SIGNATURES = {
    "g2048_tstep_last_error": (C.c_char_p, []),
    "g2048_tstep_abi_version": (_int, []),
    "g2048_tpolicy_step_workspace": (_sz, [_int, _int]),
    "g2048_tpolicy_adam_step": (_int, [_vp] * 4 + [_int, _int, _vp, _vp] + [_f] * 5 + [_vp, _vp, _sz, _vp]),
}

TTRAIN_ABI_VERSION = 1
TTRAIN_SIGNATURES = {
    "g2048_ttrain_last_error": (C.c_char_p, []),
    "g2048_ttrain_abi_version": (_int, []),
    "g2048_tpolicy_train_workspace": (_sz, [_sz, _int, _int]),
    "g2048_tpolicy_loss_grad_dropout": (_int, [_vp] * 6 + [_sz, _int, _int, _p4, _u64, _u64, _f, _f, _f] + [_vp] * 5 + [_sz, _vp]),
    "g2048_tpolicy_forward_dropout": (_int, [_vp, _vp, _sz, _int, _int, _p4, _u64, _u64, _vp, _vp, _vp, _sz, _vp]),
    "g2048_tpolicy_dropout_mask": (_int, [_u64, _u64, _int, _int, C.c_double, _sz, _int, _sz, _sz, _vp, _vp]),
}

COLLECT_ABI_VERSION = 1
COLLECT_SIGNATURES = {
    "g2048_collect_last_error": (C.c_char_p, []),
    "g2048_collect_abi_version": (_int, []),
    "g2048_qnet_collect_workspace": (_sz, [_sz]),
    "g2048_qnet_collect": (_int, [_vp] * 4 + [_int, _int, _u32, _f, _int, _int, _int, _u64, _u64, _u64, _sz, _int, _int] + [_vp] * 6 +
                           [_sz, _sz, _sz, _vp, _vp, _vp]),
}

PPO_COLLECT_ABI_VERSION = 1
PPO_COLLECT_PRECISION_SHIFT = 8
PPO_COLLECT_SIGNATURES = {
    "g2048_ppo_collect_last_error": (C.c_char_p, []),
    "g2048_ppo_collect_abi_version": (_int, []),
    "g2048_ppo_collect": (_int, [_vp] * 13 + [_u64, _u64, _vp, _u64, _sz, _int, _u32, _vp]),
}

TPOLICY_COLLECT_ABI_VERSION = 1
TPOLICY_COLLECT_PRECISION_SHIFT = 8
TPOLICY_COLLECT_SIGNATURES = {
    "g2048_tpolicy_collect_last_error": (C.c_char_p, []),
    "g2048_tpolicy_collect_abi_version": (_int, []),
    "g2048_tpolicy_collect": (_int, [_vp] * 3 + [_int, _int] + [_vp] * 9 + [_u64, _u64, _vp, _u64, _sz, _int, _u32, _vp]),
}

TBF16_ABI_VERSION = 1
TBF16_SIGNATURES = {
    "g2048_tbf16_last_error": (C.c_char_p, []),
    "g2048_tbf16_abi_version": (_int, []),
    "g2048_tpolicy_bf16_workspace": (_sz, [_sz, _int, _int]),
    "g2048_tpolicy_loss_grad_bf16": (_int, [_vp] * 6 + [_sz, _int, _int, _p4, _u64, _u64, _f, _f, _f] + [_vp] * 5 + [_sz, _vp]),
    # the header's testing section: the three products on their own
    "g2048_tbf16_test_linear": (_int, [_vp, _int, _vp, _vp, _vp, _vp, _int, _int, _sz, _int, _int, _vp, _sz, _vp]),
    "g2048_tbf16_test_dx": (_int, [_vp, _int, _vp, _vp, _vp, _vp, _int, _sz, _int, _int, _vp, _sz, _vp]),
    "g2048_tbf16_test_dw": (_int, [_vp, _int, _vp, _int, _vp, _vp, _sz, _int, _int, _vp, _sz, _vp]),
}

SEARCH_ABI_VERSION = 1
EXPECTIMAX_MAX_DEPTH = 3
SEARCH_SIGNATURES = {
    "g2048_search_last_error": (C.c_char_p, []),
    "g2048_search_abi_version": (_int, []),
    "g2048_expectimax_actions": (_int, [_vp, _vp, _vp, _vp, _int, _int, _int, _sz, _vp]),
    "g2048_play_expectimax_workspace": (_sz, [_sz]),
    "g2048_play_expectimax_games": (_int, [_vp, _vp, _int, _int, _int] + [_vp] * 7 + [_int, _u64, _u64, _sz, _u32, _vp, _sz, _vp]),
}


class Library:
    """One shared object of _build.ALL_ROWS (row `key`, of whichever table), loaded on first use and as loud as can be: a missing file, a file under
    another name than the product's, a missing symbol, another ABI version and a failed call all raise."""

    def __init__(self, key, stem, signatures, version, role="", without="", after_load=None):
        """stem: the library exports <stem>_abi_version and <stem>_last_error. role: what the messages call the library beside the
        main one ("training"); without: what the `missing` message says is lost with it. after_load(handle, path): a last check."""
        self.key, self.stem, self.signatures, self.version = key, stem, signatures, version
        self.role, self.without, self.after_load = role, without, after_load
        self.handle = None

    def path(self):
        return _build.path_of(self.key)

    def load(self):
        """The loaded library. Raises if it has not been built (python __graft_entry__.py)."""
        if self.handle is None:
            path, (product, env) = self.path(), _build.ALL_ROWS[self.key][:2]
            if not os.path.exists(path):
                raise RuntimeError("g2048: %s is missing -- build it with `python __graft_entry__.py` "
                                   "(hipcc --offload-arch=gfx950); there is no CPU fallback%s" % (path, self.without))
            if os.environ.get(env):      # A/B builds (tools/build_ab.sh) are only ever loaded on request, and say so
                print("g2048: loading the A/B build %s (%s is set)" % (path, env), file=sys.stderr)
            elif os.path.basename(path) != product:
                raise RuntimeError("g2048: refusing to load %s: only csrc/%s is the product%s library"
                                   % (path, product, self.role and "'s " + self.role))
            handle = C.CDLL(path)       # torch is imported above, so libamdhip64 resolves to the runtime torch uses
            for name, (res, args) in self.signatures.items():
                fn = getattr(handle, name)   # AttributeError here = ABI mismatch, deliberately loud
                fn.restype, fn.argtypes = res, args
            found = getattr(handle, self.stem + "_abi_version")()
            if found != self.version:
                raise RuntimeError("g2048: %sABI version mismatch (library %d, binding %d)"
                                   % (self.role and self.role + " library ", found, self.version))
            if self.after_load:
                self.after_load(handle, path)
            self.handle = handle
        return self.handle

    def check(self, rc):
        if rc != OK:
            raise RuntimeError("g2048: %s (status %d)" % (getattr(self.load(), self.stem + "_last_error")().decode(), rc))

    def call(self, device, fn, *args):
        """Invoke an entry point with `device` as the calling thread's current HIP device (a launch goes to the current device,
        which need not be the tensors' device in a one-process multi-GPU program) and check its status against this library's
        own error string."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if torch.cuda.current_device() == idx:
            rc = fn(*args)
        else:
            with torch.cuda.device(idx):
                rc = fn(*args)
        self.check(rc)

    @contextlib.contextmanager
    def swapped(self, handle):
        """Every call of the package goes to `handle`, another build bound like this one, until the block ends (tools/)."""
        mine, self.handle = self.load(), handle
        try:
            yield
        finally:
            self.handle = mine


def _refuse_instrumented(handle, path):
    flags = int(handle.g2048_build_flags())
    if flags and os.environ.get("G2048_ALLOW_INSTRUMENTED") != "1":
        # a measurement build (csrc/g2048_instrument.h) overwrites real outputs with clock ticks: only the timeline tools,
        # which set G2048_ALLOW_INSTRUMENTED=1 themselves, may load one
        raise RuntimeError("g2048: %s is an instrumented measurement build (g2048_build_flags() = 0x%x); its outputs are "
                           "not results -- refusing to load it (tools/*_timeline.py opt in with G2048_ALLOW_INSTRUMENTED=1)"
                           % (path, flags))


MAIN = Library("", "g2048", SIGNATURES, ABI_VERSION, after_load=_refuse_instrumented)
TRAIN = Library("TRAIN_", "g2048_train", TRAIN_SIGNATURES, TRAIN_ABI_VERSION, "training", " and no training pass without it")
TLEARN = Library("TLEARN_", "g2048_tlearn", TLEARN_SIGNATURES, TLEARN_ABI_VERSION, "learner", " and no gradient pass without it")
TSTEP = Library("TSTEP_", "g2048_tstep", TSTEP_SIGNATURES, TSTEP_ABI_VERSION, "step", " and no device optimiser step without it")
TTRAIN = Library("TTRAIN_", "g2048_ttrain", TTRAIN_SIGNATURES, TTRAIN_ABI_VERSION, "policy training",
                 " and no training-mode pass of the transformer policy without it")
LIBRARIES = {"": MAIN, "TRAIN_": TRAIN, "TLEARN_": TLEARN, "TSTEP_": TSTEP, "TTRAIN_": TTRAIN}
# the second table (_build.EXTENSIONS has the reason for the split): the same class, bound the same way
COLLECT = Library("COLLECT_", "g2048_collect", COLLECT_SIGNATURES, COLLECT_ABI_VERSION, "collector",
                  " and no experience collection in one launch without it")
EXTENSIONS = {"COLLECT_": COLLECT}
# the third table (_build.PPO_EXTENSIONS), for the same reason
PPO_COLLECT = Library("PPO_COLLECT_", "g2048_ppo_collect", PPO_COLLECT_SIGNATURES, PPO_COLLECT_ABI_VERSION, "PPO collector",
                      " and no PPO experience collection in one launch without it")
PPO_EXTENSIONS = {"PPO_COLLECT_": PPO_COLLECT}
# the fourth table (_build.EXTRA_ROWS): no test pins its size, so the next library is one more row here
TPOLICY_COLLECT = Library("TPOLICY_COLLECT_", "g2048_tpolicy_collect", TPOLICY_COLLECT_SIGNATURES, TPOLICY_COLLECT_ABI_VERSION,
                          "transformer policy collector", " and no experience collection of the transformer policy in one launch without it")
TBF16 = Library("TBF16_", "g2048_tbf16", TBF16_SIGNATURES, TBF16_ABI_VERSION, "bf16 learner",
                " and no bf16 gradient pass of the transformer policy without it")
SEARCH = Library("SEARCH_", "g2048_search", SEARCH_SIGNATURES, SEARCH_ABI_VERSION, "search", " and no expectimax agent without it")
EXTRA_ROWS = {"TPOLICY_COLLECT_": TPOLICY_COLLECT, "TBF16_": TBF16, "SEARCH_": SEARCH}

# the names the package, the tools and the tests call
library_path, lib, check, call = MAIN.path, MAIN.load, MAIN.check, MAIN.call
train_library_path, train_lib, train_call = TRAIN.path, TRAIN.load, TRAIN.call
tlearn_library_path, tlearn_lib, tlearn_call = TLEARN.path, TLEARN.load, TLEARN.call
tstep_library_path, tstep_lib, tstep_call = TSTEP.path, TSTEP.load, TSTEP.call
ttrain_library_path, ttrain_lib, ttrain_call = TTRAIN.path, TTRAIN.load, TTRAIN.call
collect_library_path, collect_lib, collect_call = COLLECT.path, COLLECT.load, COLLECT.call
ppo_collect_library_path, ppo_collect_lib, ppo_collect_call = PPO_COLLECT.path, PPO_COLLECT.load, PPO_COLLECT.call
tpolicy_collect_library_path, tpolicy_collect_lib, tpolicy_collect_call = TPOLICY_COLLECT.path, TPOLICY_COLLECT.load, TPOLICY_COLLECT.call
tbf16_library_path, tbf16_lib, tbf16_call = TBF16.path, TBF16.load, TBF16.call
search_library_path, search_lib, search_call = SEARCH.path, SEARCH.load, SEARCH.call


def stream_ptr(device):
    return torch.cuda.current_stream(device).cuda_stream


def require_device_tensor(t, dtype, shape_tail=None, name="tensor"):
    if not isinstance(t, torch.Tensor):
        raise TypeError("g2048: %s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("g2048: %s must live on a ROCm device (got %s); there is no CPU path" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("g2048: %s must be %s (got %s)" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("g2048: %s must be contiguous" % name)
    if shape_tail is not None and tuple(t.shape[1:]) != tuple(shape_tail):
        raise ValueError("g2048: %s must have shape (n,%s) (got %s)" % (name, ",".join(map(str, shape_tail)), tuple(t.shape)))
    return t


def u64(x):
    return int(x) & 0xFFFFFFFFFFFFFFFF
