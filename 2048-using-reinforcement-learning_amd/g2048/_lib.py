"""ctypes binding of the C-ABI in include/g2048.h (csrc/libg2048_hip.so).

There is no fallback: if the library is missing or no HIP device is visible, every
compute call raises. PyTorch is only used for device memory and streams -- tensors
are passed as data_ptr(), work is enqueued on torch's current stream.
"""
import ctypes as C
import os

import torch

from . import _build

_lib = None

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


def library_path():
    return _build.LIB


def lib():
    """The loaded C-ABI library. Raises if it has not been built (python __graft_entry__.py)."""
    global _lib
    if _lib is None:
        path = library_path()
        if not os.path.exists(path):
            raise RuntimeError("g2048: %s is missing -- build it with `python __graft_entry__.py` "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
        if os.environ.get("G2048_LIB"):      # A/B builds (tools/build_ab.sh) are only ever loaded on request, and say so
            import sys
            print("g2048: loading the A/B build %s (G2048_LIB is set)" % path, file=sys.stderr)
        elif os.path.basename(path) != "libg2048_hip.so":
            raise RuntimeError("g2048: refusing to load %s: only csrc/libg2048_hip.so is the product library" % path)
        L = C.CDLL(path)        # torch is imported above, so libamdhip64 resolves to the runtime torch uses
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)   # AttributeError here = ABI mismatch, deliberately loud
            fn.restype, fn.argtypes = res, args
        if L.g2048_abi_version() != ABI_VERSION:
            raise RuntimeError("g2048: ABI version mismatch (library %d, binding %d)" % (L.g2048_abi_version(), ABI_VERSION))
        flags = int(L.g2048_build_flags())
        if flags and os.environ.get("G2048_ALLOW_INSTRUMENTED") != "1":
            # a measurement build (csrc/g2048_instrument.h) overwrites real outputs with clock ticks: only the timeline tools,
            # which set G2048_ALLOW_INSTRUMENTED=1 themselves, may load one
            raise RuntimeError("g2048: %s is an instrumented measurement build (g2048_build_flags() = 0x%x); its outputs are "
                               "not results -- refusing to load it (tools/*_timeline.py opt in with G2048_ALLOW_INSTRUMENTED=1)"
                               % (path, flags))
        _lib = L
    return _lib


def check(rc):
    if rc != OK:
        raise RuntimeError("g2048: %s (status %d)" % (lib().g2048_last_error().decode(), rc))


# ---- the training library (include/g2048_train.h, csrc/libg2048_train_hip.so): its own table, loader, error string and version
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
_train_lib = None


def train_library_path():
    return _build.TRAIN_LIB


def train_lib():
    """The loaded training library. Raises if it has not been built (python __graft_entry__.py); as loud as lib()."""
    global _train_lib
    if _train_lib is None:
        path = train_library_path()
        if not os.path.exists(path):
            raise RuntimeError("g2048: %s is missing -- build it with `python __graft_entry__.py` "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback and no training pass without it" % path)
        if os.environ.get("G2048_TRAIN_LIB"):      # A/B builds are only ever loaded on request, and say so
            import sys
            print("g2048: loading the A/B build %s (G2048_TRAIN_LIB is set)" % path, file=sys.stderr)
        elif os.path.basename(path) != "libg2048_train_hip.so":
            raise RuntimeError("g2048: refusing to load %s: only csrc/libg2048_train_hip.so is the product's training library" % path)
        T = C.CDLL(path)
        for name, (res, args) in TRAIN_SIGNATURES.items():
            fn = getattr(T, name)   # AttributeError here = ABI mismatch, deliberately loud
            fn.restype, fn.argtypes = res, args
        if T.g2048_train_abi_version() != TRAIN_ABI_VERSION:
            raise RuntimeError("g2048: training library ABI version mismatch (library %d, binding %d)"
                               % (T.g2048_train_abi_version(), TRAIN_ABI_VERSION))
        _train_lib = T
    return _train_lib


def train_check(rc):
    if rc != OK:
        raise RuntimeError("g2048: %s (status %d)" % (train_lib().g2048_train_last_error().decode(), rc))


def train_call(device, fn, *args):
    """call() for an entry point of the training library: its status is read from that library's own error string."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if torch.cuda.current_device() == idx:
        rc = fn(*args)
    else:
        with torch.cuda.device(idx):
            rc = fn(*args)
    train_check(rc)


# ---- the transformer policy's learner library (include/g2048_tlearn.h, csrc/libg2048_tlearn_hip.so): again its own table, loader,
# error string and version
TLEARN_ABI_VERSION = 1
TLEARN_BATCH_MAX = 1024
_f = C.c_float
TLEARN_SIGNATURES = {
    "g2048_tlearn_last_error": (C.c_char_p, []),
    "g2048_tlearn_abi_version": (_int, []),
    "g2048_tpolicy_grad_workspace": (_sz, [_sz, _int, _int]),
    "g2048_tpolicy_loss_grad": (_int, [_vp] * 6 + [_sz, _int, _int, _f, _f, _f] + [_vp] * 5 + [_sz, _vp]),
}
_tlearn_lib = None


def tlearn_library_path():
    return _build.TLEARN_LIB


def tlearn_lib():
    """The loaded learner library of the transformer policy. Raises if it has not been built (python __graft_entry__.py); as loud
    as train_lib()."""
    global _tlearn_lib
    if _tlearn_lib is None:
        path = tlearn_library_path()
        if not os.path.exists(path):
            raise RuntimeError("g2048: %s is missing -- build it with `python __graft_entry__.py` "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback and no gradient pass without it" % path)
        if os.environ.get("G2048_TLEARN_LIB"):      # A/B builds are only ever loaded on request, and say so
            import sys
            print("g2048: loading the A/B build %s (G2048_TLEARN_LIB is set)" % path, file=sys.stderr)
        elif os.path.basename(path) != "libg2048_tlearn_hip.so":
            raise RuntimeError("g2048: refusing to load %s: only csrc/libg2048_tlearn_hip.so is the product's learner library" % path)
        T = C.CDLL(path)
        for name, (res, args) in TLEARN_SIGNATURES.items():
            fn = getattr(T, name)   # AttributeError here = ABI mismatch, deliberately loud
            fn.restype, fn.argtypes = res, args
        if T.g2048_tlearn_abi_version() != TLEARN_ABI_VERSION:
            raise RuntimeError("g2048: learner library ABI version mismatch (library %d, binding %d)"
                               % (T.g2048_tlearn_abi_version(), TLEARN_ABI_VERSION))
        _tlearn_lib = T
    return _tlearn_lib


def tlearn_call(device, fn, *args):
    """call() for an entry point of the learner library: its status is read from that library's own error string."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if torch.cuda.current_device() == idx:
        rc = fn(*args)
    else:
        with torch.cuda.device(idx):
            rc = fn(*args)
    if rc != OK:
        raise RuntimeError("g2048: %s (status %d)" % (tlearn_lib().g2048_tlearn_last_error().decode(), rc))


# ---- the transformer policy's optimiser-step library (include/g2048_tstep.h, csrc/libg2048_tstep_hip.so): the fourth table, loader,
# error string and version
TSTEP_ABI_VERSION = 1
TSTEP_SIGNATURES = {
    "g2048_tstep_last_error": (C.c_char_p, []),
    "g2048_tstep_abi_version": (_int, []),
    "g2048_tpolicy_step_workspace": (_sz, [_int, _int]),
    "g2048_tpolicy_adam_step": (_int, [_vp] * 4 + [_int, _int, _vp, _vp] + [_f] * 5 + [_vp, _vp, _sz, _vp]),
}
_tstep_lib = None


def tstep_library_path():
    return _build.TSTEP_LIB


def tstep_lib():
    """The loaded optimiser-step library of the transformer policy. Raises if it has not been built (python __graft_entry__.py); as
    loud as tlearn_lib()."""
    global _tstep_lib
    if _tstep_lib is None:
        path = tstep_library_path()
        if not os.path.exists(path):
            raise RuntimeError("g2048: %s is missing -- build it with `python __graft_entry__.py` "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback and no device optimiser step without it" % path)
        if os.environ.get("G2048_TSTEP_LIB"):      # A/B builds are only ever loaded on request, and say so
            import sys
            print("g2048: loading the A/B build %s (G2048_TSTEP_LIB is set)" % path, file=sys.stderr)
        elif os.path.basename(path) != "libg2048_tstep_hip.so":
            raise RuntimeError("g2048: refusing to load %s: only csrc/libg2048_tstep_hip.so is the product's step library" % path)
        T = C.CDLL(path)
        for name, (res, args) in TSTEP_SIGNATURES.items():
            fn = getattr(T, name)   # AttributeError here = ABI mismatch, deliberately loud
            fn.restype, fn.argtypes = res, args
        if T.g2048_tstep_abi_version() != TSTEP_ABI_VERSION:
            raise RuntimeError("g2048: step library ABI version mismatch (library %d, binding %d)"
                               % (T.g2048_tstep_abi_version(), TSTEP_ABI_VERSION))
        _tstep_lib = T
    return _tstep_lib


def tstep_call(device, fn, *args):
    """call() for an entry point of the step library: its status is read from that library's own error string."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if torch.cuda.current_device() == idx:
        rc = fn(*args)
    else:
        with torch.cuda.device(idx):
            rc = fn(*args)
    if rc != OK:
        raise RuntimeError("g2048: %s (status %d)" % (tstep_lib().g2048_tstep_last_error().decode(), rc))


def stream_ptr(device):
    return torch.cuda.current_stream(device).cuda_stream


def call(device, fn, *args):
    """Invoke a C-ABI entry point with `device` as the calling thread's current HIP device (a launch goes to the
    current device, which need not be the tensors' device in a one-process multi-GPU program) and check its status."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if torch.cuda.current_device() == idx:
        rc = fn(*args)
    else:
        with torch.cuda.device(idx):
            rc = fn(*args)
    check(rc)


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
