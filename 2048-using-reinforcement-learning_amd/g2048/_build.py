"""Builds csrc/libg2048_hip.so, csrc/libg2048_train_hip.so, csrc/libg2048_tlearn_hip.so, csrc/libg2048_tstep_hip.so and
csrc/libg2048_ttrain_hip.so, and the extensions csrc/libg2048_collect_hip.so, csrc/libg2048_ppo_collect_hip.so and
csrc/libg2048_tpolicy_collect_hip.so, for gfx950 with hipcc (cross-compiles without a GPU).

    python -m g2048._build [-o LIBRARY] [extra compiler flags ...]           (from the package directory)
    python -m g2048._build --train [-o LIBRARY] [extra compiler flags ...]   (the training library alone)
    python -m g2048._build --tlearn [-o LIBRARY] [extra compiler flags ...]  (the transformer policy's learner library alone)
    python -m g2048._build --tstep [-o LIBRARY] [extra compiler flags ...]   (the transformer policy's optimiser-step library alone)
    python -m g2048._build --ttrain [-o LIBRARY] [extra compiler flags ...]  (the transformer policy's training-mode library alone)
    python -m g2048._build --collect [-o LIBRARY] [extra compiler flags ...] (the experience collector's library alone)
    python -m g2048._build --ppo-collect [-o LIBRARY] [extra compiler flags ...]   (the PPO experience collector's library alone)
    python -m g2048._build --tpolicy-collect [-o LIBRARY] [extra compiler flags ...]   (the transformer policy's collector alone)
    python -m g2048._build --tbf16 [-o LIBRARY] [extra compiler flags ...]   (the transformer policy's bf16 gradient library alone)
    python -m g2048._build --search [-o LIBRARY] [extra compiler flags ...]  (the expectimax agent's library alone)

The libraries are built in-tree so that they travel with the source snapshot; they are
git-ignored. -ffp-contract=off is REQUIRED: the reward / heuristic kernels follow
the reference's f64 operation order (mul then add, never fma).

LIBRARIES has a row per library; one more library is one more row there and one in g2048/_lib.py.
libg2048_train_hip.so (include/g2048_train.h) holds the Q-network's training-mode entry points: the main library's export
table is closed (ABI 5), so they live in a second library with the same flags and the same version script.
libg2048_tlearn_hip.so (include/g2048_tlearn.h) holds the transformer policy's PPO loss and gradient pass, a third library for
the same reason: the training library's table is closed too.
libg2048_tstep_hip.so (include/g2048_tstep.h) holds the transformer policy's NaN gate, clipping and Adam step, a fourth library:
the learner library's table is closed as well.
libg2048_ttrain_hip.so (include/g2048_ttrain.h) holds the transformer policy's training-mode passes (the encoder's live dropout), a
fifth library for the same reason; its kernels are the learner library's, shared as csrc/g2048_tpolicy_grad_pass.h.
EXTENSIONS is a second table of the same row shape, and libg2048_collect_hip.so (include/g2048_collect.h: the hybrid agent's
experience collection in one launch) is its one row. The split says nothing about the library: the tests pin LIBRARIES at five
rows, so the sixth shared object is counted here.
PPO_EXTENSIONS is a third table of that row shape, and libg2048_ppo_collect_hip.so (include/g2048_ppo_collect.h: the PPO agent's
experience collection in one launch) is its one row, for the same reason once more: the tests pin EXTENSIONS at that one row.
EXTRA_ROWS is the fourth and LAST table of that row shape: the tests pin ROWS, the union of the three above, at seven keys, and
nothing pins this one's size, so the next library is one more row here and not a fifth table. Its first row is
libg2048_tpolicy_collect_hip.so (include/g2048_tpolicy_collect.h: the transformer policy's experience collection in one launch); its
second is libg2048_tbf16_hip.so (include/g2048_tbf16.h: the transformer policy's gradient pass with bf16 feed-forward products; the
kernels are the learner library's plus csrc/g2048_tpolicy_bf16.h); its third is libg2048_search_hip.so (include/g2048_search.h: the
expectimax agent's decisions and complete games; csrc/g2048_expectimax.hip with the value function in csrc/g2048_expectimax.h).
Everything below reads ALL_ROWS, every table.
"""
import os
import shutil
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
INCLUDE = os.path.join(CSRC, "..", "..", "include")
# key: (product file, environment variable that names an A/B build to load in its place (tools/), sources, public headers).
# The key is the prefix of the module's names for the row: TRAIN_LIB, TRAIN_SOURCES; the main library's are LIB and SOURCES.
LIBRARIES = {
    "": ("libg2048_hip.so", "G2048_LIB",
         ["g2048_kernels.hip", "g2048_beam.hip", "g2048_rollout.hip", "g2048_policy.hip", "g2048_tpolicy.hip", "g2048_qnet.hip",
          "g2048_qnet_batch.hip", "g2048_qnet_grad.hip", "g2048_qnet_step.hip", "g2048_per.hip", "g2048_ppo_grad.hip", "g2048_ppo_step.hip"],
         ["g2048.h", "g2048_testing.h"]),
    "TRAIN_": ("libg2048_train_hip.so", "G2048_TRAIN_LIB", ["g2048_qnet_train.hip"], ["g2048_train.h"]),
    "TLEARN_": ("libg2048_tlearn_hip.so", "G2048_TLEARN_LIB", ["g2048_tpolicy_grad.hip"], ["g2048_tlearn.h"]),
    "TSTEP_": ("libg2048_tstep_hip.so", "G2048_TSTEP_LIB", ["g2048_tpolicy_step.hip"], ["g2048_tstep.h"]),
    "TTRAIN_": ("libg2048_ttrain_hip.so", "G2048_TTRAIN_LIB", ["g2048_tpolicy_train.hip"], ["g2048_ttrain.h"]),
}
EXTENSIONS = {
    "COLLECT_": ("libg2048_collect_hip.so", "G2048_COLLECT_LIB", ["g2048_qnet_collect.hip"], ["g2048_collect.h"]),
}
PPO_EXTENSIONS = {
    "PPO_COLLECT_": ("libg2048_ppo_collect_hip.so", "G2048_PPO_COLLECT_LIB", ["g2048_ppo_collect.hip"], ["g2048_ppo_collect.h"]),
}
ROWS = {**LIBRARIES, **EXTENSIONS, **PPO_EXTENSIONS}  # the seven shared objects the older tests count, whichever table counts them
EXTRA_ROWS = {
    "TPOLICY_COLLECT_": ("libg2048_tpolicy_collect_hip.so", "G2048_TPOLICY_COLLECT_LIB", ["g2048_tpolicy_collect.hip"],
                         ["g2048_tpolicy_collect.h"]),
    "TBF16_": ("libg2048_tbf16_hip.so", "G2048_TBF16_LIB", ["g2048_tpolicy_bf16.hip"], ["g2048_tbf16.h"]),
    "SEARCH_": ("libg2048_search_hip.so", "G2048_SEARCH_LIB", ["g2048_expectimax.hip"], ["g2048_search.h"]),
}
ALL_ROWS = {**ROWS, **EXTRA_ROWS}  # every shared object of the build
PUBLIC_HEADERS = [os.path.join(INCLUDE, h) for row in ALL_ROWS.values() for h in row[3]]
# LIB, SOURCES, TRAIN_LIB, TRAIN_SOURCES, ...: what the loader, the tools and the tests read; needs_build() and build() read the
# paths from here too, so a path that is replaced at run time is the one they look at
for _key, (_file, _env, _sources, _) in ALL_ROWS.items():
    globals()[_key + "LIB"] = os.environ.get(_env) or os.path.join(CSRC, _file)
    globals()[_key + "SOURCES"] = _sources
# -fvisibility=hidden: the export table is exactly what the two headers declare with G2048_API (tests/test_abi_and_host.py)
# -amdgpu-kernarg-preload-count: the first kernel-argument dwords arrive in SGPRs with the wavefront instead of through s_load +
# s_waitcnt at its head (gfx950 takes up to 14 next to the kernarg pointer; the short kernels order their arguments for it:
# 12.9 -> 12.55 us per 1 Mi-board step launch, profiles/r05_kernel_heads.txt)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
         "-mllvm", "-amdgpu-kernarg-preload-count=16",
         "-Wl,--version-script=" + os.path.join(CSRC, "g2048_exports.map"), "-Wall", "-Wno-unused-function"]


def path_of(key):
    return globals()[key + "LIB"]


def _stale(lib):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    # every file a source can include is a dependency: whatever lies in csrc/ (sources, headers, .inc) + the public headers
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc", ".hpp", ".map"))] + PUBLIC_HEADERS
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def needs_build():
    return any(_stale(path_of(key)) for key in ALL_ROWS)


def build_one(key, lib=None, extra_flags=(), verbose=False):
    """The library of row `key` alone, always made: the product's, or an A/B build at `lib` (loaded through the row's variable)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = lib or path_of(key)
    srcs = [os.path.join(CSRC, f) for f in ALL_ROWS[key][2] if os.path.exists(os.path.join(CSRC, f))]
    cmd = [hipcc] + FLAGS + list(extra_flags) + ["-o", out] + srcs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


def build(force=False, verbose=False, lib=None, extra_flags=()):
    """The product libraries, each only if it is stale. lib / extra_flags: an A/B or measurement build of the MAIN library next to
    the product's (tools/build_ab.sh); such a build is always made, and the other libraries are left alone."""
    if lib is not None:
        return build_one("", lib, extra_flags, verbose)
    for key in ALL_ROWS:
        if force or _stale(path_of(key)):
            build_one(key, None, extra_flags, verbose)
    return path_of("")


if __name__ == "__main__":          # [--train | --tlearn | --tstep | --ttrain | --collect | --ppo-collect | --tpolicy-collect | --tbf16 | --search] [-o LIBRARY] [extra compiler flags ...]
    out, args = None, sys.argv[1:]
    key = next((k for k in ALL_ROWS if k and args[:1] == ["--" + k[:-1].lower().replace("_", "-")]), None)
    if key:
        args = args[1:]
    if args[:1] == ["-o"]:
        out, args = args[1], args[2:]
    if key:
        print(build_one(key, lib=out, extra_flags=args, verbose=True))
    else:
        print(build(force=True, verbose=True, lib=out, extra_flags=args))
