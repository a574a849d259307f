"""Builds csrc/libg2048_hip.so, csrc/libg2048_train_hip.so, csrc/libg2048_tlearn_hip.so and csrc/libg2048_tstep_hip.so for gfx950
with hipcc (cross-compiles without a GPU).

    python -m g2048._build [-o LIBRARY] [extra compiler flags ...]           (from the package directory)
    python -m g2048._build --train [-o LIBRARY] [extra compiler flags ...]   (the training library alone)
    python -m g2048._build --tlearn [-o LIBRARY] [extra compiler flags ...]  (the transformer policy's learner library alone)
    python -m g2048._build --tstep [-o LIBRARY] [extra compiler flags ...]   (the transformer policy's optimiser-step library alone)

The libraries are built in-tree so that they travel with the source snapshot; they are
git-ignored. -ffp-contract=off is REQUIRED: the reward / heuristic kernels follow
the reference's f64 operation order (mul then add, never fma).

libg2048_train_hip.so (include/g2048_train.h) holds the Q-network's training-mode entry points: the main library's export
table is closed (ABI 5), so they live in a second library with the same flags and the same version script.
libg2048_tlearn_hip.so (include/g2048_tlearn.h) holds the transformer policy's PPO loss and gradient pass, a third library for
the same reason: the training library's table is closed too.
libg2048_tstep_hip.so (include/g2048_tstep.h) holds the transformer policy's NaN gate, clipping and Adam step, a fourth library:
the learner library's table is closed as well.
"""
import os
import shutil
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
LIB = os.environ.get("G2048_LIB") or os.path.join(CSRC, "libg2048_hip.so")     # G2048_LIB: A/B builds only (tools/)
TRAIN_LIB = os.environ.get("G2048_TRAIN_LIB") or os.path.join(CSRC, "libg2048_train_hip.so")     # G2048_TRAIN_LIB: A/B builds only
SOURCES = ["g2048_kernels.hip", "g2048_beam.hip", "g2048_rollout.hip", "g2048_policy.hip", "g2048_tpolicy.hip",
           "g2048_qnet.hip", "g2048_qnet_batch.hip", "g2048_qnet_grad.hip", "g2048_qnet_step.hip", "g2048_per.hip", "g2048_ppo_grad.hip",
           "g2048_ppo_step.hip"]
TLEARN_LIB = os.environ.get("G2048_TLEARN_LIB") or os.path.join(CSRC, "libg2048_tlearn_hip.so")   # G2048_TLEARN_LIB: A/B builds only
TRAIN_SOURCES = ["g2048_qnet_train.hip"]
TLEARN_SOURCES = ["g2048_tpolicy_grad.hip"]
TSTEP_LIB = os.environ.get("G2048_TSTEP_LIB") or os.path.join(CSRC, "libg2048_tstep_hip.so")      # G2048_TSTEP_LIB: A/B builds only
TSTEP_SOURCES = ["g2048_tpolicy_step.hip"]
INCLUDE = os.path.join(CSRC, "..", "..", "include")
PUBLIC_HEADERS = [os.path.join(INCLUDE, "g2048.h"), os.path.join(INCLUDE, "g2048_testing.h"), os.path.join(INCLUDE, "g2048_train.h"),
                  os.path.join(INCLUDE, "g2048_tlearn.h"), os.path.join(INCLUDE, "g2048_tstep.h")]
# -fvisibility=hidden: the export table is exactly what the two headers declare with G2048_API (tests/test_abi_and_host.py)
# -amdgpu-kernarg-preload-count: the first kernel-argument dwords arrive in SGPRs with the wavefront instead of through s_load +
# s_waitcnt at its head (gfx950 takes up to 14 next to the kernarg pointer; the short kernels order their arguments for it:
# 12.9 -> 12.55 us per 1 Mi-board step launch, profiles/r05_kernel_heads.txt)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
         "-mllvm", "-amdgpu-kernarg-preload-count=16",
         "-Wl,--version-script=" + os.path.join(CSRC, "g2048_exports.map"), "-Wall", "-Wno-unused-function"]


def _stale(lib):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    # every file a source can include is a dependency: whatever lies in csrc/ (sources, headers, .inc) + the public headers
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc", ".hpp", ".map"))] + PUBLIC_HEADERS
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def needs_build():
    return _stale(LIB) or _stale(TRAIN_LIB) or _stale(TLEARN_LIB) or _stale(TSTEP_LIB)


def _compile(sources, out, extra_flags, verbose):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    srcs = [os.path.join(CSRC, f) for f in sources if os.path.exists(os.path.join(CSRC, f))]
    cmd = [hipcc] + FLAGS + list(extra_flags) + ["-o", out] + srcs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


def build(force=False, verbose=False, lib=None, extra_flags=()):
    """The four product libraries, each only if it is stale. lib / extra_flags: an A/B or measurement build of the MAIN library next to
    the product's (tools/build_ab.sh); such a build is always made, and the other three libraries are left alone."""
    if lib is not None:
        return _compile(SOURCES, lib, extra_flags, verbose)
    if force or _stale(LIB):
        _compile(SOURCES, LIB, extra_flags, verbose)
    if force or _stale(TRAIN_LIB):
        _compile(TRAIN_SOURCES, TRAIN_LIB, extra_flags, verbose)
    if force or _stale(TLEARN_LIB):
        _compile(TLEARN_SOURCES, TLEARN_LIB, extra_flags, verbose)
    if force or _stale(TSTEP_LIB):
        _compile(TSTEP_SOURCES, TSTEP_LIB, extra_flags, verbose)
    return LIB


def build_train(lib=None, extra_flags=(), verbose=False):
    """The training library alone, always made: the product's, or an A/B build at `lib` (loaded through G2048_TRAIN_LIB)."""
    return _compile(TRAIN_SOURCES, lib or TRAIN_LIB, extra_flags, verbose)


def build_tlearn(lib=None, extra_flags=(), verbose=False):
    """The transformer policy's learner library alone, always made: the product's, or an A/B build at `lib` (loaded through
    G2048_TLEARN_LIB)."""
    return _compile(TLEARN_SOURCES, lib or TLEARN_LIB, extra_flags, verbose)


def build_tstep(lib=None, extra_flags=(), verbose=False):
    """The transformer policy's optimiser-step library alone, always made: the product's, or an A/B build at `lib` (loaded through
    G2048_TSTEP_LIB)."""
    return _compile(TSTEP_SOURCES, lib or TSTEP_LIB, extra_flags, verbose)


if __name__ == "__main__":          # [--train | --tlearn | --tstep] [-o LIBRARY] [extra compiler flags ...]
    import sys
    out, args = None, sys.argv[1:]
    train, tlearn, tstep = args[:1] == ["--train"], args[:1] == ["--tlearn"], args[:1] == ["--tstep"]
    if train or tlearn or tstep:
        args = args[1:]
    if args[:1] == ["-o"]:
        out, args = args[1], args[2:]
    if train:
        print(build_train(lib=out, extra_flags=args, verbose=True))
    elif tlearn:
        print(build_tlearn(lib=out, extra_flags=args, verbose=True))
    elif tstep:
        print(build_tstep(lib=out, extra_flags=args, verbose=True))
    else:
        print(build(force=True, verbose=True, lib=out, extra_flags=args))
