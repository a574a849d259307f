"""The host side of csrc/g2048_step_common.h, which the three optimiser-step entry points share: decimal_of, the check of the Adam
hyper-parameters and its messages, the chunks behind the workspace sizes, the clip coefficient and the bias corrections -- in a
stand-alone program (tests/host_step) built without device code and with ASan + UBSan, run here without a GPU."""
import os
import re
import subprocess

from conftest import REPO


def test_the_shared_step_header_on_the_host_asan_ubsan_clean():
    d = os.path.join(REPO, "tests", "host_step")
    subprocess.check_call(["make", "-C", d, "-s"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([os.path.join(d, "step_common_host")], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    done = re.search(r"step_common_host: (\d+) checks, 0 failed", out.stdout)
    assert done and int(done.group(1)) >= 100 and "FAILED" not in out.stdout, out.stdout
