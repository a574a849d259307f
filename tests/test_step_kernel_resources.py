"""What the compiler reports for every step_kernel instantiation, with no GPU: registers, scratch and occupancy from its own
summary in the assembly listing, and the modelled VALU cycles per wavefront of tools/isa_cost.py for the two headline variants.

The chained headline of bench.py keeps two launches of the two-boards-per-lane kernel resident together, which needs all 8
wavefront slots of a SIMD: an instantiation that allocates more than 64 VGPRs drops to 7, and one that spills pays for it in
scratch traffic. The cycle caps are the figures of the commit before the two-board path took 32-bit byte offsets and an
unconditional load head (2453 and 1230 with the flags of g2048/_build.py); this tree measures 2432 and 1230."""
import os
import re
import subprocess
import sys

import pytest

from conftest import PKG, REPO

LINK_ONLY = ("-shared", "-Wl,")
CAPS = {"ILb0ELb0ELi2ELi256ELb0ELb0E": 2453, "ILb0ELb0ELi1ELi256ELb0ELb0E": 1230}


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    sys.path.insert(0, PKG)
    from g2048 import _build
    flags = [f for f in _build.FLAGS if not f.startswith(LINK_ONLY)]
    out = str(tmp_path_factory.mktemp("step_listing") / "g2048_kernels.s")
    hipcc = _build.shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", "-o", out, os.path.join(_build.CSRC, "g2048_kernels.hip")],
                          stderr=subprocess.DEVNULL)
    return out


def step_kernels(text):
    """{mangled name: (NumVgprs, ScratchSize, Occupancy)} of every step_kernel instantiation in the listing."""
    found = {}
    for m in re.finditer(r"^(_Z\w*11step_kernelI\w+):.*?^\.Lfunc_end.*?; NumVgprs: (\d+).*?; ScratchSize: (\d+).*?; Occupancy: (\d+)",
                         text, re.S | re.M):
        found[m.group(1)] = tuple(int(m.group(k)) for k in (2, 3, 4))
    return found


def test_every_step_kernel_fits_eight_waves_without_scratch(listing):
    from test_gpu_step_matrix import STEP_KERNELS
    found = step_kernels(open(listing).read())
    assert len(found) == len(STEP_KERNELS), sorted(found)
    for name, (vgprs, scratch, occupancy) in sorted(found.items()):
        print(name[:60], "NumVgprs", vgprs, "ScratchSize", scratch, "Occupancy", occupancy)
    for name, (vgprs, scratch, occupancy) in found.items():
        assert scratch == 0, (name, scratch)
        assert occupancy == 8, (name, vgprs, occupancy)


def test_modelled_cycles_of_the_headline_variants(listing):
    out = subprocess.check_output([sys.executable, os.path.join(REPO, "tools", "isa_cost.py"), listing, "step_kernel"], text=True)
    seen = {}
    for line in out.splitlines():
        for key in CAPS:
            if key in line:
                seen[key] = int(re.search(r"est cycles/wave (\d+)", line).group(1))
    print(seen)
    assert set(seen) == set(CAPS), out
    for key, cap in CAPS.items():
        assert seen[key] <= cap, (key, seen[key], cap)
