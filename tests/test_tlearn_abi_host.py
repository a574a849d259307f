"""What only the learner library has (csrc/libg2048_tlearn_hip.so, include/g2048_tlearn.h): its batch limit, its workspace
arithmetic, every argument check of g2048_tpolicy_loss_grad before any device call (there is no device here) and the Python
layer's refusals. Its export table, header, binding table, inventory of bounds tests and loader are checked with the other
libraries' (tests/test_libraries_abi_host.py)."""
import ctypes as C
import os
import re

import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    return _lib


def test_the_batch_limit_is_the_header_s(built):
    hdr = open(os.path.join(REPO, "include", "g2048_tlearn.h")).read()
    assert int(re.search(r"#define G2048_TLEARN_BATCH_MAX (\d+)", hdr).group(1)) == 1024 == built.TLEARN_BATCH_MAX


def test_workspace_query_refuses_shapes_and_grows(built):
    ws = built.tlearn_lib().g2048_tpolicy_grad_workspace
    assert ws(0, 2048, 2) == 0 and ws(1025, 2048, 2) == 0 and ws(64, 48, 2) == 0 and ws(64, 0, 2) == 0 and ws(64, 2048, 0) == 0
    assert ws(64, 2048, 65) == 0 and ws(64, 65568, 2) == 0
    assert 0 < ws(1, 32, 1) < ws(2, 32, 1) < ws(17, 32, 1) < ws(1024, 32, 1)
    assert ws(64, 32, 2) < ws(64, 64, 2) < ws(64, 2048, 2) and ws(64, 2048, 1) < ws(64, 2048, 2)
    assert all(ws(n, ff, l) % 16 == 0 for n in (1, 3, 17, 1024) for ff in (32, 96, 2048) for l in (1, 3))
    assert ws(1024, 2048, 2) == 396800000, "the figure DESIGN.md states for N = 1,024, dim_ff 2,048, 2 layers"


def test_argument_checks_happen_before_any_device_call(built):
    """Host addresses that are never dereferenced: every refusal is decided from the arguments alone, and N = 0 returns 0."""
    T = built.tlearn_lib()
    err = lambda: T.g2048_tlearn_last_error().decode()      # noqa: E731
    n, ff, layers = 17, 96, 2
    nb = T.g2048_tpolicy_grad_workspace(n, ff, layers)
    p = 0x10000                                              # 16-byte aligned, not null
    f = C.c_float

    def call(boards=p, plain=p, actions=p, old=p, adv=p, ret=p, n=n, ff=ff, layers=layers, clip=0.3, vc=0.4, ec=0.05, grad=p, losses=p,
             probs=p, value=p, ws=p, nb=nb):
        return T.g2048_tpolicy_loss_grad(boards, plain, actions, old, adv, ret, n, ff, layers, f(clip), f(vc), f(ec), grad, losses, probs,
                                         value, ws, nb, None)

    assert call(n=0) == 0, "N = 0 returns G2048_OK and launches nothing"
    assert call(n=0, boards=None, ws=None, nb=0) == 0
    for name in ("boards", "plain", "actions", "old", "adv", "ret", "grad", "losses", "probs", "value", "ws"):
        assert call(**{name: None}) == -1 and "null pointer" in err(), name
    assert call(n=1025, nb=1 << 40) == -1 and "1024" in err()
    assert call(ff=48) == -1 and "multiple of 32" in err()
    assert call(layers=0) == -1 and "n_layers" in err()
    assert call(nb=nb - 1) == -1 and "workspace" in err() and str(nb) in err()
    for name, off in (("boards", 8), ("plain", 4), ("grad", 8), ("probs", 4), ("ws", 8), ("actions", 4), ("old", 2), ("losses", 1), ("value", 2)):
        assert call(**{name: p + off}) == -1 and "misaligned" in err(), name
    for name in ("clip", "vc", "ec"):
        assert call(**{name: -0.1}) == -1 and call(**{name: float("nan")}) == -1 and call(**{name: float("inf")}) == -1, name
        assert "finite" in err()


def test_python_refuses_before_the_library(built):
    from g2048 import ops
    with pytest.raises(ValueError, match="1024"):
        ops.tpolicy_grad_workspace_bytes(1025, 2048, 2)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.tpolicy_grad_workspace_bytes(64, 48, 2)
    assert ops.tpolicy_grad_workspace_bytes(1024, 2048, 2) == 396800000
