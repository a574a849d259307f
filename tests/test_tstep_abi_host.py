"""What only the step library has (csrc/libg2048_tstep_hip.so, include/g2048_tstep.h): its workspace arithmetic, every argument
check of g2048_tpolicy_adam_step before any device call (there is no device here) and the Python layer's refusals. Its export
table, header, binding table, inventory of bounds tests and loader are checked with the other libraries'
(tests/test_libraries_abi_host.py)."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from g2048 import _lib
    return _lib


def test_workspace_query_refuses_shapes_and_is_a_multiple_of_16(built):
    ws = built.tstep_lib().g2048_tpolicy_step_workspace
    assert ws(48, 2) == 0 and ws(0, 2) == 0 and ws(2048, 0) == 0 and ws(2048, 65) == 0 and ws(65568, 2) == 0 and ws(-32, 2) == 0
    shapes = [(ff, l) for ff in (32, 96, 2048, 4096, 65536) for l in (1, 2, 3, 64)]
    assert all(ws(ff, l) > 0 and ws(ff, l) % 16 == 0 for ff, l in shapes)
    assert max(ws(ff, l) for ff, l in shapes) <= 1024 * 8 + 16, "at most 1,024 partial sums and one 16-byte record"
    # a partial per 1,024 floats up to 1,024 partials: 158, 194 and 686 of them; at 1,230,601 floats a chunk is 2,048 floats: 601
    assert [ws(32, 1), ws(96, 2), ws(2048, 2), ws(4096, 2)] == [158 * 8 + 16, 194 * 8 + 16, 686 * 8 + 16, 601 * 8 + 8 + 16]


def test_argument_checks_happen_before_any_device_call(built):
    """Host addresses that are never dereferenced: every refusal is decided from the arguments alone, each call below with exactly
    one defect."""
    T = built.tstep_lib()
    err = lambda: T.g2048_tstep_last_error().decode()      # noqa: E731
    ff, layers = 96, 2
    nb = T.g2048_tpolicy_step_workspace(ff, layers)
    p = 0x10000                                              # 16-byte aligned, not null
    f = C.c_float
    nan, inf = float("nan"), float("inf")

    def call(plain=p, grad=p, m=p, v=p, ff=ff, layers=layers, loss=p, counters=p, lr=3e-4, b1=0.9, b2=0.999, eps=1e-8, max_norm=0.5,
             norm=p, ws=p, nb=nb):
        return T.g2048_tpolicy_adam_step(plain, grad, m, v, ff, layers, loss, counters, f(lr), f(b1), f(b2), f(eps), f(max_norm), norm, ws,
                                         nb, None)

    for name in ("plain", "grad", "m", "v", "counters", "norm", "ws"):
        assert call(**{name: None}) == -1 and "g2048_tpolicy_adam_step: null pointer" in err(), name
    for name in ("plain", "grad", "m", "v", "ws"):
        for off in (4, 8):
            assert call(**{name: p + off}) == -1 and "misaligned" in err(), (name, off)
    assert call(counters=p + 4) == -1 and "misaligned" in err()
    assert call(norm=p + 2) == -1 and "misaligned" in err()
    assert call(loss=p + 2) == -1 and "misaligned" in err()
    assert call(ff=48) == -1 and "multiple of 32" in err()
    assert call(ff=65568) == -1 and "multiple of 32" in err()
    assert call(layers=0) == -1 and "n_layers" in err()
    assert call(layers=65) == -1 and "n_layers" in err()
    for key in ("lr", "b1", "b2", "eps"):
        for bad in (nan, inf, -inf, -1e-3):
            assert call(**{key: bad}) == -1 and "finite and not negative" in err(), (key, bad)
    for key in ("b1", "b2"):
        for bad in (1.0, 1.5):
            assert call(**{key: bad}) == -1 and "must be below 1" in err(), (key, bad)
    for bad in (nan, 0.0, -0.5, -inf):
        assert call(max_norm=bad) == -1 and "max_norm must be above 0" in err(), bad
    assert call(nb=nb - 1) == -1 and "workspace" in err() and str(nb) in err()
    assert call(nb=0) == -1 and str(nb) in err()


def test_python_refuses_before_the_library(built):
    from g2048 import ops
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.tpolicy_step_workspace_bytes(48, 2)
    with pytest.raises(ValueError, match="1 .. 64 layers"):
        ops.tpolicy_step_workspace_bytes(2048, 0)
    assert ops.tpolicy_step_workspace_bytes(2048, 2) == 686 * 8 + 16
