"""CPU tests of the batched drop-in seat: every new symbol is exported and bound, misuse that needs no device work is
refused with SQPHIP_EINVAL, and the Python wrappers refuse ragged input before the library sees a pointer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sqpsolver_jl_amd import _lib
from sqpsolver_jl_amd.host import Context, QpHip, QpData

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
SEAT = ["sqphip_qp_solve_batch", "sqphip_qp_stats_batch"]
MERIT = ["sqphip_norm_violations_batch", "sqphip_kt_residuals_batch", "sqphip_norm_complementarity_batch",
         "sqphip_compute_phi_batch", "sqphip_compute_qmodel_batch", "sqphip_compute_derivative_full_batch"]


def test_every_batch_symbol_is_declared_exported_and_bound():
    _lib.build()
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "sqphip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for sym in SEAT + MERIT:
        proto = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % sym, hdr, flags=re.S)
        assert proto, sym
        assert sym in _lib.EXPORTS and hasattr(L, sym)
        fn = getattr(L, sym)
        assert fn.argtypes is not None and len(fn.argtypes) == len(proto.group(1).split(",")), sym
        # `count, inst` in front, behind the context
        assert fn.argtypes[1] is C.c_int32 and fn.argtypes[2] == C.POINTER(C.c_int32), sym
    # the scalar twin of every merit call exists, and the batch form has its operands plus count and inst
    for sym in MERIT:
        twin = getattr(L, sym[:-len("_batch")])
        assert len(getattr(L, sym).argtypes) == len(twin.argtypes) + 2, sym
    # the Julia shim binds the seat and one merit call
    jl = open(os.path.join(ROOT, "julia", "SqpHip.jl")).read()
    assert "(:sqphip_qp_solve_batch, LIBSQPHIP)" in jl
    assert any("(:%s, LIBSQPHIP)" % s in jl for s in MERIT)


def test_null_context_and_null_arrays_are_einval():
    L = _lib.lib()
    d = (C.c_double * 8)(); i = (C.c_int32 * 2)()
    dn, inn = C.POINTER(C.c_double)(), C.POINTER(C.c_int32)()
    dp = C.cast(d, C.POINTER(C.c_double)); ip = C.cast(i, C.POINTER(C.c_int32))
    assert L.sqphip_qp_solve_batch(None, 1, ip, ip, dp, dp, dp, dp, dp, dp, dn, dp, dp, dp, dp, dn, ip) == EINVAL
    assert L.sqphip_qp_stats_batch(None, 1, ip, ip, ip, ip, dp) == EINVAL
    assert L.sqphip_norm_violations_batch(None, 1, ip, dp, dp, 1, dp) == EINVAL
    assert L.sqphip_kt_residuals_batch(None, 1, ip, dp, dp, dp, dp, dp, dp) == EINVAL
    assert L.sqphip_norm_complementarity_batch(None, 1, ip, dp, dp, 0, dp) == EINVAL
    assert L.sqphip_compute_phi_batch(None, 1, ip, dp, dp, dp, dp, 0, dp) == EINVAL
    assert L.sqphip_compute_qmodel_batch(None, 1, ip, dp, dp, dp, dp, dp, dn, dp, 1, dp) == EINVAL
    assert L.sqphip_compute_derivative_full_batch(None, 1, ip, dp, dp, dp, dp, dn, 0, dn, dp) == EINVAL
    # required arrays: checked before the context is touched (any non-null handle will do -- it is never dereferenced)
    fake = C.c_void_p(C.addressof(d))
    assert L.sqphip_qp_solve_batch(fake, 1, ip, inn, dp, dp, dp, dp, dp, dp, dn, dp, dp, dp, dp, dn, ip) == EINVAL   # mode
    assert L.sqphip_qp_solve_batch(fake, 1, ip, ip, dn, dp, dp, dp, dp, dp, dn, dp, dp, dp, dp, dn, ip) == EINVAL    # x_k
    assert L.sqphip_qp_solve_batch(fake, 1, ip, ip, dp, dn, dp, dp, dp, dp, dn, dp, dp, dp, dp, dn, ip) == EINVAL    # delta
    assert L.sqphip_qp_solve_batch(fake, 1, ip, ip, dp, dp, dp, dp, dp, dn, dn, dp, dp, dp, dp, dn, ip) == EINVAL    # Jval
    assert L.sqphip_qp_solve_batch(fake, 1, ip, ip, dp, dp, dp, dp, dp, dp, dn, dn, dp, dp, dp, dn, ip) == EINVAL    # p
    assert L.sqphip_qp_solve_batch(fake, 1, ip, ip, dp, dp, dp, dp, dp, dp, dn, dp, dp, dp, dp, dn, inn) == EINVAL   # status
    assert L.sqphip_norm_violations_batch(fake, 1, ip, dn, dp, 1, dp) == EINVAL
    assert L.sqphip_norm_violations_batch(fake, 1, ip, dp, dp, 3, dp) == EINVAL                                      # pnorm
    assert L.sqphip_kt_residuals_batch(fake, 1, ip, dp, dp, dp, dp, dn, dp) == EINVAL
    assert L.sqphip_norm_complementarity_batch(fake, 1, ip, dp, dn, 0, dp) == EINVAL
    assert L.sqphip_compute_phi_batch(fake, 1, ip, dn, dp, dp, dp, 0, dp) == EINVAL
    assert L.sqphip_compute_qmodel_batch(fake, 1, ip, dp, dn, dp, dp, dp, dn, dp, 1, dp) == EINVAL                   # p with a step
    assert L.sqphip_compute_derivative_full_batch(fake, 1, ip, dp, dp, dp, dp, dn, 1, dn, dp) == EINVAL              # slack under FR


class _NoLibrary:
    """stands where the library would: any call into it fails the test"""
    def __getattr__(self, name):
        def refuse(*args):
            raise AssertionError(f"{name} was called with malformed input")
        return refuse


def _ctx(n=3, m=2, nnzj=4, nnzh=2, batch=4):
    c = Context.__new__(Context)
    c.L, c.h = _NoLibrary(), None
    c.n, c.m, c.batch, c.nnzj, c.nnzh = n, m, batch, nnzj, nnzh
    return c


def test_wrappers_refuse_ragged_input_before_the_library():
    c = _ctx()
    ok = dict(inst=[0, 1], mode=[0, 0], x_k=[np.zeros(3)] * 2, delta=[1.0, 2.0], mu=1.0, df=[np.zeros(3)] * 2,
              E=[np.zeros(2)] * 2, jval=[np.zeros(4)] * 2, hval=[np.zeros(2)] * 2)
    bad = [("x_k", [np.zeros(3), np.zeros(2)]), ("x_k", [np.zeros(3)]), ("df", [np.zeros(3), np.zeros(4)]),
           ("E", [np.zeros(2), np.zeros(3)]), ("jval", [np.zeros(4)] * 3), ("hval", [np.zeros(2), np.zeros(1)]),
           ("hval", [np.zeros(2), None]), ("mode", [0]), ("delta", [1.0, 2.0, 3.0]), ("mu", [1.0]), ("inst", []),
           ("x_k", [np.zeros((1, 3))] * 2)]
    for key, val in bad:
        with pytest.raises(ValueError):
            c.qp_solve_batch(**{**ok, key: val})
    with pytest.raises(ValueError):
        c.norm_violations_batch([0, 1], [np.zeros(2)] * 2, [np.zeros(3), np.zeros(2)])
    with pytest.raises(ValueError):
        c.kt_residuals_batch([0, 1], [np.zeros(3)] * 2, [np.zeros(2)] * 2, [np.zeros(3)] * 2, [np.zeros(3)] * 2, [np.zeros(4)])
    with pytest.raises(ValueError):
        c.norm_complementarity_batch([0, 1], [np.zeros(2)] * 2, [np.zeros(3)] * 2)
    with pytest.raises(ValueError):
        c.compute_phi_batch([0, 1], [1.0], [np.zeros(2)] * 2, [np.zeros(3)] * 2, 1.0, 0)
    with pytest.raises(ValueError):
        c.compute_qmodel_batch([0, 1], [np.zeros(3)] * 2, [np.zeros(3)] * 2, [np.zeros(3)] * 2, [np.zeros(2)] * 2,
                               [np.zeros(4), np.zeros(5)], None, 1.0, 1)
    with pytest.raises(ValueError):
        c.compute_derivative_full_batch([0, 1], [np.zeros(3)] * 2, [np.zeros(3)] * 2, [np.zeros(2)] * 2, [1.0, 1.0],
                                        [np.zeros(2), np.zeros(1)])
    # the QpData helpers go through the same checks
    q = QpHip(c)
    dta = [QpData(np.zeros(2), np.zeros(3), np.zeros(4), np.zeros(2), None, None, None, None, 0),
           QpData(np.zeros(2), np.zeros(3), np.zeros(3), np.zeros(2), None, None, None, None, 0)]
    for call in (lambda: q.sub_optimize_batch([0, 1], dta, [np.zeros(3)] * 2, [1.0, 1.0]),
                 lambda: q.sub_optimize_FR_batch([0, 1], dta, [np.zeros(3)] * 2, 1.0),
                 lambda: q.sub_optimize_lp_batch([0, 1], dta, [np.zeros(3)] * 2)):
        with pytest.raises(ValueError):
            call()
