"""The scenario queue of a QCQP context (sqphip_qcqp_stream_begin / _set, sqphip_sqp_stream_get_full) as far as it can be
checked without a GPU: the symbols are exported by libsqphip.so and declared in include/sqphip.h (tests/test_abi.py compares
the header with _lib.EXPORTS), they refuse a NULL handle, and host.Context has the methods."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import sqpsolver_jl_amd as pkg                                        # noqa: E402
from sqpsolver_jl_amd import _lib                                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sqphip_qcqp_stream_begin", "sqphip_qcqp_stream_set", "sqphip_sqp_stream_get_full")
EINVAL = -1


def test_symbols_are_exported_and_declared():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "sqphip.h")).read()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    # the declared argument counts are the ones the ctypes layer passes
    assert len(L.sqphip_qcqp_stream_begin.argtypes) == 3
    assert len(L.sqphip_qcqp_stream_set.argtypes) == 13
    assert len(L.sqphip_sqp_stream_get_full.argtypes) == 10


def test_null_handle_is_refused():
    L = _lib.lib()
    assert L.sqphip_qcqp_stream_begin(None, 4, 1) == EINVAL
    assert L.sqphip_qcqp_stream_set(None, 0, *([None] * 11)) == EINVAL
    assert L.sqphip_sqp_stream_get_full(None, 0, *([None] * 8)) == EINVAL


def test_host_context_has_the_methods():
    for name in ("qcqp_stream_begin", "qcqp_stream_set", "stream_get_full"):
        assert callable(getattr(pkg.Context, name, None)), name


def test_header_no_longer_says_the_queue_cannot_carry_qcqp_values():
    header = open(os.path.join(ROOT, "include", "sqphip.h")).read()
    assert "does not carry QCQP values" not in header
