"""smx_compose_batch's C ABI without a GPU: the ctypes mirror of smx_batch has the header's
layout, and the argument errors come back before any HIP call."""
import ctypes as C
import os

import pytest

from semantic_merge_amd import _abi
from semantic_merge_amd._lib import LIB_PATH

from _util import assert_header_layout

SMX_OK, SMX_E_ARG, SMX_E_WORKSPACE = 0, -1, -4


def test_smx_batch_matches_header():
    assert_header_layout({"smx_batch": _abi.SmxBatch})


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB_PATH), "build libsmx.so first (__graft_entry__.build())"
    return _abi.declare(C.CDLL(LIB_PATH))


def test_workspace_query(lib):
    size = C.c_size_t(0)
    assert lib.smx_compose_batch_workspace_bytes(1000, C.byref(size)) == SMX_OK
    assert size.value > 0
    assert lib.smx_compose_batch_workspace_bytes(-1, C.byref(size)) == SMX_E_ARG
    assert lib.smx_last_error()
    assert lib.smx_compose_batch_workspace_bytes(0, C.byref(size)) == SMX_OK


def _batch(n_merges, n_total, buf):
    """A batch whose every pointer is the (host) buffer `buf`: the calls below fail before
    anything reads it."""
    p = C.addressof(buf) if buf is not None else 0
    return _abi.SmxBatch(n_merges, n_total, 4, *([p] * 16), 0)


def test_argument_errors_without_gpu(lib):
    buf = (C.c_uint8 * 4096)()
    ws = (C.c_uint8 * 4096)()
    need = C.c_size_t(0)
    assert lib.smx_compose_batch_workspace_bytes(1, C.byref(need)) == SMX_OK
    assert 0 < need.value <= 4096
    # negative sizes
    for b in (_batch(-1, 10, buf), _batch(1, -1, buf)):
        assert lib.smx_compose_batch(C.byref(b), ws, 4096, None) == SMX_E_ARG
    b = _batch(1, 10, buf)
    b.n_sym = -1
    assert lib.smx_compose_batch(C.byref(b), ws, 4096, None) == SMX_E_ARG
    b = _batch(1, 10, buf)
    b.grid_cap = -1
    assert lib.smx_compose_batch(C.byref(b), ws, 4096, None) == SMX_E_ARG
    # null columns with one merge; then each pointer alone
    assert lib.smx_compose_batch(C.byref(_batch(1, 10, None)), ws, 4096, None) == SMX_E_ARG
    for fname, ft in _abi.SmxBatch._fields_:
        if ft is C.c_void_p:
            b = _batch(1, 10, buf)
            setattr(b, fname, None)
            assert lib.smx_compose_batch(C.byref(b), ws, 4096, None) == SMX_E_ARG, fname
    assert lib.smx_compose_batch(None, ws, 4096, None) == SMX_E_ARG
    # a short or missing workspace
    b = _batch(1, 10, buf)
    assert lib.smx_compose_batch(C.byref(b), ws, need.value - 1, None) == SMX_E_WORKSPACE
    assert lib.smx_compose_batch(C.byref(b), None, 4096, None) == SMX_E_WORKSPACE
    assert b"workspace" in lib.smx_last_error()


def test_no_merges_is_ok(lib):
    assert lib.smx_compose_batch(C.byref(_batch(0, 0, None)), None, 0, None) == SMX_OK
