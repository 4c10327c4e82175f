"""smx_screen's C ABI without a GPU: the ctypes mirror of smx_screen has the header's layout,
the library exports the new symbols, and the argument errors come back before any HIP call."""
import ctypes as C
import os

import pytest

from semantic_merge_amd import _abi
from semantic_merge_amd._lib import LIB_PATH

from _util import assert_header_layout

SMX_OK, SMX_E_ARG, SMX_E_WORKSPACE = 0, -1, -4


def test_smx_screen_matches_header():
    assert_header_layout({"struct smx_screen": _abi.SmxScreen})


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB_PATH), "build libsmx.so first (__graft_entry__.build())"
    return _abi.declare(C.CDLL(LIB_PATH))


def test_symbols_exported(lib):
    for name in ("smx_screen_workspace_bytes", "smx_screen"):
        assert name in _abi.EXPORTS
        assert hasattr(lib, name), name
    assert lib.smx_screen.argtypes[0] is C.POINTER(_abi.SmxScreen)
    assert _abi.SCREEN_CLASSES[-1] == _abi.SCREEN_MAX_RENAMES == 2048


def test_workspace_query(lib):
    size = C.c_size_t(0)
    assert lib.smx_screen_workspace_bytes(100, 50_000, 1000, C.byref(size)) == SMX_OK
    assert size.value >= 50_000 * 36   # the rename records: three keys, index, symbol, class per op
    for args in ((-1, 10, 1), (1, -1, 1), (1, 10, -1), (1 << 31, 10, 1), (1, 10, 1 << 31)):
        assert lib.smx_screen_workspace_bytes(*args, C.byref(size)) == SMX_E_ARG, args
        assert lib.smx_last_error()
    assert lib.smx_screen_workspace_bytes(5, 5, 5, None) == SMX_E_ARG
    assert lib.smx_screen_workspace_bytes(0, 0, 0, C.byref(size)) == SMX_OK


N_PTR = 12


def _screen(n_logs, n_total, n_pairs, buf):
    """A screen whose every pointer is the (host) buffer `buf`: the calls below fail before
    anything reads it."""
    p = C.addressof(buf) if buf is not None else 0
    return _abi.SmxScreen(n_logs, n_total, n_pairs, *([p] * N_PTR), 0)


def test_argument_errors_without_gpu(lib):
    buf = (C.c_uint8 * 4096)()
    ws = (C.c_uint8 * 8192)()
    need = C.c_size_t(0)
    assert lib.smx_screen_workspace_bytes(2, 10, 1, C.byref(need)) == SMX_OK
    assert 0 < need.value <= 8192

    def call(s, w=ws, nbytes=8192):
        rc = lib.smx_screen(C.byref(s) if s is not None else None, w, nbytes, None)
        if rc != SMX_OK:
            assert lib.smx_last_error(), "an error code without a message"
        return rc

    # negative sizes
    for s in (_screen(-1, 10, 1, buf), _screen(2, -1, 1, buf), _screen(2, 10, -1, buf)):
        assert call(s) == SMX_E_ARG
    s = _screen(2, 10, 1, buf)
    s.grid_cap = -1
    assert call(s) == SMX_E_ARG
    # null columns with one pair; then each pointer alone
    assert call(_screen(2, 10, 1, None)) == SMX_E_ARG
    n_ptr = 0
    for fname, ft in _abi.SmxScreen._fields_:
        if ft is C.c_void_p:
            s = _screen(2, 10, 1, buf)
            setattr(s, fname, None)
            assert call(s) == SMX_E_ARG, fname   # (conflicts / conf_off: exactly one of them null)
            n_ptr += 1
    assert n_ptr == N_PTR
    # conflicts and conf_off: both or neither.  Both null is valid (capacity 0 everywhere):
    # the call goes on to the workspace check, which fails before any HIP call
    s = _screen(2, 10, 1, buf)
    s.conflicts = None
    assert call(s) == SMX_E_ARG and b"conf_off" in lib.smx_last_error()
    s.conf_off = None
    assert call(s, ws, need.value - 1) == SMX_E_WORKSPACE
    assert call(None) == SMX_E_ARG
    # the columns may be null when there are no ops
    s = _screen(2, 0, 1, buf)
    for fname in ("kind", "ts", "oid_hi", "oid_lo", "sym", "v0"):
        setattr(s, fname, None)
    assert call(s, ws, 0) == SMX_E_WORKSPACE
    # a short or missing workspace
    s = _screen(2, 10, 1, buf)
    assert call(s, ws, need.value - 1) == SMX_E_WORKSPACE
    assert call(s, None, 8192) == SMX_E_WORKSPACE
    assert b"workspace" in lib.smx_last_error()


def test_no_pairs_or_no_logs_is_ok(lib):
    assert lib.smx_screen(C.byref(_screen(0, 0, 0, None)), None, 0, None) == SMX_OK
    buf = (C.c_uint8 * 64)()
    assert lib.smx_screen(C.byref(_screen(3, 10, 0, buf)), None, 0, None) == SMX_OK
    assert lib.smx_screen(C.byref(_screen(0, 10, 5, buf)), None, 0, None) == SMX_OK
