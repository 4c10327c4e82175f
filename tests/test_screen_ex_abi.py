"""smx_screen_ex's C ABI without a GPU: the library exports and declares the two symbols, an
unknown flag is refused, the workspace query with flags = 0 is smx_screen's, and smx_screen's
argument errors come back before any HIP call with SMX_SCREEN_LARGE set as well."""
import ctypes as C
import os

import pytest

from semantic_merge_amd import _abi
from semantic_merge_amd._lib import LIB_PATH

SMX_OK, SMX_E_ARG, SMX_E_WORKSPACE = 0, -1, -4
LARGE = _abi.SCREEN_LARGE
N_PTR = 12


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB_PATH), "build libsmx.so first (__graft_entry__.build())"
    return _abi.declare(C.CDLL(LIB_PATH))


def _screen(n_logs, n_total, n_pairs, buf):
    """A screen whose every pointer is the (host) buffer `buf`: the calls below fail before
    anything reads it."""
    p = C.addressof(buf) if buf is not None else 0
    return _abi.SmxScreen(n_logs, n_total, n_pairs, *([p] * N_PTR), 0)


def test_symbols_exported_and_declared(lib):
    assert LARGE == 1
    for name in ("smx_screen_ex_workspace_bytes", "smx_screen_ex"):
        assert name in _abi.EXPORTS
        assert hasattr(lib, name), name
    assert lib.smx_screen_ex.argtypes == [C.POINTER(_abi.SmxScreen), C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
    assert lib.smx_screen_ex_workspace_bytes.argtypes[3] is C.c_uint32
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "smx.h")) as fh:
        hdr = fh.read()
    assert "#define SMX_SCREEN_LARGE 1u" in hdr


def test_unknown_flag(lib):
    buf = (C.c_uint8 * 4096)()
    ws = (C.c_uint8 * 8192)()
    size = C.c_size_t(0)
    for flags in (2, 3, 4, 1 << 31, 0xFFFFFFFE):
        assert lib.smx_screen_ex_workspace_bytes(2, 10, 1, flags, C.byref(size)) == SMX_E_ARG, flags
        assert b"flag" in lib.smx_last_error()
        assert lib.smx_screen_ex(C.byref(_screen(2, 10, 1, buf)), ws, 8192, flags, None) == SMX_E_ARG, flags
        assert b"flag" in lib.smx_last_error()
        # (before any other check: a screen of no pairs, which is valid under known flags)
        assert lib.smx_screen_ex(C.byref(_screen(0, 0, 0, None)), None, 0, flags, None) == SMX_E_ARG, flags


def test_workspace_query(lib):
    a, b = C.c_size_t(0), C.c_size_t(0)
    for sizes in ((0, 0, 0), (2, 10, 1), (100, 50_000, 1000), (7, 123_457, 3), (16384, 1 << 22, 1 << 20)):
        assert lib.smx_screen_workspace_bytes(*sizes, C.byref(a)) == SMX_OK
        assert lib.smx_screen_ex_workspace_bytes(*sizes, 0, C.byref(b)) == SMX_OK
        assert a.value == b.value, sizes
        assert lib.smx_screen_ex_workspace_bytes(*sizes, LARGE, C.byref(b)) == SMX_OK
        assert b.value >= a.value, sizes
    prev = 0
    for n_total in (0, 1, 63, 64, 65, 2048, 2049, 100_000, 100_001, 1 << 24, (1 << 31) - 1):
        assert lib.smx_screen_ex_workspace_bytes(10, n_total, 50, LARGE, C.byref(b)) == SMX_OK
        assert b.value >= prev, n_total    # monotone in n_total
        prev = b.value
    assert prev >= ((1 << 31) - 1) * 44    # the records and the two index arrays of the sort
    for args in ((-1, 10, 1), (1, -1, 1), (1, 10, -1), (1 << 31, 10, 1), (1, 10, 1 << 31), (1, 1 << 31, 1)):
        assert lib.smx_screen_ex_workspace_bytes(*args, LARGE, C.byref(b)) == SMX_E_ARG, args
        assert lib.smx_last_error()
    assert lib.smx_screen_ex_workspace_bytes(1, 1 << 31, 1, 0, C.byref(b)) == SMX_OK   # (as smx_screen's)
    assert lib.smx_screen_ex_workspace_bytes(5, 5, 5, LARGE, None) == SMX_E_ARG


@pytest.mark.parametrize("flags", [0, LARGE])
def test_argument_errors_without_gpu(lib, flags):
    buf = (C.c_uint8 * 4096)()
    ws = (C.c_uint8 * 8192)()
    need = C.c_size_t(0)
    assert lib.smx_screen_ex_workspace_bytes(2, 10, 1, flags, C.byref(need)) == SMX_OK
    assert 0 < need.value <= 8000

    def call(s, w=ws, nbytes=8192):
        rc = lib.smx_screen_ex(C.byref(s) if s is not None else None, w, nbytes, flags, None)
        if rc != SMX_OK:
            assert lib.smx_last_error(), "an error code without a message"
        return rc

    # negative sizes
    for s in (_screen(-1, 10, 1, buf), _screen(2, -1, 1, buf), _screen(2, 10, -1, buf)):
        assert call(s) == SMX_E_ARG
    s = _screen(2, 10, 1, buf)
    s.grid_cap = -1
    assert call(s) == SMX_E_ARG
    if flags:
        assert call(_screen(2, 1 << 31, 1, buf)) == SMX_E_ARG and b"n_total" in lib.smx_last_error()
    # null pointers: all of them, then each alone
    assert call(_screen(2, 10, 1, None)) == SMX_E_ARG
    for fname, ft in _abi.SmxScreen._fields_:
        if ft is C.c_void_p:
            s = _screen(2, 10, 1, buf)
            setattr(s, fname, None)
            assert call(s) == SMX_E_ARG, fname   # (conflicts / conf_off: exactly one of them null)
    assert call(None) == SMX_E_ARG
    # conflicts and conf_off both null is valid: the call goes on to the workspace check
    s = _screen(2, 10, 1, buf)
    s.conflicts = s.conf_off = None
    assert call(s, ws, need.value - 1) == SMX_E_WORKSPACE
    # a workspace too small, missing or misaligned
    s = _screen(2, 10, 1, buf)
    assert call(s, ws, need.value - 1) == SMX_E_WORKSPACE
    assert call(s, None, 8192) == SMX_E_WORKSPACE
    base = C.addressof(ws)
    odd = (C.c_uint8 * 8000).from_address(base + (8 - base % 8) % 8 + 4)
    assert call(s, odd, 8000) == SMX_E_WORKSPACE
    assert b"workspace" in lib.smx_last_error()
    if flags:   # what smx_screen asks for does not do for the large mode
        small = C.c_size_t(0)
        assert lib.smx_screen_workspace_bytes(2, 10, 1, C.byref(small)) == SMX_OK
        assert small.value < need.value and call(s, ws, small.value) == SMX_E_WORKSPACE


@pytest.mark.parametrize("flags", [0, LARGE])
def test_no_pairs_or_no_logs_is_ok(lib, flags):
    assert lib.smx_screen_ex(C.byref(_screen(0, 0, 0, None)), None, 0, flags, None) == SMX_OK
    buf = (C.c_uint8 * 64)()
    assert lib.smx_screen_ex(C.byref(_screen(3, 10, 0, buf)), None, 0, flags, None) == SMX_OK
    assert lib.smx_screen_ex(C.byref(_screen(0, 10, 5, buf)), None, 0, flags, None) == SMX_OK
