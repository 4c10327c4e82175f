"""smx_screen_candidates' C ABI without a GPU: the ctypes mirror of smx_candidates has the
header's layout, the library exports the new symbols, and the argument errors come back before
any HIP call."""
import ctypes as C
import os

import pytest

from semantic_merge_amd import _abi
from semantic_merge_amd._lib import LIB_PATH

from _util import assert_header_layout

SMX_OK, SMX_E_ARG, SMX_E_WORKSPACE = 0, -1, -4


def test_smx_candidates_matches_header():
    assert_header_layout({"struct smx_candidates": _abi.SmxCandidates})


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB_PATH), "build libsmx.so first (__graft_entry__.build())"
    return _abi.declare(C.CDLL(LIB_PATH))


def test_symbols_exported(lib):
    for name in ("smx_screen_candidates_workspace_bytes", "smx_screen_candidates"):
        assert name in _abi.EXPORTS
        assert hasattr(lib, name), name
    assert lib.smx_screen_candidates.argtypes[0] is C.POINTER(_abi.SmxCandidates)
    assert _abi.CAND_MAX_LOGS == 16384


def test_workspace_query(lib):
    size = C.c_size_t(0)
    assert lib.smx_screen_candidates_workspace_bytes(100, 50_000, C.byref(size)) == SMX_OK
    # two key arrays and two value arrays for the sort, and a bit per pair of logs
    assert size.value >= 50_000 * 24 + 100 * 100 // 8
    small = size.value
    assert lib.smx_screen_candidates_workspace_bytes(_abi.CAND_MAX_LOGS, 50_000, C.byref(size)) == SMX_OK
    assert size.value >= small + _abi.CAND_MAX_LOGS ** 2 // 8
    for args in ((-1, 10), (1, -1), (_abi.CAND_MAX_LOGS + 1, 10), (1, 1 << 31)):
        assert lib.smx_screen_candidates_workspace_bytes(*args, C.byref(size)) == SMX_E_ARG, args
        assert lib.smx_last_error()
    assert lib.smx_screen_candidates_workspace_bytes(5, 5, None) == SMX_E_ARG
    assert lib.smx_screen_candidates_workspace_bytes(0, 0, C.byref(size)) == SMX_OK


PTRS = ("log_off", "kind", "sym", "v0", "pair_a", "pair_b", "counts", "log_info")


def _cand(n_logs, n_total, pair_cap, buf):
    """A call whose every pointer is the (host) buffer `buf`: the calls below fail before
    anything reads it."""
    p = C.addressof(buf) if buf is not None else 0
    c = _abi.SmxCandidates(n_logs, n_total)
    for name in PTRS:
        setattr(c, name, p)
    c.pair_cap = pair_cap
    return c


def test_argument_errors_without_gpu(lib):
    assert [f for f, t in _abi.SmxCandidates._fields_ if t is C.c_void_p] == list(PTRS)
    buf = (C.c_uint8 * 4096)()
    ws = (C.c_uint64 * 2048)()   # (8-byte aligned)
    nbytes = 8 * 2048
    need = C.c_size_t(0)
    assert lib.smx_screen_candidates_workspace_bytes(2, 10, C.byref(need)) == SMX_OK
    assert 0 < need.value <= nbytes

    def call(c, w=ws, n=nbytes):
        rc = lib.smx_screen_candidates(C.byref(c) if c is not None else None, w, n, None)
        if rc != SMX_OK:
            assert lib.smx_last_error(), "an error code without a message"
        return rc

    assert call(None) == SMX_E_ARG
    # negative sizes, too many logs, too many ops
    for c in (_cand(-1, 10, 4, buf), _cand(2, -1, 4, buf), _cand(2, 10, -1, buf),
              _cand(_abi.CAND_MAX_LOGS + 1, 10, 4, buf), _cand(2, 1 << 31, 4, buf)):
        assert call(c) == SMX_E_ARG
    c = _cand(2, 10, 4, buf)
    c.grid_cap = -1
    assert call(c) == SMX_E_ARG
    # every pointer null; then each alone: only log_info may be null
    assert call(_cand(2, 10, 4, None)) == SMX_E_ARG
    for name in PTRS:
        c = _cand(2, 10, 4, buf)
        setattr(c, name, None)
        assert call(c, ws, need.value - 1) == (SMX_E_WORKSPACE if name == "log_info" else SMX_E_ARG), name
    # the pair arrays may be null with pair_cap = 0, one of them or both; the columns with no ops:
    # those calls go on to the workspace check, which fails before any HIP call
    for names in (("pair_a",), ("pair_b",), ("pair_a", "pair_b")):
        c = _cand(2, 10, 0, buf)
        for name in names:
            setattr(c, name, None)
        assert call(c, ws, need.value - 1) == SMX_E_WORKSPACE
    c = _cand(2, 0, 4, buf)
    for name in ("kind", "sym", "v0"):
        setattr(c, name, None)
    assert call(c, ws, 0) == SMX_E_WORKSPACE
    # a short, missing or misaligned workspace
    c = _cand(2, 10, 4, buf)
    assert call(c, ws, need.value - 1) == SMX_E_WORKSPACE
    assert call(c, None, nbytes) == SMX_E_WORKSPACE
    assert b"workspace" in lib.smx_last_error()
    assert call(c, C.c_void_p(C.addressof(ws) + 4), nbytes - 8) == SMX_E_WORKSPACE


def test_no_logs_is_ok(lib):
    assert lib.smx_screen_candidates(C.byref(_cand(0, 0, 0, None)), None, 0, None) == SMX_OK
    buf = (C.c_uint8 * 64)()
    assert lib.smx_screen_candidates(C.byref(_cand(0, 10, 5, buf)), None, 0, None) == SMX_OK
