"""smx_compose_pairs' C ABI without a GPU: the ctypes mirror of smx_pairs has the header's
layout, the library exports and declares the two symbols, an unknown flag is refused before any
other check, the workspace query is monotone in its arguments and larger with SMX_BATCH_LARGE,
and every argument and workspace error comes back before any HIP call, on host pointers."""
import ctypes as C
import os

import pytest

from semantic_merge_amd import _abi
from semantic_merge_amd._lib import LIB_PATH

from _util import assert_header_layout

SMX_OK, SMX_E_ARG, SMX_E_WORKSPACE = 0, -1, -4
LARGE = _abi.BATCH_LARGE
LIM = (1 << 31) - 1
N_PTR = 18  # the pointers of smx_pairs


def test_smx_pairs_matches_header():
    assert_header_layout({"smx_pairs": _abi.SmxPairs})
    assert [f for f, _ in _abi.SmxPairs._fields_][:5] == ["n_logs", "n_total", "n_pairs", "n_sym", "n_out"]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB_PATH), "build libsmx.so first (__graft_entry__.build())"
    return _abi.declare(C.CDLL(LIB_PATH))


def _pairs(buf, n_logs=2, n_total=10, n_pairs=3, n_out=30):
    """A struct whose every pointer is the (host) buffer `buf`: the calls below fail before
    anything reads it."""
    p = C.addressof(buf) if buf is not None else 0
    return _abi.SmxPairs(n_logs, n_total, n_pairs, 4, n_out, *([p] * N_PTR), 0)


def test_symbols_exported_and_declared(lib):
    for name in ("smx_compose_pairs_workspace_bytes", "smx_compose_pairs"):
        assert name in _abi.EXPORTS
        assert hasattr(lib, name), name
    assert lib.smx_compose_pairs.argtypes == [C.POINTER(_abi.SmxPairs), C.c_void_p, C.c_size_t, C.c_uint32,
                                              C.c_void_p]
    assert lib.smx_compose_pairs_workspace_bytes.argtypes == [C.c_int64, C.c_int64, C.c_int64, C.c_uint32,
                                                              C.POINTER(C.c_size_t)]
    assert sum(ft is C.c_void_p for _, ft in _abi.SmxPairs._fields_) == N_PTR


def test_unknown_flag_is_rejected_first(lib):
    buf = (C.c_uint8 * 4096)()
    ws = (C.c_uint64 * 4096)()
    size = C.c_size_t(0)
    for flags in (2, 3, 4, 1 << 31, 0xFFFFFFFE):
        assert lib.smx_compose_pairs_workspace_bytes(2, 3, 30, flags, C.byref(size)) == SMX_E_ARG, flags
        assert b"flag" in lib.smx_last_error()
        assert lib.smx_compose_pairs_workspace_bytes(-1, 3, 30, flags, None) == SMX_E_ARG
        assert b"flag" in lib.smx_last_error()
        assert lib.smx_compose_pairs(C.byref(_pairs(buf)), ws, 32768, flags, None) == SMX_E_ARG, flags
        assert b"flag" in lib.smx_last_error()
        # (before any other check: a null struct, a negative size, and no pairs, which is valid under known flags)
        assert lib.smx_compose_pairs(None, ws, 32768, flags, None) == SMX_E_ARG and b"flag" in lib.smx_last_error()
        assert lib.smx_compose_pairs(C.byref(_pairs(buf, n_total=-1)), ws, 32768, flags, None) == SMX_E_ARG
        assert b"flag" in lib.smx_last_error()
        assert lib.smx_compose_pairs(C.byref(_pairs(None, 0, 0, 0, 0)), None, 0, flags, None) == SMX_E_ARG, flags


def test_workspace_query(lib):
    a, b = C.c_size_t(0), C.c_size_t(0)

    def q(n_logs, n_pairs, n_out, flags):
        assert lib.smx_compose_pairs_workspace_bytes(n_logs, n_pairs, n_out, flags, C.byref(a)) == SMX_OK
        return a.value

    steps = (0, 1, 63, 64, 65, 1000, 100_001, 1 << 20, LIM)
    for flags in (0, LARGE):
        for fixed in (0, 7, 5000):
            for grow in range(3):
                prev = 0
                for v in steps:
                    args = [fixed] * 3
                    args[grow] = v
                    size = q(*args, flags)
                    assert size >= prev, (flags, args)
                    prev = size
        assert q(1, 1, 1, flags) > 0
        assert q(LIM, 5, 5, flags) > q(1, 5, 5, flags) and q(5, LIM, 5, flags) > q(5, 1, 5, flags)
    # without the flag the size does not depend on n_out; with it, 64 bytes per entry (equal
    # steps of 64 entries, a multiple of every array's alignment, add equal bytes) and 4 per pair more
    assert q(9, 40, 0, 0) == q(9, 40, 1 << 40, 0)
    sizes = [q(9, 40, n, LARGE) for n in (0, 64, 128, 4096, 4160)]
    assert sizes[1] - sizes[0] == sizes[2] - sizes[1] == sizes[4] - sizes[3] == 64 * 64
    assert q(0, 0, 0, LARGE) >= q(0, 0, 0, 0)  # (nothing to add for no pairs and no results)
    for n_logs, n_pairs, n_out in ((3, 1, 0), (1, 0, 1),(9, 40, 1), (9, 40, 5000), (LIM, LIM, LIM)):
        assert q(n_logs, n_pairs, n_out, LARGE) > q(n_logs, n_pairs, n_out, 0), (n_logs, n_pairs, n_out)
    # limits
    for flags in (0, LARGE):
        for args in ((-1, 1, 1), (1 << 31, 1, 1), (1, -1, 1), (1, 1 << 31, 1), (1, 1, -1)):
            assert lib.smx_compose_pairs_workspace_bytes(*args, flags, C.byref(b)) == SMX_E_ARG, args
            assert lib.smx_last_error()
        assert lib.smx_compose_pairs_workspace_bytes(5, 5, 5, flags, None) == SMX_E_ARG
    assert lib.smx_compose_pairs_workspace_bytes(1, 1, 1 << 31, LARGE, C.byref(b)) == SMX_E_ARG
    assert b"n_out" in lib.smx_last_error()
    assert lib.smx_compose_pairs_workspace_bytes(1, 1, LIM, LARGE, C.byref(b)) == SMX_OK


@pytest.mark.parametrize("flags", [0, LARGE])
def test_argument_errors_without_gpu(lib, flags):
    buf = (C.c_uint8 * 4096)()
    ws = (C.c_uint64 * 4096)()
    need = C.c_size_t(0)
    assert lib.smx_compose_pairs_workspace_bytes(2, 3, 30, flags, C.byref(need)) == SMX_OK
    assert 0 < need.value <= 32000

    def run(s, w=ws, nbytes=32768):
        rc = lib.smx_compose_pairs(C.byref(s) if s is not None else None, w, nbytes, flags, None)
        if rc != SMX_OK:
            assert lib.smx_last_error(), "an error code without a message"
        return rc

    # negative sizes, counts past 2^31 - 1, n_sym past 2^32 - 1
    for field, value in (("n_logs", -1), ("n_total", -1), ("n_pairs", -1), ("n_sym", -1), ("n_out", -1),
                         ("grid_cap", -1), ("n_logs", 1 << 31), ("n_pairs", 1 << 31), ("n_sym", 1 << 32)):
        s = _pairs(buf)
        setattr(s, field, value)
        assert run(s) == SMX_E_ARG, (field, value)
    assert b"n_sym" in lib.smx_last_error()
    # the largest n_sym is an argument still: it reaches the workspace check
    s = _pairs(buf)
    s.n_sym = (1 << 32) - 1
    assert run(s, ws, need.value - 1) == SMX_E_WORKSPACE
    # (the limits on n_total and n_out are the flag's: the unflagged call goes on to its workspace check)
    for field in ("n_total", "n_out"):
        s = _pairs(buf)
        setattr(s, field, 1 << 31)
        assert run(s, ws, 32768 if flags else 0) == (SMX_E_ARG if flags else SMX_E_WORKSPACE), field
        if flags:
            assert field.encode() in lib.smx_last_error()
    # a null struct, null pointers all at once, then each pointer alone
    assert run(None) == SMX_E_ARG and run(_pairs(None)) == SMX_E_ARG
    n_ptr = 0
    for fname, ft in _abi.SmxPairs._fields_:
        if ft is C.c_void_p:
            s = _pairs(buf)
            setattr(s, fname, None)
            assert run(s) == SMX_E_ARG, fname
            n_ptr += 1
    assert n_ptr == N_PTR
    # a workspace too small, missing or misaligned; with the flag also the unflagged size
    s = _pairs(buf)
    assert run(s, ws, need.value - 1) == SMX_E_WORKSPACE
    assert run(s, None, 32768) == SMX_E_WORKSPACE
    assert b"workspace" in lib.smx_last_error()
    odd = (C.c_uint8 * 32000).from_address(C.addressof(ws) + 4)
    assert run(s, odd, 32000) == SMX_E_WORKSPACE
    if flags:
        small = C.c_size_t(0)
        assert lib.smx_compose_pairs_workspace_bytes(2, 3, 30, 0, C.byref(small)) == SMX_OK
        assert small.value < need.value and run(s, ws, small.value) == SMX_E_WORKSPACE


@pytest.mark.parametrize("flags", [0, LARGE])
def test_no_pairs_or_no_logs_is_ok(lib, flags):
    assert lib.smx_compose_pairs(C.byref(_pairs(None, 0, 0, 0, 0)), None, 0, flags, None) == SMX_OK
    buf = (C.c_uint8 * 64)()
    assert lib.smx_compose_pairs(C.byref(_pairs(buf, n_pairs=0)), None, 0, flags, None) == SMX_OK
    assert lib.smx_compose_pairs(C.byref(_pairs(buf, n_logs=0)), None, 0, flags, None) == SMX_OK
    assert lib.smx_compose_pairs(C.byref(_pairs(None, 5, 10, 0, 0)), None, 0, flags, None) == SMX_OK
