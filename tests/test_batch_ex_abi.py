"""smx_compose_batch_ex / smx_compose_batch_shared_ex's C ABI without a GPU: the library exports
and declares the four symbols, an unknown flag is refused before any other check, the workspace
queries with flags = 0 are the unflagged ones, the flagged size is linear in n_total, and the
argument errors come back before any HIP call with SMX_BATCH_LARGE set as well."""
import ctypes as C
import os

import pytest

from semantic_merge_amd import _abi
from semantic_merge_amd._lib import LIB_PATH

SMX_OK, SMX_E_ARG, SMX_E_WORKSPACE = 0, -1, -4
LARGE = _abi.BATCH_LARGE
LIM = (1 << 31) - 1


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB_PATH), "build libsmx.so first (__graft_entry__.build())"
    return _abi.declare(C.CDLL(LIB_PATH))


def _batch(n_merges, n_total, buf):
    p = C.addressof(buf) if buf is not None else 0
    return _abi.SmxBatch(n_merges, n_total, 4, *([p] * 16), 0)


def _shared(n_merges, n_total, n_shared, buf):
    p = C.addressof(buf) if buf is not None else 0
    return _abi.SmxBatchShared(n_merges, n_total, 4, n_shared, *([p] * 15), 0, 0)


def _calls(lib):
    """(call, query, struct maker) of the plain and of the shared form, on 3 merges of 10 ops."""
    return ((lib.smx_compose_batch_ex, lambda f, out: lib.smx_compose_batch_ex_workspace_bytes(3, 10, f, out),
             lambda buf, m=3, n=10: _batch(m, n, buf)),
            (lib.smx_compose_batch_shared_ex,
             lambda f, out: lib.smx_compose_batch_shared_ex_workspace_bytes(3, 10, 4, f, out),
             lambda buf, m=3, n=10: _shared(m, n, 4 if n >= 4 else 0, buf)))


def test_symbols_exported_and_declared(lib):
    assert LARGE == 1
    for name in ("smx_compose_batch_ex_workspace_bytes", "smx_compose_batch_ex",
                 "smx_compose_batch_shared_ex_workspace_bytes", "smx_compose_batch_shared_ex"):
        assert name in _abi.EXPORTS
        assert hasattr(lib, name), name
    assert lib.smx_compose_batch_ex.argtypes == [C.POINTER(_abi.SmxBatch), C.c_void_p, C.c_size_t, C.c_uint32,
                                                 C.c_void_p]
    assert lib.smx_compose_batch_shared_ex.argtypes == [C.POINTER(_abi.SmxBatchShared), C.c_void_p, C.c_size_t,
                                                        C.c_uint32, C.c_void_p]
    assert lib.smx_compose_batch_ex_workspace_bytes.argtypes[2] is C.c_uint32
    assert lib.smx_compose_batch_shared_ex_workspace_bytes.argtypes[3] is C.c_uint32
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "smx.h")) as fh:
        assert "#define SMX_BATCH_LARGE 1u" in fh.read()


def test_unknown_flag(lib):
    buf = (C.c_uint8 * 4096)()
    ws = (C.c_uint64 * 4096)()
    size = C.c_size_t(0)
    for flags in (2, 3, 4, 1 << 31, 0xFFFFFFFE):
        for call, query, make in _calls(lib):
            assert query(flags, C.byref(size)) == SMX_E_ARG, flags
            assert b"flag" in lib.smx_last_error()
            assert call(C.byref(make(buf)), ws, 32768, flags, None) == SMX_E_ARG, flags
            assert b"flag" in lib.smx_last_error()
            # (before any other check: a null batch, and a batch of no merges, which is valid under known flags)
            assert call(None, ws, 32768, flags, None) == SMX_E_ARG and b"flag" in lib.smx_last_error()
            assert call(C.byref(make(None, 0, 0)), None, 0, flags, None) == SMX_E_ARG, flags
        assert lib.smx_compose_batch_ex_workspace_bytes(-1, 10, flags, None) == SMX_E_ARG
        assert b"flag" in lib.smx_last_error()


def test_workspace_query(lib):
    a, b, c = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    for m in (0, 1, 63, 64, 65, 1000, 1 << 20, LIM):
        for n_total in (0, 10, 1 << 40):  # (the unflagged size does not depend on n_total)
            assert lib.smx_compose_batch_workspace_bytes(m, C.byref(a)) == SMX_OK
            assert lib.smx_compose_batch_ex_workspace_bytes(m, n_total, 0, C.byref(b)) == SMX_OK
            assert a.value == b.value, m
            assert lib.smx_compose_batch_shared_workspace_bytes(m, C.byref(a)) == SMX_OK
            assert lib.smx_compose_batch_shared_ex_workspace_bytes(m, n_total, 0, 0, C.byref(b)) == SMX_OK
            assert a.value == b.value, m
    # flagged: at least the unflagged size, and linear in n_total: equal steps of 64 ops (a
    # multiple of every array's alignment) add equal bytes, 64 per op
    assert lib.smx_compose_batch_workspace_bytes(7, C.byref(a)) == SMX_OK
    sizes = []
    for n_total in (0, 64, 128, 4096, 4160, 1 << 24, (1 << 24) + 64):
        assert lib.smx_compose_batch_ex_workspace_bytes(7, n_total, LARGE, C.byref(b)) == SMX_OK
        assert b.value >= a.value
        sizes.append(b.value)
    assert sizes[1] - sizes[0] == sizes[2] - sizes[1] == sizes[4] - sizes[3] == sizes[6] - sizes[5] == 64 * 64
    assert sizes[5] - sizes[0] == (1 << 24) * 64
    prev = 0
    for n_total in (0, 1, 63, 65, 2048, 2049, 100_001, LIM):
        assert lib.smx_compose_batch_ex_workspace_bytes(10, n_total, LARGE, C.byref(b)) == SMX_OK
        assert b.value >= prev and b.value <= a.value + 4096 + 64 * n_total + 5 * 256  # (linear: no more than 64 per op)
        prev = b.value
    # the shared form is sized by its results: n_out = n_total - n_shared + n_merges * n_shared
    assert lib.smx_compose_batch_shared_ex_workspace_bytes(8, 2100 + 800, 2100, LARGE, C.byref(b)) == SMX_OK
    assert lib.smx_compose_batch_ex_workspace_bytes(8, 800 + 8 * 2100, LARGE, C.byref(c)) == SMX_OK
    assert b.value == c.value
    # limits
    for args in ((-1, 10), (1 << 31, 10), (1, -1), (1, 1 << 31), (1, 1 << 40)):
        assert lib.smx_compose_batch_ex_workspace_bytes(*args, LARGE, C.byref(b)) == SMX_E_ARG, args
        assert lib.smx_last_error()
    assert lib.smx_compose_batch_ex_workspace_bytes(1, LIM, LARGE, C.byref(b)) == SMX_OK
    for args in ((1, 1 << 31, 0), (1, 10, 11), (1, 10, -1), (3, 1 << 30, 1 << 30), (-1, 10, 1)):
        assert lib.smx_compose_batch_shared_ex_workspace_bytes(*args, LARGE, C.byref(b)) == SMX_E_ARG, args
    assert lib.smx_compose_batch_ex_workspace_bytes(5, 5, LARGE, None) == SMX_E_ARG
    assert lib.smx_compose_batch_shared_ex_workspace_bytes(5, 5, 1, LARGE, None) == SMX_E_ARG


@pytest.mark.parametrize("flags", [0, LARGE])
def test_argument_errors_without_gpu(lib, flags):
    buf = (C.c_uint8 * 4096)()
    ws = (C.c_uint64 * 4096)()
    for call, query, make in _calls(lib):
        need = C.c_size_t(0)
        assert query(flags, C.byref(need)) == SMX_OK
        assert 0 < need.value <= 32000

        def run(s, w=ws, nbytes=32768):
            rc = call(C.byref(s) if s is not None else None, w, nbytes, flags, None)
            if rc != SMX_OK:
                assert lib.smx_last_error(), "an error code without a message"
            return rc

        assert run(make(buf, -1)) == SMX_E_ARG and run(make(buf, 3, -1)) == SMX_E_ARG
        s = make(buf)
        s.grid_cap = -1
        assert run(s) == SMX_E_ARG
        s = make(buf)
        s.n_sym = 1 << 32
        assert run(s) == SMX_E_ARG
        # (the limit is the flag's: the unflagged call goes on to its workspace check)
        assert run(make(buf, 3, 1 << 31), ws, 32768 if flags else 0) == (SMX_E_ARG if flags else SMX_E_WORKSPACE)
        if flags:
            assert b"n_total" in lib.smx_last_error()
        assert run(make(None)) == SMX_E_ARG and run(None) == SMX_E_ARG
        for fname, ft in type(make(buf))._fields_:
            if ft is C.c_void_p:
                s = make(buf)
                setattr(s, fname, None)
                assert run(s) == SMX_E_ARG, fname
        # a workspace too small or missing; with the flag also a misaligned one, and the unflagged size
        s = make(buf)
        assert run(s, ws, need.value - 1) == SMX_E_WORKSPACE
        assert run(s, None, 32768) == SMX_E_WORKSPACE
        assert b"workspace" in lib.smx_last_error()
        if flags:
            base = C.addressof(ws)
            odd = (C.c_uint8 * 32000).from_address(base + 4)
            assert run(s, odd, 32000) == SMX_E_WORKSPACE
            small = C.c_size_t(0)
            assert query(0, C.byref(small)) == SMX_OK
            assert small.value < need.value and run(s, ws, small.value) == SMX_E_WORKSPACE
    # the shared form's result size has the limit too: 3 merges against 2^30 shared ops
    if flags:
        s = _shared(3, (1 << 30) + 10, 1 << 30, buf)
        assert lib.smx_compose_batch_shared_ex(C.byref(s), ws, 32768, flags, None) == SMX_E_ARG


@pytest.mark.parametrize("flags", [0, LARGE])
def test_no_merges_is_ok(lib, flags):
    assert lib.smx_compose_batch_ex(C.byref(_batch(0, 0, None)), None, 0, flags, None) == SMX_OK
    assert lib.smx_compose_batch_shared_ex(C.byref(_shared(0, 0, 0, None)), None, 0, flags, None) == SMX_OK
    buf = (C.c_uint8 * 64)()
    assert lib.smx_compose_batch_ex(C.byref(_batch(0, 10, buf)), None, 0, flags, None) == SMX_OK
    assert lib.smx_compose_batch_shared_ex(C.byref(_shared(0, 10, 4, buf)), None, 0, flags, None) == SMX_OK
