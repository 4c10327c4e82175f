"""smx_screen_tree's C ABI without a GPU: the ctypes mirror of smx_screen_tree has the header's
layout, the library exports and declares the two symbols, a non-zero flag is refused before any
other check, the workspace query is monotone, 8-byte aligned and the documented formula, and every
argument and workspace error comes back before any HIP call, on host pointers."""
import ctypes as C
import os

import pytest

from semantic_merge_amd import _abi
from semantic_merge_amd._lib import LIB_PATH

from _util import assert_header_layout

SMX_OK, SMX_E_ARG, SMX_E_WORKSPACE = 0, -1, -4
LIM = (1 << 31) - 1
N_PTR = 14  # the pointers of smx_screen_tree
SIZES = ("n_logs", "n_total", "n_nodes", "n_levels", "n_acc")
WIDE = ("n_logs", "n_total", "n_nodes", "n_acc")  # the sizes that reach 2^31 - 1


def test_smx_screen_tree_matches_header():
    assert_header_layout({"struct smx_screen_tree": _abi.SmxScreenTree})
    assert [f for f, _ in _abi.SmxScreenTree._fields_][:5] == list(SIZES)
    assert sum(ft is C.c_void_p for _, ft in _abi.SmxScreenTree._fields_) == N_PTR


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB_PATH), "build libsmx.so first (__graft_entry__.build())"
    return _abi.declare(C.CDLL(LIB_PATH))


def _tree(buf, n_logs=2, n_total=10, n_nodes=3, n_levels=2, n_acc=12):
    """A struct whose every pointer is the (host) buffer `buf`: the calls below fail before
    anything reads it."""
    p = C.addressof(buf) if buf is not None else 0
    return _abi.SmxScreenTree(n_logs, n_total, n_nodes, n_levels, n_acc, *([p] * N_PTR), 0)


def test_symbols_exported_and_declared(lib):
    for name in ("smx_screen_tree_workspace_bytes", "smx_screen_tree"):
        assert name in _abi.EXPORTS
        assert hasattr(lib, name), name
    assert lib.smx_screen_tree.argtypes == [C.POINTER(_abi.SmxScreenTree), C.c_void_p, C.c_size_t, C.c_uint32,
                                            C.c_void_p]
    assert lib.smx_screen_tree_workspace_bytes.argtypes == [C.c_int64] * 5 + [C.c_uint32, C.POINTER(C.c_size_t)]


def test_a_flag_is_rejected_first(lib):
    buf = (C.c_uint8 * 4096)()
    ws = (C.c_uint64 * 8192)()
    size = C.c_size_t(0)
    for flags in (1, 2, 1 << 31, 0xFFFFFFFF):
        assert lib.smx_screen_tree_workspace_bytes(2, 10, 3, 2, 12, flags, C.byref(size)) == SMX_E_ARG, flags
        assert b"flag" in lib.smx_last_error()
        assert lib.smx_screen_tree_workspace_bytes(-1, 10, 3, 2, 12, flags, None) == SMX_E_ARG
        assert b"flag" in lib.smx_last_error()
        for s in (_tree(buf), None, _tree(buf, n_total=-1), _tree(None, 0, 0, 0, 0, 0)):
            assert lib.smx_screen_tree(C.byref(s) if s is not None else None, ws, 65536, flags, None) == SMX_E_ARG
            assert b"flag" in lib.smx_last_error()


def test_workspace_query_is_monotone_and_the_documented_formula(lib):
    a = C.c_size_t(0)

    def q(*sizes):
        assert lib.smx_screen_tree_workspace_bytes(*sizes, 0, C.byref(a)) == SMX_OK
        assert a.value % 8 == 0, sizes
        return a.value

    def al(x):
        return (x + 255) & ~255

    def formula(L, T, N, D, A):
        """include/smx.h: every part rounded up to 256 bytes."""
        screen = 256 + al(4 * L) + 3 * al(4 * N) + 3 * al(8 * (T + A)) + 3 * al(4 * (T + A))
        return screen + al(8 * N) + 2 * al(4 * N) + al(4 * D) + al(16 * D) + 2 * al(4 * T)

    steps = (0, 1, 63, 64, 65, 1000, 2049, 100_001, 1 << 20, LIM)
    for fixed in (0, 7, 3000):
        for grow in range(5):
            prev = 0
            for v in steps:
                if grow == 3 and v > _abi.TREE_MAX_LEVELS:
                    continue
                args = [fixed] * 5
                args[grow] = v
                size = q(*args)
                assert size >= prev, args
                assert size == formula(*args), args
                prev = size
    assert q(1, 1, 1, 1, 1) > 0
    # equal steps of 64 entries add equal bytes: 4 per log, 28 per node (three class lists, two
    # verdicts of 4 and 8 bytes, acc_node), 20 per level, 44 per op (36 of records, the large sort's
    # two index arrays) and 36 per entry of n_acc (one buffer of records)
    base = q(64, 64, 64, 64, 64)
    assert q(128, 64, 64, 64, 64) - base == 4 * 64
    assert q(64, 128, 64, 64, 64) - base == q(64, 192, 64, 64, 64) - q(64, 128, 64, 64, 64) == 44 * 64
    assert q(64, 64, 128, 64, 64) - base == 28 * 64
    assert q(64, 64, 64, 128, 64) - base == 20 * 64
    assert q(64, 64, 64, 64, 128) - base == q(64, 64, 64, 64, 192) - q(64, 64, 64, 64, 128) == 36 * 64
    for bad in (-1, 1 << 31):
        for at in range(5):
            args = [1] * 5
            args[at] = bad
            assert lib.smx_screen_tree_workspace_bytes(*args, 0, C.byref(a)) == SMX_E_ARG, args
            assert lib.smx_last_error()
    assert lib.smx_screen_tree_workspace_bytes(1, 1, 1, _abi.TREE_MAX_LEVELS + 1, 1, 0, C.byref(a)) == SMX_E_ARG
    assert q(1, 1, 1, _abi.TREE_MAX_LEVELS, 1) > 0
    assert lib.smx_screen_tree_workspace_bytes(5, 5, 5, 5, 5, 0, None) == SMX_E_ARG
    assert q(LIM, LIM, LIM, _abi.TREE_MAX_LEVELS, LIM) >= 44 * LIM + 36 * LIM + 28 * LIM


def test_argument_errors_without_gpu(lib):
    buf = (C.c_uint8 * 4096)()
    ws = (C.c_uint64 * 8192)()
    need = C.c_size_t(0)
    assert lib.smx_screen_tree_workspace_bytes(2, 10, 3, 2, 12, 0, C.byref(need)) == SMX_OK
    assert 0 < need.value <= 65000

    def run(s, w=ws, nbytes=65536):
        rc = lib.smx_screen_tree(C.byref(s) if s is not None else None, w, nbytes, 0, None)
        if rc != SMX_OK:
            assert lib.smx_last_error(), "an error code without a message"
        return rc

    # negative sizes, sizes past 2^31 - 1, too many levels, a negative grid_cap
    for field, value in [(f, -1) for f in SIZES] + [("grid_cap", -1)] + [(f, 1 << 31) for f in WIDE] + \
            [("n_levels", _abi.TREE_MAX_LEVELS + 1)]:
        s = _tree(buf)
        setattr(s, field, value)
        assert run(s) == SMX_E_ARG, (field, value)
    # a null struct, null pointers all at once, then each pointer alone (conflicts / conf_off:
    # exactly one of them null)
    assert run(None) == SMX_E_ARG and run(_tree(None)) == SMX_E_ARG
    n_ptr = 0
    for fname, ft in _abi.SmxScreenTree._fields_:
        if ft is C.c_void_p:
            s = _tree(buf)
            setattr(s, fname, None)
            assert run(s) == SMX_E_ARG, fname
            n_ptr += 1
    assert n_ptr == N_PTR
    # conflicts and conf_off both null is valid: the call goes on to the workspace check; so do a
    # null log_off without logs and null columns without ops
    s = _tree(buf)
    s.conflicts = s.conf_off = None
    assert run(s, ws, need.value - 1) == SMX_E_WORKSPACE
    s = _tree(buf, n_logs=0, n_total=0)
    for f in ("log_off", "kind", "ts", "oid_hi", "oid_lo", "sym", "v0"):
        setattr(s, f, None)
    assert run(s, ws, 8) == SMX_E_WORKSPACE
    # a workspace too small, missing or misaligned
    s = _tree(buf)
    assert run(s, ws, need.value - 1) == SMX_E_WORKSPACE
    assert run(s, None, 65536) == SMX_E_WORKSPACE
    assert b"workspace" in lib.smx_last_error()
    odd = (C.c_uint8 * 65000).from_address(C.addressof(ws) + 4)
    assert run(s, odd, 65000) == SMX_E_WORKSPACE
    # the most levels are accepted as far as the workspace check
    assert run(_tree(buf, n_levels=_abi.TREE_MAX_LEVELS), ws, 8) == SMX_E_WORKSPACE


def test_no_nodes_is_ok(lib):
    assert lib.smx_screen_tree(C.byref(_tree(None, 0, 0, 0, 0, 0)), None, 0, 0, None) == SMX_OK
    buf = (C.c_uint8 * 64)()
    assert lib.smx_screen_tree(C.byref(_tree(buf, n_nodes=0)), None, 0, 0, None) == SMX_OK
    assert lib.smx_screen_tree(C.byref(_tree(None, 5, 10, 0, 3, 0)), None, 0, 0, None) == SMX_OK
