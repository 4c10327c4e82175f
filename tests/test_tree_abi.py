"""smx_compose_tree's C ABI without a GPU: the ctypes mirror of smx_tree has the header's layout,
the library exports and declares the two symbols, a non-zero flag is refused before any other
check, n_levels over SMX_TREE_MAX_LEVELS is an argument error, the workspace query is monotone,
linear and 8-byte aligned, and every argument and workspace error comes back before any HIP
call, on host pointers."""
import ctypes as C
import os

import pytest

from semantic_merge_amd import _abi
from semantic_merge_amd._lib import LIB_PATH

from _util import assert_header_layout

SMX_OK, SMX_E_ARG, SMX_E_WORKSPACE = 0, -1, -4
LIM = (1 << 31) - 1
N_PTR = 21  # the pointers of smx_tree
SIZES = ("n_logs", "n_total", "n_nodes", "n_levels", "n_sym", "n_out")
MAXL = 4096


def test_smx_tree_matches_header():
    assert_header_layout({"smx_tree": _abi.SmxTree})
    assert [f for f, _ in _abi.SmxTree._fields_][:6] == list(SIZES)
    assert sum(ft is C.c_void_p for _, ft in _abi.SmxTree._fields_) == N_PTR
    assert _abi.TREE_MAX_LEVELS == MAXL
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "smx.h")) as fh:
        assert f"#define SMX_TREE_MAX_LEVELS {MAXL}\n" in fh.read()


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB_PATH), "build libsmx.so first (__graft_entry__.build())"
    return _abi.declare(C.CDLL(LIB_PATH))


def _tree(buf, n_logs=2, n_total=10, n_nodes=5, n_levels=3, n_out=30, empty_str=-1):
    """A struct whose every pointer is the (host) buffer `buf`: the calls below fail before
    anything reads it."""
    p = C.addressof(buf) if buf is not None else 0
    return _abi.SmxTree(n_logs, n_total, n_nodes, n_levels, 4, n_out, *([p] * N_PTR), 0, empty_str)


def test_symbols_exported_and_declared(lib):
    for name in ("smx_compose_tree_workspace_bytes", "smx_compose_tree"):
        assert name in _abi.EXPORTS
        assert hasattr(lib, name), name
    assert lib.smx_compose_tree.argtypes == [C.POINTER(_abi.SmxTree), C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
    assert lib.smx_compose_tree_workspace_bytes.argtypes == [C.c_int64] * 4 + [C.c_uint32, C.POINTER(C.c_size_t)]


def test_a_flag_is_rejected_first(lib):
    buf = (C.c_uint8 * 4096)()
    ws = (C.c_uint64 * 8192)()
    size = C.c_size_t(0)
    for flags in (1, 2, 1 << 31, 0xFFFFFFFF):
        assert lib.smx_compose_tree_workspace_bytes(2, 5, 3, 30, flags, C.byref(size)) == SMX_E_ARG, flags
        assert b"flag" in lib.smx_last_error()
        assert lib.smx_compose_tree_workspace_bytes(-1, 5, 3, 30, flags, None) == SMX_E_ARG
        assert b"flag" in lib.smx_last_error()
        for s in (_tree(buf), None, _tree(buf, n_total=-1), _tree(buf, n_levels=MAXL + 1), _tree(None, 0, 0, 0, 0, 0)):
            assert lib.smx_compose_tree(C.byref(s) if s is not None else None, ws, 65536, flags, None) == SMX_E_ARG
            assert b"flag" in lib.smx_last_error()


def test_workspace_query_is_monotone_and_aligned(lib):
    a = C.c_size_t(0)

    def q(n_logs, n_nodes, n_levels, n_out):
        assert lib.smx_compose_tree_workspace_bytes(n_logs, n_nodes, n_levels, n_out, 0, C.byref(a)) == SMX_OK
        assert a.value % 8 == 0
        return a.value

    steps = (0, 1, 63, 64, 65, 1000, 100_001, 1 << 20, LIM)
    for fixed in (0, 7, 3000):
        for grow in range(4):
            prev = 0
            for v in steps:
                if grow == 2 and v > MAXL:
                    continue
                args = [fixed] * 4
                args[grow] = v
                size = q(*args)
                assert size >= prev, args
                prev = size
    assert q(1, 1, 1, 1) > 0
    # equal steps of 64 entries (a multiple of every array's alignment) add equal bytes: 4 per log,
    # 20 per node, 20 per level and 57 per entry of n_out -- no state buffers
    base = q(64, 64, 64, 64)
    assert q(128, 64, 64, 64) - base == q(192, 64, 64, 64) - q(128, 64, 64, 64) == 4 * 64
    assert q(64, 128, 64, 64) - base == q(64, 192, 64, 64) - q(64, 128, 64, 64) == 20 * 64
    assert q(64, 64, 128, 64) - base == q(64, 64, 192, 64) - q(64, 64, 128, 64) == 20 * 64
    assert q(64, 64, 64, 320) - base == q(64, 64, 64, 576) - q(64, 64, 64, 320) == 57 * 256
    # less per entry than smx_compose_train, which keeps two state buffers
    assert lib.smx_compose_train_workspace_bytes(64, 64, 64, 1 << 20, 0, C.byref(a)) == SMX_OK
    train = a.value
    assert q(64, 64, 64, 1 << 20) < train
    for args in ((-1, 1, 1, 1), (1 << 31, 1, 1, 1), (1, -1, 1, 1), (1, 1 << 31, 1, 1), (1, 1, -1, 1), (1, 1, MAXL + 1, 1),
                 (1, 1, 1, -1), (1, 1, 1, 1 << 31)):
        assert lib.smx_compose_tree_workspace_bytes(*args, 0, C.byref(a)) == SMX_E_ARG, args
        assert lib.smx_last_error()
    assert lib.smx_compose_tree_workspace_bytes(5, 5, 5, 5, 0, None) == SMX_E_ARG
    assert lib.smx_compose_tree_workspace_bytes(LIM, LIM, MAXL, LIM, 0, C.byref(a)) == SMX_OK


def test_argument_errors_without_gpu(lib):
    buf = (C.c_uint8 * 4096)()
    ws = (C.c_uint64 * 8192)()
    need = C.c_size_t(0)
    assert lib.smx_compose_tree_workspace_bytes(2, 5, 3, 30, 0, C.byref(need)) == SMX_OK
    assert 0 < need.value <= 65000

    def run(s, w=ws, nbytes=65536):
        rc = lib.smx_compose_tree(C.byref(s) if s is not None else None, w, nbytes, 0, None)
        if rc != SMX_OK:
            assert lib.smx_last_error(), "an error code without a message"
        return rc

    # negative sizes, counts past 2^31 - 1, n_sym past 2^32 - 1, empty_str below SMX_NONE, too many levels
    for field, value in [(f, -1) for f in SIZES] + [("grid_cap", -1), ("empty_str", -2), ("n_sym", 1 << 32),
                                                    ("n_levels", MAXL + 1), ("n_levels", 1 << 31)] + \
                        [(f, 1 << 31) for f in SIZES if f not in ("n_sym", "n_levels")]:
        s = _tree(buf)
        setattr(s, field, value)
        assert run(s) == SMX_E_ARG, (field, value)
    s = _tree(buf, n_levels=MAXL + 1)
    assert run(s) == SMX_E_ARG and b"SMX_TREE_MAX_LEVELS" in lib.smx_last_error()
    # the most levels and the largest n_sym are arguments still: they reach the workspace check
    s = _tree(buf, n_levels=MAXL)
    s.n_sym = (1 << 32) - 1
    assert run(s, ws, need.value - 1) == SMX_E_WORKSPACE
    # a null struct, null pointers all at once, then each pointer alone (v1_alt: only with empty_str set)
    assert run(None) == SMX_E_ARG and run(_tree(None)) == SMX_E_ARG
    n_ptr = 0
    for fname, ft in _abi.SmxTree._fields_:
        if ft is C.c_void_p:
            s = _tree(buf, empty_str=7)
            setattr(s, fname, None)
            assert run(s) == SMX_E_ARG, fname
            n_ptr += 1
    assert n_ptr == N_PTR
    s = _tree(buf)
    s.v1_alt = None
    assert run(s, ws, need.value - 1) == SMX_E_WORKSPACE  # (not read without an empty string: may be null)
    # a workspace too small, missing or misaligned
    s = _tree(buf)
    assert run(s, ws, need.value - 1) == SMX_E_WORKSPACE
    assert run(s, None, 65536) == SMX_E_WORKSPACE
    assert b"workspace" in lib.smx_last_error()
    odd = (C.c_uint8 * 65000).from_address(C.addressof(ws) + 4)
    assert run(s, odd, 65000) == SMX_E_WORKSPACE


def test_no_nodes_is_ok(lib):
    assert lib.smx_compose_tree(C.byref(_tree(None, 0, 0, 0, 0, 0)), None, 0, 0, None) == SMX_OK
    buf = (C.c_uint8 * 64)()
    assert lib.smx_compose_tree(C.byref(_tree(buf, n_nodes=0)), None, 0, 0, None) == SMX_OK
    assert lib.smx_compose_tree(C.byref(_tree(None, 5, 10, 0, 7, 0)), None, 0, 0, None) == SMX_OK
