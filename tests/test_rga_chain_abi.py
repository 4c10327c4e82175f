"""smx_rga_replay_chain's C ABI without a GPU: the ctypes mirror of smx_rga_chain has the
header's layout, the library exports and declares the two symbols, the workspace query is
monotone in n_jobs, n_links and n_out, every argument and workspace error comes back before any
HIP call, on host pointers, and n_jobs = 0 needs no workspace."""
import ctypes as C
import os

import pytest

from semantic_merge_amd import _abi
from semantic_merge_amd._lib import LIB_PATH

from _util import assert_header_layout

SMX_OK, SMX_E_ARG, SMX_E_WORKSPACE = 0, -1, -4
IDX_MAX = (1 << 30) - 1  # RGA_IDX_MASK: what smx_rga_replay accepts for n_ops
LIM = (1 << 31) - 1
N_PTR = 10  # the pointers of smx_rga_chain


def test_smx_rga_chain_matches_header():
    assert_header_layout({"smx_rga_chain": _abi.SmxRgaChain, "smx_rga_out": _abi.SmxRgaOut})
    names = [f for f, _ in _abi.SmxRgaChain._fields_]
    assert names[:8] == ["n_total", "n_segs", "n_jobs", "n_links", "n_out", "seg_off", "job_off", "job_seg"]
    # then the event columns of smx_rga_ops, without `list`: as smx_rga_onto
    assert names[8:] == [f for f, _ in _abi.SmxRgaOps._fields_ if f not in ("n_ops", "n_lists", "list")]
    assert names[8:] == [f for f, _ in _abi.SmxRgaOnto._fields_][7:]


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB_PATH), "build libsmx.so first (__graft_entry__.build())"
    return _abi.declare(C.CDLL(LIB_PATH))


def _chain(buf, n_total=10, n_segs=4, n_jobs=3, n_links=7, n_out=30):
    """A struct whose every pointer is the (host) buffer `buf`: the calls below fail before
    anything reads it."""
    p = C.addressof(buf) if buf is not None else 0
    return _abi.SmxRgaChain(n_total, n_segs, n_jobs, n_links, n_out, *([p] * N_PTR))


def _out(buf, tomb=False):
    p = C.addressof(buf) if buf is not None else 0
    return _abi.SmxRgaOut(p, p, p, p, p if tomb else None)


def test_symbols_exported_and_declared(lib):
    for name in ("smx_rga_replay_chain_workspace_bytes", "smx_rga_replay_chain"):
        assert name in _abi.EXPORTS
        assert hasattr(lib, name), name
    assert lib.smx_rga_replay_chain.argtypes == [C.POINTER(_abi.SmxRgaChain), C.POINTER(_abi.SmxRgaOut), C.c_void_p,
                                                 C.c_size_t, C.c_void_p]
    assert lib.smx_rga_replay_chain_workspace_bytes.argtypes == [C.c_int64, C.c_int64, C.c_int64,
                                                                 C.POINTER(C.c_size_t)]
    assert sum(ft is C.c_void_p for _, ft in _abi.SmxRgaChain._fields_) == N_PTR


def test_workspace_query(lib):
    a = C.c_size_t(0)

    def q(n_jobs, n_links, n_out):
        assert lib.smx_rga_replay_chain_workspace_bytes(n_jobs, n_links, n_out, C.byref(a)) == SMX_OK
        return a.value

    counts = (0, 1, 63, 64, 65, 255, 256, 257, 1000, 65_536, 65_537, 1 << 20, LIM - 1)
    outs = (0, 1, 63, 64, 65, 1000, 100_001, 1 << 20, IDX_MAX)
    for fixed in (0, 7, 5000):
        for arg, values in ((0, counts), (1, counts), (2, outs)):
            prev = 0
            for v in values:
                args = [fixed] * 3
                args[arg] = v
                size = q(*args)
                assert size >= prev, args
                prev = size
    assert q(1, 1, 1) > 0
    assert q(LIM - 1, 5, 5) > q(1, 5, 5) and q(5, LIM - 1, 5) > q(5, 1, 5) and q(5, 5, IDX_MAX) > q(5, 5, 1)
    # the jobs' slices (survivors, records, sort positions, states) and the column map are sized by n_out
    assert q(5, 9, 1 << 20) - q(5, 9, 1 << 19) >= (1 << 19) * (16 + 4 + 4 + 4 + 1 + 4)
    # the link scan's two arrays
    assert q(5, 1 << 20, 100) - q(5, 1 << 19, 100) == (1 << 19) * 8
    # onto's layout for (n_jobs, n_out) without its 16 bytes per job, plus the map and the link arrays
    onto = C.c_size_t(0)
    for nj, nk, no in ((1, 1, 1), (300, 700, 5000), (70_000, 70_000, 100_000), (3, 0, 0)):
        assert lib.smx_rga_replay_onto_workspace_bytes(nj, no, C.byref(onto)) == SMX_OK
        r = lambda b: (b + 255) & ~255
        assert q(nj, nk, no) == onto.value - r((nj + 1) * 16) + r(max(no, 1) * 4) + 2 * r((nk + 1) * 4)
    # limits: negative sizes, n_out past what smx_rga_replay takes for n_ops, no result pointer
    for args in ((-1, 1, 1), (1, -1, 1), (1, 1, -1), (LIM, 1, 1), (1, LIM, 1), (1 << 31, 1, 1), (1, 1 << 31, 1),
                 (1, 1, IDX_MAX + 1), (1, 1, 1 << 31)):
        assert lib.smx_rga_replay_chain_workspace_bytes(*args, C.byref(a)) == SMX_E_ARG, args
        assert lib.smx_last_error()
    assert lib.smx_rga_replay_chain_workspace_bytes(5, 5, 5, None) == SMX_E_ARG


@pytest.mark.parametrize("tomb", [False, True])
def test_argument_errors_without_gpu(lib, tomb):
    buf = (C.c_uint8 * 4096)()
    ws = (C.c_uint64 * 8192)()
    need = C.c_size_t(0)
    assert lib.smx_rga_replay_chain_workspace_bytes(3, 7, 30, C.byref(need)) == SMX_OK
    assert 0 < need.value <= 65000

    def run(s, o="default", w=ws, nbytes=65536):
        o = _out(buf, tomb) if o == "default" else o
        rc = lib.smx_rga_replay_chain(C.byref(s) if s is not None else None, C.byref(o) if o is not None else None,
                                      w, nbytes, None)
        assert rc != SMX_OK  # (no call of this test may get as far as the device)
        assert lib.smx_last_error(), "an error code without a message"
        return rc

    # negative sizes; n_total and n_out above 2^30 - 1; n_segs, n_jobs, n_links at or above 2^31 - 1
    for field, value in (("n_total", -1), ("n_segs", -1), ("n_jobs", -1), ("n_links", -1), ("n_out", -1),
                         ("n_total", IDX_MAX + 1), ("n_out", IDX_MAX + 1), ("n_total", 1 << 31), ("n_out", 1 << 40),
                         ("n_jobs", LIM), ("n_segs", LIM), ("n_links", LIM), ("n_links", 1 << 33)):
        s = _chain(buf)
        setattr(s, field, value)
        assert run(s) == SMX_E_ARG, (field, value)
    # the largest n_total is an argument still: it reaches the workspace check
    s = _chain(buf, n_total=IDX_MAX)
    assert run(s, nbytes=need.value - 1) == SMX_E_WORKSPACE
    # a null struct, a null output, null pointers all at once, then each pointer alone
    assert run(None) == SMX_E_ARG and run(_chain(buf), None) == SMX_E_ARG and run(_chain(None)) == SMX_E_ARG
    n_ptr = 0
    for fname, ft in _abi.SmxRgaChain._fields_:
        if ft is C.c_void_p:
            s = _chain(buf)
            setattr(s, fname, None)
            assert run(s) == SMX_E_ARG, fname
            n_ptr += 1
    assert n_ptr == N_PTR
    for fname in ("out_value", "out_src", "out_offsets", "counts"):
        o = _out(buf, tomb)
        setattr(o, fname, None)
        assert run(_chain(buf), o) == SMX_E_ARG, fname
    # (a null pointer with a zero size is no error: no events, no columns, no links; it goes on
    # to the workspace check)
    s = _chain(buf, n_total=0, n_links=0)
    for fname in ("op", "value", "anchor", "t", "author", "opid_hi", "opid_lo", "job_seg"):
        setattr(s, fname, None)
    small = C.c_size_t(0)
    assert lib.smx_rga_replay_chain_workspace_bytes(3, 0, 30, C.byref(small)) == SMX_OK
    assert run(s, nbytes=small.value - 1) == SMX_E_WORKSPACE
    o = _out(buf, tomb)
    o.out_value = o.out_src = None
    assert run(_chain(buf, n_out=0), o, nbytes=0) == SMX_E_WORKSPACE
    # a workspace too small, missing or misaligned
    s = _chain(buf)
    assert run(s, nbytes=need.value - 1) == SMX_E_WORKSPACE
    assert run(s, w=None) == SMX_E_WORKSPACE
    assert b"workspace" in lib.smx_last_error()
    odd = (C.c_uint8 * 65000).from_address(C.addressof(ws) + 4)
    assert run(s, w=odd, nbytes=65000) == SMX_E_WORKSPACE
    assert b"aligned" in lib.smx_last_error()


def test_no_jobs_arguments_are_checked_without_a_workspace(lib):
    """n_jobs = 0 needs no workspace: the query gives a size, but a call with none passes the
    workspace check (its arguments are still checked; what it writes is checked on the GPU, in
    tests/test_gpu_rga_chain.py)."""
    buf = (C.c_uint8 * 64)()
    a = C.c_size_t(0)
    assert lib.smx_rga_replay_chain_workspace_bytes(0, 0, 0, C.byref(a)) == SMX_OK
    s = _chain(buf, n_total=0, n_segs=0, n_jobs=0, n_links=0, n_out=0)
    o = _out(buf)
    o.out_offsets = None  # the one thing an n_jobs = 0 call writes besides counts
    assert lib.smx_rga_replay_chain(C.byref(s), C.byref(o), None, 0, None) == SMX_E_ARG
    assert b"null output" in lib.smx_last_error()
    s.seg_off = None
    assert lib.smx_rga_replay_chain(C.byref(s), C.byref(_out(buf)), None, 0, None) == SMX_E_ARG
    assert b"workspace" not in lib.smx_last_error()
