"""smx_train_stage's and smx_train_land's C ABI without a GPU: the ctypes mirror of smx_train_step
has the header's layout, the library exports and declares the two symbols, and every argument
error comes back before any HIP call, on host pointers, with a message."""
import ctypes as C
import os

import pytest

from semantic_merge_amd import _abi
from semantic_merge_amd._lib import LIB_PATH

from _util import assert_header_layout

SMX_OK, SMX_E_ARG = 0, -1
LIM = (1 << 31) - 1
PTRS = [f for f, ft in _abi.SmxTrainStep._fields_ if ft is C.c_void_p]
SIZES = ("n_total", "n_sym", "n_acc", "log_lo", "log_n", "conflict_cap", "record_cap")
COLS = ("kind", "ts", "oid_hi", "oid_lo", "sym", "v0", "v1")
ACC = ("acc_src", "acc_addr", "acc_file", "acc_ctx")
STAGED = tuple("st_" + c for c in COLS)
RESULT = ("order", "addr", "file", "ctx")
OUT = ("out_src", "out_addr", "out_file", "out_ctx")
# the pointers each call uses in a step with n_total, n_acc, conflict_cap and record_cap above zero
USES = {"smx_train_stage": COLS + ("v1_alt",) + ACC[:3] + STAGED + ("status",),
        "smx_train_land": ("v1_alt",) + ACC + RESULT + ("conflicts", "counts") + OUT + ("records", "status")}


def test_smx_train_step_matches_header():
    assert_header_layout({"smx_train_step": _abi.SmxTrainStep})
    assert [f for f, ft in _abi.SmxTrainStep._fields_ if ft is C.c_int64] == \
        ["n_total", "n_sym", "n_acc", "log_lo", "log_n", "conflict_cap", "record_cap"]
    assert len(PTRS) == 31 and _abi.SmxTrainStep._fields_[-1] == ("empty_str", C.c_int32)


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(LIB_PATH), "build libsmx.so first (__graft_entry__.build())"
    return _abi.declare(C.CDLL(LIB_PATH))


def _step(bufs, **kw):
    """A step over 100 ops (an accumulator of 10, a log of 20 at 30) whose every pointer is a host
    buffer of its own (`bufs`; None: null): the calls below fail before anything reads them."""
    s = _abi.SmxTrainStep(n_total=100, n_sym=4, n_acc=10, log_lo=30, log_n=20, conflict_cap=10, record_cap=20,
                          empty_str=-1)
    for i, f in enumerate(PTRS):
        setattr(s, f, C.addressof(bufs[i]) if bufs is not None else None)
    for f, v in kw.items():
        setattr(s, f, v)
    return s


@pytest.fixture(scope="module")
def bufs():
    return [(C.c_uint8 * 64)() for _ in PTRS]


def test_symbols_exported_and_declared(lib):
    for name in ("smx_train_stage", "smx_train_land"):
        assert name in _abi.EXPORTS
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == [C.POINTER(_abi.SmxTrainStep), C.c_void_p]
        assert getattr(lib, name).restype is C.c_int


@pytest.mark.parametrize("name", ["smx_train_stage", "smx_train_land"])
def test_argument_errors_without_gpu(lib, bufs, name):
    fn = getattr(lib, name)

    def run(s):
        rc = fn(C.byref(s) if s is not None else None, None)
        if rc != SMX_OK:
            assert lib.smx_last_error(), "an error code without a message"
        return rc

    assert run(None) == SMX_E_ARG
    # negative sizes, empty_str below SMX_NONE, n_sym past 2^32 - 1
    for field, value in [(f, -1) for f in SIZES] + [("empty_str", -2), ("n_sym", 1 << 32)]:
        assert run(_step(bufs, **{field: value})) == SMX_E_ARG, (field, value)
    # n_total, and the accumulator and the log together, past 2^31 - 1
    assert run(_step(bufs, n_total=1 << 31)) == SMX_E_ARG
    assert run(_step(bufs, n_total=LIM, n_acc=LIM, log_lo=0, log_n=1)) == SMX_E_ARG
    assert run(_step(bufs, n_total=LIM, n_acc=1 << 31, log_lo=0, log_n=0)) == SMX_E_ARG
    assert run(_step(bufs, n_total=LIM, n_acc=1 << 62, log_lo=0, log_n=1 << 62)) == SMX_E_ARG
    # a log that leaves the columns
    assert run(_step(bufs, log_lo=81)) == SMX_E_ARG
    assert run(_step(bufs, log_lo=101, log_n=0)) == SMX_E_ARG
    assert run(_step(bufs, n_total=LIM, log_lo=LIM, log_n=LIM)) == SMX_E_ARG
    assert b"log" in lib.smx_last_error()
    # v1_alt: null only without an empty string, or without columns
    assert run(_step(bufs, v1_alt=None, empty_str=0)) == SMX_E_ARG
    assert b"v1_alt" in lib.smx_last_error()
    # all the pointers null, then each pointer that the call uses alone
    assert run(_step(None)) == SMX_E_ARG
    for f in USES[name]:
        assert run(_step(bufs, empty_str=7, **{f: None})) == SMX_E_ARG, f
    assert set(USES[name]) <= set(PTRS)


def test_land_refuses_an_accumulator_out_that_is_the_accumulator_in(lib, bufs):
    for o in OUT:
        for i in ACC:
            s = _step(bufs)
            setattr(s, o, getattr(s, i))
            assert lib.smx_train_land(C.byref(s), None) == SMX_E_ARG, (o, i)
            assert b"alias" in lib.smx_last_error()


def test_an_empty_step_is_ok_and_launches_nothing(lib, bufs):
    for name in ("smx_train_stage", "smx_train_land"):
        assert getattr(lib, name)(C.byref(_step(bufs, n_acc=0, log_n=0)), None) == SMX_OK
        assert getattr(lib, name)(C.byref(_step(None, n_acc=0, log_n=0)), None) == SMX_OK
        assert getattr(lib, name)(C.byref(_step(None, n_total=0, n_acc=0, log_lo=0, log_n=0)), None) == SMX_OK
