"""The size queries of the three batched composes give pinned sizes (no GPU needed).

The counts are those of the library before smx_compose_pairs was folded onto the shared batched
path: a caller that sized its workspace then still fits, and a layout change shows up here on
purpose.  The shapes sit on both sides of the 256-byte rounding of a class list (64 entries of
4 bytes) and of BATCH_MAX_OPS."""
import ctypes

import pytest

from semantic_merge_amd import _abi
from semantic_merge_amd._lib import LIB_PATH

LARGE = _abi.BATCH_LARGE
N_TOTAL = (0, 1, 2049)
# smx_compose_batch_ex_workspace_bytes: {(n_merges, flags): bytes at each n_total of N_TOTAL}
BATCH = {
    (0, 0): (256, 256, 256), (1, 0): (1024, 1024, 1024), (64, 0): (1024, 1024, 1024), (65, 0): (1792, 1792, 1792),
    (0, LARGE): (256, 1536, 132608), (1, LARGE): (1280, 2560, 133632), (64, LARGE): (1280, 2560, 133632),
    (65, LARGE): (2304, 3584, 134656),
}
# smx_compose_batch_shared_ex_workspace_bytes with n_shared == n_total (with n_shared == 0: BATCH's)
SHARED_ALL = {
    (0, 0): (256, 256, 256), (1, 0): (1024, 1024, 1024), (64, 0): (1024, 1024, 1024), (65, 0): (1792, 1792, 1792),
    (0, LARGE): (256, 256, 256), (1, LARGE): (1280, 2560, 133632), (64, LARGE): (1280, 5376, 8393984),
    (65, LARGE): (2304, 7680, 8527360),
}
# smx_compose_pairs_workspace_bytes: {(n_logs, n_pairs, n_out): (bytes with flags 0, with SMX_BATCH_LARGE)}
PAIRS = {(0, 0, 0): (256, 256), (1, 1, 2): (1536, 3072), (64, 65, 4098): (2560, 266496), (65, 64, 1): (1792, 3328)}


@pytest.fixture(scope="module")
def lib():
    handle = ctypes.CDLL(LIB_PATH)
    _abi.declare(handle)
    return handle


def _bytes(query, *args):
    got = ctypes.c_size_t(0)
    assert query(*args, ctypes.byref(got)) == 0, args
    return got.value


@pytest.mark.parametrize("n_merges,flags", list(BATCH), ids=[f"{m}-{f}" for m, f in BATCH])
def test_batch_and_shared_workspace_bytes_pinned(lib, n_merges, flags):
    for n_total, plain, shared_all in zip(N_TOTAL, BATCH[n_merges, flags], SHARED_ALL[n_merges, flags]):
        assert _bytes(lib.smx_compose_batch_ex_workspace_bytes, n_merges, n_total, flags) == plain, n_total
        assert _bytes(lib.smx_compose_batch_shared_ex_workspace_bytes, n_merges, n_total, 0, flags) == plain, n_total
        assert _bytes(lib.smx_compose_batch_shared_ex_workspace_bytes, n_merges, n_total, n_total,
                      flags) == shared_all, n_total


@pytest.mark.parametrize("shape", list(PAIRS), ids=[str(s) for s in PAIRS])
def test_pairs_workspace_bytes_pinned(lib, shape):
    assert tuple(_bytes(lib.smx_compose_pairs_workspace_bytes, *shape, flags) for flags in (0, LARGE)) == PAIRS[shape]


def test_plain_queries_pinned(lib):
    assert _bytes(lib.smx_compose_batch_workspace_bytes, 65) == 1792
    assert _bytes(lib.smx_compose_batch_shared_workspace_bytes, 65) == 1792
