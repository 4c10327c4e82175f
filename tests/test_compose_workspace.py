"""smx_compose_workspace_bytes gives the workspace layout's pinned sizes (no GPU needed).

The counts are those of the library before smx_compose.hip was split by role: a caller that
sized its workspace then still fits, and a layout change shows up here on purpose."""
import ctypes

import pytest

from semantic_merge_amd import _abi
from semantic_merge_amd._lib import LIB_PATH

EXPECTED = [
    ((0, 0, 0), 23552),
    ((1, 0, 1), 23552),
    ((1000, 1000, 10), 232704),
    ((2048, 1, 4), 239616),
    ((1 << 18, 1 << 18, 1 << 16), 57438976),
    ((3_000_000, 1_000_000, 1 << 22), 541598208),
]


@pytest.fixture(scope="module")
def lib():
    handle = ctypes.CDLL(LIB_PATH)
    _abi.declare(handle)
    return handle


@pytest.mark.parametrize("sizes,expected", EXPECTED, ids=[str(s) for s, _ in EXPECTED])
def test_compose_workspace_bytes_pinned(lib, sizes, expected):
    got = ctypes.c_size_t(0)
    assert lib.smx_compose_workspace_bytes(*sizes, ctypes.byref(got)) == 0
    assert got.value == expected
