"""smx_rga_workspace_bytes gives the workspace layout's pinned sizes (no GPU needed).

The counts are those of the library before smx_rga.hip was split by role: a caller that
sized its workspace then still fits, and a layout change shows up here on purpose.  3072
events is one partition tile (the histogram's block count steps there); 255 / 256 / 257
lists are where the padding of the survivor counts to 256-list chunks steps."""
import ctypes

import pytest

from semantic_merge_amd import _abi
from semantic_merge_amd._lib import LIB_PATH

SMX_E_ARG = -1

EXPECTED = [
    ((0, 0), 13568),
    ((1, 1), 13568),
    ((3072, 1), 174336),
    ((3073, 1), 177408),
    ((3073, 255), 179712),
    ((20_000, 256), 1082624),
    ((20_000, 257), 1082624),
    ((20_000, 65_536), 2127104),
    ((20_000, 65_537), 2127104),
    ((1_000_000, 5000), 53428992),
    ((10_000_000, 50_000), 534195456),
]


@pytest.fixture(scope="module")
def lib():
    handle = ctypes.CDLL(LIB_PATH)
    _abi.declare(handle)
    return handle


@pytest.mark.parametrize("sizes,expected", EXPECTED, ids=[str(s) for s, _ in EXPECTED])
def test_rga_workspace_bytes_pinned(lib, sizes, expected):
    got = ctypes.c_size_t(0)
    assert lib.smx_rga_workspace_bytes(*sizes, ctypes.byref(got)) == 0
    assert got.value == expected


def test_rga_workspace_bytes_argument_errors(lib):
    got = ctypes.c_size_t(0)
    assert lib.smx_rga_workspace_bytes(-1, 1, ctypes.byref(got)) == SMX_E_ARG
    assert lib.smx_rga_workspace_bytes(1, -1, ctypes.byref(got)) == SMX_E_ARG
    assert lib.smx_rga_workspace_bytes(1, 1, None) == SMX_E_ARG
