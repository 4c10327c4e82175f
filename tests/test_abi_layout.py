"""The ctypes mirrors in semantic_merge_amd/_abi.py have the C layout of include/smx.h
(sizes and field offsets, from a host C program compiled against the header)."""
from semantic_merge_amd import _abi

from _util import assert_header_layout

STRUCTS = {"smx_ops": _abi.SmxOps, "smx_compose_out": _abi.SmxComposeOut, "smx_shard": _abi.SmxShard,
           "smx_rga_ops": _abi.SmxRgaOps, "smx_rga_out": _abi.SmxRgaOut}


def test_ctypes_structs_match_header():
    assert_header_layout(STRUCTS)
