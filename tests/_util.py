"""Shared helpers: golden fixtures -> ops -> (marshal, compose backend, materialize) -> JSON."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from semantic_merge_amd.marshal import marshal
from semantic_merge_amd.materialize import materialize_conflicts, materialize_ops
from semantic_merge_amd.ops import Op

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HDR_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def load(name):
    with open(os.path.join(GOLD, name)) as fh:
        return json.load(fh)


def to_ops(dicts):
    return [Op.from_dict(d) for d in dicts]


def jline(obj):
    return json.dumps(obj, ensure_ascii=False, separators=(",", ":"))


def run_backend(backend, A, B):
    """backend(soa) -> (order, addr, file, ctx, pairs); returns (out_dicts, conflict_dicts)."""
    oa, ob = to_ops(A), to_ops(B)
    soa = marshal(oa, ob)
    order, addr, file, ctx, pairs = backend(soa)
    allops = oa + ob
    out = materialize_ops(allops, soa.kind, soa.strings, order, addr, file, ctx)
    conf = materialize_conflicts(allops, np.asarray(pairs).reshape(-1, 2))
    return [o.to_dict() for o in out], [c.to_dict() for c in conf]


def assert_case(backend, case, label=""):
    out, conf = run_backend(backend, case["A"], case["B"])
    assert jline(out) == jline(case["out"]), f"{label}: composed ops differ"
    assert jline(conf) == jline(case["conflicts"]), f"{label}: conflicts differ"


def _eq_soa(gpu, ref, label):
    """Both (order, addr, file, ctx, conflict pairs) tuples are equal, array by array."""
    names = ("order", "addr", "file", "ctx", "conflicts")
    for name, g, r in zip(names, gpu, ref):
        assert g.shape == r.shape, f"{label}: {name} shape {g.shape} vs {r.shape}"
        if not np.array_equal(g, r):
            bad = np.flatnonzero(g.reshape(-1) != r.reshape(-1))[:5]
            raise AssertionError(f"{label}: {name} differs at {bad.tolist()}")


def assert_header_layout(structs):
    """Every ctypes class of `structs` ({C struct name: class}) has the size, the fields and
    the field offsets of its struct in include/smx.h, from a host C program compiled against
    the header."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "smx.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        r = subprocess.run(["gcc", "-I", HDR_DIR, "-o", exe, src], capture_output=True, text=True)
        if r.returncode != 0 and "not found" in r.stderr:
            pytest.skip("no C compiler")
        assert r.returncode == 0, r.stderr
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {}
    for line in filter(None, out):
        *cname, fname, value = line.split()
        got.setdefault(" ".join(cname), {})[fname] = int(value)
    for cname, py in structs.items():
        assert got[cname].pop("size") == ctypes.sizeof(py), cname
        assert set(got[cname]) == {f for f, _ in py._fields_}, cname
        for fname, _ in py._fields_:
            assert got[cname][fname] == getattr(py, fname).offset, (cname, fname)
