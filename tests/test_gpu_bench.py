"""bench.py's command line: a plain run is the headline alone, and --dump-outputs writes
what the last timed step computed (checked here against the CPU oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle
from semantic_merge_amd import synth
from semantic_merge_amd._lib import DeviceCompose

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("order", "addr", "file", "ctx")
FULL_ONLY = ("pmc", "cpu_baseline", "end_to_end", "small_merge", "async_api", "graph_api",
             "stages_ms_per_step", "stage_calls_per_step")


def _load(d):
    out = {}
    for f in os.listdir(d):
        a = np.load(os.path.join(d, f))
        assert a.dtype == np.float64
        out[f[:-4]] = a
    return out


def _check(dump, ref):
    k, nc = len(ref[0]), len(ref[4])
    assert dump["counts"].tolist() == [k, nc]
    idx = dump["sample_index"].astype(np.int64)
    live = idx < k
    for name, r in zip(NAMES, ref):
        assert np.array_equal(dump[name][live], r[idx[live]].astype(np.float64)), name
        assert np.all(dump[name][~live] == -1.0), name
    assert np.array_equal(dump["conflicts"], ref[4].astype(np.float64))
    return idx


def test_plain_run_and_dump(tmp_path):
    """bench.py --gpus 1 --steps 3 --warmup 1 on a 2.4M-op config-3-shaped log (above the
    dump's sample size, so the per-op arrays are sampled): exit 0, three timed steps, the
    --full legs absent, and the dump equal to the oracle's results on the same log
    generated again here (so the inputs depend on the arguments alone)."""
    import bench
    n_ops, n_sym = 2_400_000, 20_000
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--n-ops",
           str(n_ops), "--n-sym", str(n_sym), "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(n_ops / (out["ms_per_step"] * 1e-3), rel=2e-3)
    assert out["metric"] == bench.METRIC and out["unit"] == "ops/s" and out["dtype"] == "u64"
    assert out["higher_is_better"] is True
    for key in FULL_ONLY:
        assert out[key] is None, key
    a = _load(tmp_path)
    assert sorted(a) == sorted(NAMES + ("conflicts", "counts", "sample_index"))
    assert sum(v.nbytes for v in a.values()) <= 64 * 2**20
    spec = synth.LiftSpec(**{**synth.CONFIGS["c3"].__dict__, "n_total": n_ops, "n_sym": n_sym})
    soa = synth.lift_soa(synth.lift_logs(spec))
    idx = _check(a, oracle.compose(soa))
    assert len(idx) < n_ops and np.all(np.diff(idx) > 0)
    assert out["config"]["composed_ops"] == int(a["counts"][0])


def test_dump_small_is_whole(tmp_path):
    """Below the sample size the dump holds every composed op."""
    import bench
    soa = synth.lift_soa(synth.lift_logs(synth.LiftSpec(30_001, 300, 5)))
    dc = DeviceCompose(soa)
    dc.run()
    bench.dump_outputs(str(tmp_path), dc, 0, 1)
    idx = _check(_load(tmp_path), oracle.compose(soa))
    assert np.array_equal(idx, np.arange(soa.n))
