#!/usr/bin/env python3
"""Batched compose with SMX_BATCH_LARGE against the loop it replaces.

For each shape: M merges of ~n ops on device-resident columns, composed (a) by one
smx_compose_batch_ex call with SMX_BATCH_LARGE and (b) by a loop of smx_compose, one call per
merge -- what ComposeSession.compose_many does for merges over 2048 ops without the flag.  Both
are timed with device events on one stream (the loop's per-merge host round trips fall inside
its interval: that is its cost), alternated in one run after a warm-up, and reported as
median (min - max) in microseconds.  The results of the two are compared before timing.  The
shared form: a 2100-op shared log against 256 own logs of ~100 ops, against the same loop.

    python tools/batch_large_probe.py [--reps 7] [--out profiles/batch_large/probe.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from semantic_merge_amd import _abi, synth  # noqa: E402
from semantic_merge_amd._lib import DeviceBatch, DeviceBatchShared, DeviceCompose  # noqa: E402
from semantic_merge_amd.marshal import ID_UUID, TS_ISO, SharedSoA  # noqa: E402

COLS = ("kind", "ts", "oid_hi", "oid_lo", "sym", "v0", "v1")


def lift(n, seed):
    return synth.lift_soa(synth.lift_logs(synth.LiftSpec(n, max(n // 100, 2), seed, divergent=0.05)))


def timed(torch, fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def stats(xs):
    return {"median_us": round(statistics.median(xs), 1), "min_us": round(min(xs), 1), "max_us": round(max(xs), 1)}


def probe(torch, name, batch, singles, reps):
    stream = torch.cuda.current_stream()

    def loop():
        for dc in singles:
            dc.run()

    batch.run()
    loop()
    got = batch.results()
    for m, dc in enumerate(singles):   # equality with the loop's results, before any timing
        for g, w in zip(got[m], dc.results()):
            assert np.array_equal(g, w), f"{name}: merge {m} differs from smx_compose"
    tb, tl = [], []
    for _ in range(reps):
        tb.append(timed(torch, batch.run, stream))
        tl.append(timed(torch, loop, stream))
    row = {"shape": name, "merges": len(singles), "batch": stats(tb), "loop": stats(tl),
           "loop_over_batch": round(statistics.median(tl) / statistics.median(tb), 2)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--max-ops", type=int, default=1 << 25, help="skip shapes of more ops in all")
    args = ap.parse_args()
    import torch
    rows = []
    for n in (3000, 16000, 64000):
        for M in (1, 16, 256):
            if n * M > args.max_ops:
                continue
            soas = [lift(n + 7 * (m % 5), 1000 + m % 16) for m in range(min(M, 16))]
            soas = [soas[m % len(soas)] for m in range(M)]
            rows.append(probe(torch, f"{M} x {n}", DeviceBatch(soas, flags=_abi.BATCH_LARGE),
                              [DeviceCompose(s) for s in soas], args.reps))
    base = lift(2 * 26000, 77)
    lens = [60 + (37 * m) % 81 for m in range(256)]
    keep = np.concatenate([np.arange(2100), base.n_a + np.arange(sum(lens))])
    off = 2100 + np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.int64)
    ssoa = SharedSoA(2100, off, *[np.ascontiguousarray(getattr(base, c)[keep]) for c in COLS], base.n_sym, [],
                     TS_ISO, ID_UUID)
    rows.append(probe(torch, "shared 2100 + 256 x ~100", DeviceBatchShared(ssoa, flags=_abi.BATCH_LARGE),
                      [DeviceCompose(ssoa.merge(m)) for m in range(256)], args.reps))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
