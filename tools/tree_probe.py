"""Time smx_compose_tree on the GPU against smx_compose_train on the same states spelled out as
root-to-node trains: the same LogsSoA resident on the device once, both rigs (DeviceTree,
DeviceTrains) in one process, their device time between two events around INNER calls on one
stream.  Two shapes:

    stack    every prefix of a 32-log stack of ~40-op logs: a path of 32 nodes and 32 levels,
             against 32 trains of 1 .. 32 steps (32 steps against 528)
    window   a 16-log window of ~100-op logs with every drop-one fallback: the prefixes 1..k and,
             per dropped member i, the prefixes without it; against the same paths as trains

The two forms alternate, ROUNDS times each after WARM warm-up rounds; per call the median with
min to max, in microseconds.  Both forms' results are compared once, node by node.  The number
of steps each form executes is exact: the tree's nodes against the sum of the paths' lengths.

    python tools/tree_probe.py [--out profiles/tree/probe.json] [--rounds 15] [--inner 20]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from semantic_merge_amd._lib import DeviceTrains, DeviceTree, _torch  # noqa: E402
from semantic_merge_amd._session import tree_levels  # noqa: E402
from semantic_merge_amd.marshal import marshal_logs, move_file_alt  # noqa: E402

from train_probe import make_logs  # noqa: E402

WARM = 3


def stack(k):
    """(parent, log) of every prefix of a stack of k logs."""
    return [(n - 1 if n else None, n) for n in range(k)]


def window(k):
    """The prefixes of a window of k logs, and per dropped member i the prefixes of the window
    without it, under the shared prefix 0 .. i-1."""
    nodes = stack(k)
    for i in range(k):
        at = i - 1 if i else None
        for l in range(i + 1, k):
            nodes.append((at, l))
            at = len(nodes) - 1
    return nodes


SHAPES = (("stack: prefixes of 32 logs x 40 ops", stack, 32, 40), ("window: 16 logs x 100 ops, drop-one fallbacks", window, 16, 100))


def per_call_us(torch, rig, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        rig.run()
    end.record()
    end.synchronize()
    return 1e3 * start.elapsed_time(end) / inner


def stat(xs):
    return {"median_us": round(statistics.median(xs), 2), "min_us": round(min(xs), 2), "max_us": round(max(xs), 2)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    torch = _torch()
    rows = []
    for label, make, k, n_ops in SHAPES:
        logs, _ = make_logs(1, k, n_ops)
        nodes = make(k)
        lsoa = marshal_logs(logs)
        alt, empty = move_file_alt([o for x in logs for o in x], lsoa.kind, lsoa.strings)
        order, level_off, back = tree_levels([p for p, _ in nodes])
        parents = np.asarray([-1 if nodes[n][0] is None else back[nodes[n][0]] for n in order], np.int32)
        node_log = np.asarray([nodes[n][1] for n in order], np.int32)
        paths = []
        for n in range(len(nodes)):
            path, up = [], n
            while up >= 0:
                path.append(int(node_log[up]))
                up = int(parents[up])
            paths.append(path[::-1])
        tree = DeviceTree(lsoa, parents, node_log, level_off, v1_alt=alt, empty_str=empty)
        trains = DeviceTrains(lsoa, paths, v1_alt=alt, empty_str=empty)
        tree.run()
        trains.run()
        got, want = tree.results(), trains.results()
        same = all(all(np.array_equal(a, b) for a, b in zip(g[:4], w[:4])) and (g[5], g[6]) == w[5][-1][:2]
                   and np.array_equal(g[7], w[5][-1][2]) for g, w in zip(got, want))
        t_tree, t_train = [], []
        for r in range(WARM + args.rounds):
            a, b = per_call_us(torch, tree, args.inner), per_call_us(torch, trains, args.inner)
            if r >= WARM:
                t_tree.append(a)
                t_train.append(b)
        row = {"shape": label, "nodes": len(nodes), "levels": len(level_off) - 1,
               "tree_launches": 1 + 3 * (len(level_off) - 1), "train_launches": 5,
               "tree_steps": len(nodes), "train_steps": sum(len(p) for p in paths),
               "conflicting_nodes": sum(1 for g in got if g[6] > 0), "equal": same, "rounds": args.rounds,
               "inner": args.inner, "compose_tree": stat(t_tree), "compose_train": stat(t_train),
               "train_over_tree_median": round(statistics.median(t_train) / statistics.median(t_tree), 2)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
