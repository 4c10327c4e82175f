"""Generate tests/golden/train_cases.json by running the REFERENCE implementation.

A merge train over logs P1..Pk is the host loop that ``semmerge`` callers run today:

    acc = []
    for P in train:
        out, conflicts = compose_oplogs(acc, P)
        if conflicts:        # semmerge exits 1 before applying anything (__main__.py:65-69):
            continue         # the log is put off the train
        acc = out

This tool imports the reference read-only, as tools/make_golden.py does, runs exactly that loop
of its ``compose_oplogs`` on small random trains and records the inputs and its outputs: per
case the logs, the train (log indices, in order), the ops the last landed step leaves, and per
step the conflicts (an empty list: the step landed).  The logs are drawn from make_golden.py's
pools over few symbols, so that conflicts, evictions and None-valued moves are frequent.
Nothing from the reference is copied.

The file is written in a short form that loses nothing (tests/_train.py's golden_case reads it
back, and every case is checked here to read back to exactly the reference's dicts): an input op
is [id, type, symbolId, addressId, params, [timestamp]] (plus guards and effects where it has
any); an output op is [log, index] of the input op it is a clone of, plus [params, addressId]
where the reference changed them; a conflict is its A and B ops in that form (its other fields
follow from them: conflict.py:34-49).

    python tools/make_train_golden.py
"""
from __future__ import annotations

import json
import os
import random
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402

sys.path.insert(0, os.path.join(G.REPO, "tests"))

N_CASES = 150
SEED = 20261020
SIZES = [0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 6, 8, 12]  # ops per log: 0 to 12, short ones more often
N_LOGS = [1, 2, 2, 3, 3, 3, 4, 4, 5, 6]            # logs per case: 1 to 6


def rand_log(rng, n, ts_mode, id_mode, syms, pool):
    log = []
    for _ in range(n):
        d = G.rand_op(rng, ts_mode, id_mode, syms, pool)
        if rng.random() < 0.9:  # (most ops without the bulky fields: the file stays small)
            d["guards"], d["effects"] = {}, {}
        r = rng.random()
        if r < 0.30:    # renames of few names: divergent ones conflict, equal ones do not
            d["type"] = "renameSymbol"
            d["params"] = {"oldName": "old", "newName": rng.choice(["p", "q", "p", None])}
            f = rng.choice(G.FILES)
            if f != "MISSING":
                d["params"]["file"] = f
        elif r < 0.55:  # moves whose address or file is often None or missing
            d["type"] = "moveDecl"
            d["params"] = {"oldAddress": "a0"}
            a = rng.choice(G.ADDRS + [None, "MISSING"])
            if a != "MISSING":
                d["params"]["newAddress"] = a
            f = rng.choice(G.FILES + [None, "MISSING"])
            if f != "MISSING":
                d["params"]["newFile"] = f
            f2 = rng.choice(G.FILES)
            if f2 != "MISSING":
                d["params"]["file"] = f2
        log.append(d)
    return log


def run_train(compose, ops_mod, logs, train):
    objs = [[ops_mod.Op.from_dict(d) for d in log] for log in logs]
    before = json.dumps([[o.to_dict() for o in log] for log in objs])
    acc, steps = [], []
    for l in train:
        out, conf = compose.compose_oplogs(acc, objs[l])
        steps.append([c.to_dict() for c in conf])
        if not conf:
            acc = out
    assert json.dumps([[o.to_dict() for o in log] for log in objs]) == before, "reference mutated inputs"
    return {"logs": logs, "train": list(train), "out": [o.to_dict() for o in acc], "steps": steps}


def make_cases(compose, ops_mod, n_cases, seed):
    rng = random.Random(seed)
    cases = []
    for c in range(n_cases):
        ts_mode = "iso" if c % 4 else "any"
        id_mode = ["uuid", "short", "long", "short", "short"][c % 5]
        syms = [f"s{i}" for i in range(rng.choice([1, 2, 2, 3]))]
        pool = []
        logs = [rand_log(rng, rng.choice(SIZES), ts_mode, id_mode, syms, pool) for _ in range(rng.choice(N_LOGS))]
        train = list(range(len(logs)))
        if c % 6 == 5:  # another order, a subset, a log more than once
            train = [rng.randrange(len(logs)) for _ in range(rng.randint(1, 6))]
        cases.append(run_train(compose, ops_mod, logs, train))
    return cases


def short_op(d):
    prov = d["provenance"]
    assert d["schemaVersion"] == 1 and prov.get("rev") == "base" and set(prov) <= {"rev", "timestamp"}
    s = [d["id"], d["type"], d["target"]["symbolId"], d["target"]["addressId"], d["params"],
         [prov["timestamp"]] if "timestamp" in prov else []]
    return s + [d["guards"], d["effects"]] if d["guards"] or d["effects"] else s


def short_clone(logs, train, d):
    """[log, index] of an input op of the train that `d` is a clone of, with [params, addressId]
    behind it where they are not the input op's."""
    for l in train:
        for i, src in enumerate(logs[l]):
            if d == src:
                return [l, i]
    for l in train:
        for i, src in enumerate(logs[l]):
            if d == {**src, "params": d["params"], "target": d["target"]} and \
                    d["target"]["symbolId"] == src["target"]["symbolId"]:
                return [l, i, d["params"], d["target"]["addressId"]]
    raise AssertionError("an output op that is no clone of an input op")


def short_case(case):
    from _train import golden_case
    logs, train = case["logs"], case["train"]
    out = {"logs": [[short_op(d) for d in log] for log in logs], "train": train,
           "out": [short_clone(logs, train, d) for d in case["out"]],
           "steps": [[[short_clone(logs, train, c["opA"]), short_clone(logs, train, c["opB"])] for c in step]
                     for step in case["steps"]]}
    back = golden_case(json.loads(json.dumps(out)))
    assert back == case, "the short form does not read back to the reference's dicts"
    return out


def main() -> None:
    compose, _, ops_mod = G._import_reference()
    cases = make_cases(compose, ops_mod, N_CASES, SEED)
    path = os.path.join(G.GOLD, "train_cases.json")
    with open(path, "w") as fh:  # one case per line
        fh.write("[\n" + ",\n".join(json.dumps(short_case(c), separators=(",", ":")) for c in cases) + "\n]\n")
    steps = [s for c in cases for s in c["steps"]]
    print(f"train cases: {len(cases)}, steps: {len(steps)}, evicted: {sum(1 for s in steps if s)}, "
          f"bytes: {os.path.getsize(path)}")


if __name__ == "__main__":
    main()
