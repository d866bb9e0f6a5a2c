#!/usr/bin/env python3
"""Randomised check of the POA engine's sequence-to-graph DP against the plain Python recurrence and, pair by pair and graph
by graph, against the oracle's scalar POA (oracle/poa_oracle.cpp), under one alignment type of `cluster -A`.

usage: fuzz_poa.py [graphs] [seed] [--type 0|1|2]   (each graph: 4-9 additions of mutated / cut / extended copies)
       fuzz_poa.py --case "<dict>" [--type 0|1|2]   (replays one case of tests/fuzz_cases.run_consensus_poa, as
                                                     test_fuzz_consensus_with_real_graphs prints it; --type overrides its poa_type)"""
import argparse
import ast
import random
import sys
import time

sys.path.insert(0, ".")
from isonclust2_amd import api  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from tests.poa_common import mutate, random_addition  # noqa: E402
from tests.poa_modes_common import boundary_violations, mode_path_score, mode_score  # noqa: E402
from tests.test_gpu_poa import Poa  # noqa: E402
from tests.test_gpu_poa_modes import ModePoa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("graphs", nargs="?", type=int, default=20)
ap.add_argument("seed", nargs="?", type=int, default=1)
ap.add_argument("--type", type=int, default=None, choices=[0, 1, 2])
ap.add_argument("--case", default=None)
a = ap.parse_args()
ctx = api.Context(0)

if a.case:
    from tests import fuzz_cases as fz
    c = ast.literal_eval(a.case)
    if a.type is not None:
        c["poa_type"] = a.type
    ok, why = fz.run_consensus_poa(ctx, c)
    print("ok" if ok else f"MISMATCH: {why}", c)
    sys.exit(0 if ok else 1)

T = a.type or 0
rng = random.Random(a.seed)
bad = adds = 0
t0 = time.time()
for g in range(a.graphs):
    poa, orc = (ModePoa(ctx, T) if T else Poa(ctx)), po.OraclePoa(mode=T)
    ln = rng.choice([40, 90, 200, 260, 330])
    truth = bytes(rng.choice(b"ACGT") for _ in range(ln))
    first = mutate(rng, truth, rng.choice([0.0, 0.05, 0.15]))
    poa.create(0, first)
    orc.create(0, first)
    for t in range(rng.randint(4, 9)):
        r = random_addition(rng, truth, t)
        if not r:
            continue
        bases, rank, ef, et, ew = poa.graph(0)
        want = mode_score(bases, rank, ef, et, r, T)
        poa.add(0, r, w=1 + t % 3)
        orc.add(0, r, w=1 + t % 3)
        nodes, pos, score = poa.last_alignment()
        on, op, os_ = orc.last_alignment()
        adds += 1
        why = []
        if score != want:
            why.append(f"device {score}, recurrence {want}")
        elif mode_path_score(bases, ef, et, r, nodes, pos, T) != score or boundary_violations(ef, et, len(bases), len(r), nodes, pos, T):
            why.append("the path does not rescore or breaks the type's boundaries")
        if score != os_ or nodes.tolist() != on.tolist() or pos.tolist() != op.tolist():
            why.append(f"the oracle's alignment differs (score {os_}, {len(on)} pairs against {len(nodes)})")
        db, ob = poa.graph(0), orc.graph(0)
        if db[0] != ob[0] or db[1].tolist() != ob[1].tolist() or sorted(zip(*(x.tolist() for x in db[2:]))) != sorted(zip(*(x.tolist() for x in ob[2:]))):
            why.append("the oracle's graph differs")
        if why:
            bad += 1
            print(f"MISMATCH type {T} graph {g} add {t}: {'; '.join(why)}; nodes {len(bases)}, read {len(r)}", flush=True)
            break
    poa.close()
    orc.close()
    print(f"graph {g}: {adds} additions checked, {bad} mismatches, {time.time() - t0:.0f} s", flush=True)
print(f"done: type {T}, {adds} additions, {bad} mismatches")
sys.exit(1 if bad else 0)
