#!/usr/bin/env python3
"""What the quality-weighted consensus of every isoform costs (align_pairs_blocks_polish_weighted), on the three batches of
tools/align_iso_polish_bench.py under random quality lines (bytes '!' + 2 .. 42).

    tools/align_iso_polish_weighted_bench.py [CALLS=7] [--unweighted-only]

(a) per batch, after two warm-up calls of each route, CALLS rounds of the routes in turn; wall milliseconds per call as median
(min - max):
  align_pairs_blocks_polish            the unweighted fused call.  --unweighted-only measures it alone: run from the root of a
                                       checkout of the parent commit, which has no weighted call, it gives the figure (a) is held
                                       against;
  align_pairs_blocks_polish_weighted   the weighted fused call.
(b) the device times of the kernels of both calls from their IOC_TRACE lines, CALLS calls each, two series in turn:
k_ops_project_weights beside k_ops_project_ins, k_group_pile_weighted beside k_group_pile (the same isoforms, the same member
lists: everything in front of the pile is the same call), and the call kernels in both modes.  The difference between the two
series of one kernel is the run-to-run spread.
profiles/iso_polish_weighted.txt holds the tables."""
import re
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from isonclust2_amd import api  # noqa: E402
from align_blocks_bench import four_isoforms  # noqa: E402
from align_split_bench import sliced, traced  # noqa: E402
from align_split_polish_bench import two_variants  # noqa: E402


def fmt(v):
    return f"{statistics.median(v):9.3f} ({min(v):.3f} - {max(v):.3f})"


def device_ms(fn, mark, names, calls):
    dev = {k: [] for k in names}
    for _ in range(calls):
        _, text = traced(fn)
        line = " ".join(ln.strip() for ln in text.splitlines() if mark in ln)
        for k in names:
            dev[k].append(float(re.search(re.escape(k) + r" ([0-9.]+) ms", line).group(1)))
    return dev


PLAIN = ("k_ops_project_ins", "k_group_pile", "k_pile_call")
WEIGHTED = ("k_ops_project_ins", "k_ops_project_weights", "k_group_pile_weighted", "k_pile_call<weighted>")


def main(calls, unweighted_only):
    ctx = api.Context(0)
    rng = np.random.default_rng(31)
    for name, seqs, pairs, segs, sop, _ in (sliced(), two_variants(), four_isoforms()):
        ctx.align_set_pool(seqs)
        ctx.align_set_pool_qual([rng.integers(35, 76, len(s)).astype(np.uint8).tobytes() for s in seqs])
        routes = {"align_pairs_blocks_polish": lambda: ctx.align_pairs_blocks_polish(pairs, 11, segs, sop, rows=False)}
        if not unweighted_only:
            routes["align_pairs_blocks_polish_weighted"] = lambda: ctx.align_pairs_blocks_polish_weighted(pairs, 11, segs, sop, rows=False)
        for fn in routes.values():
            fn(), fn()
        ms = {k: [] for k in routes}
        for _ in range(calls):
            for k, fn in routes.items():
                t0 = time.perf_counter()
                fn()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        print(f"{name}: {len(pairs)} pairs")
        print(f"  wall ms per call: median (min - max) over {calls} calls, the routes in turn")
        for k, v in ms.items():
            print(f"  {k:<36} {fmt(v)}")
        if unweighted_only:
            continue
        plain, got = routes["align_pairs_blocks_polish"](), routes["align_pairs_blocks_polish_weighted"]()
        assert plain["reads"].tobytes() == got["reads"].tobytes() and plain["gseg_off"].tolist() == got["gseg_off"].tolist()
        differ = sum(a != b for s, t in zip(plain["gseq"], got["gseq"]) for a, b in zip(s, t))
        print("  isoforms called per segment:", [len(s) for s in got["gseq"]][:12], "bytes:", sum(len(q) for s in got["gseq"] for q in s),
              "sequences that differ from the unweighted call's:", differ)
        print(f"  device ms from the IOC_TRACE lines: median (min - max) over {calls} calls, two series of each call in turn")
        for series in (1, 2):
            for k, v in device_ms(routes["align_pairs_blocks_polish"], "aligner: blocks polish:", PLAIN, calls).items():
                print(f"  unweighted  series {series}  {k:<24} {fmt(v)}")
            for k, v in device_ms(routes["align_pairs_blocks_polish_weighted"], "aligner: blocks polish weighted:", WEIGHTED, calls).items():
                print(f"  weighted    series {series}  {k:<24} {fmt(v)}")
    ctx.close()
    return 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--unweighted-only"]
    sys.exit(main(int(args[0]) if args else 7, "--unweighted-only" in sys.argv[1:]))
