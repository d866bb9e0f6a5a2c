#!/usr/bin/env python3
"""What the exon blocks cost (align_pairs_blocks), on the read sets of tools/align_correct_bench.py and on one with isoforms,
beside the call it shares its alignments' cost with: align_pairs_alleles, the same alignment, pile and projection without the stage
(and with the site search and the allele gather instead).

    tools/align_blocks_bench.py [CALLS=7] [--alleles-only]

Three batches — 192 pairs of 3 kb on 12 segments, 3000 reads of two variants of one 300-base segment, and 1200 reads of four
isoforms of one 1000-base segment (blocks_common's cuts, 8 % errors).  Per batch, after two warm-up calls of each route, CALLS
rounds of the calls in turn; wall milliseconds per call as median (min - max).  Then the device times from the IOC_TRACE line of
the fused call: ms_blocks (the eight kernels of ioc_read_blocks.hip together) beside k_ops_pileup and k_ops_project.
--alleles-only measures align_pairs_alleles alone: run from the root of a checkout of the parent commit, which has no
align_pairs_blocks, it gives the figure the fused call is held against.  profiles/read_blocks.txt holds the tables."""
import random
import re
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from isonclust2_amd import api  # noqa: E402
from align_split_bench import mutate, sliced, traced  # noqa: E402
from align_split_polish_bench import two_variants  # noqa: E402


def four_isoforms(n=1200):
    rng = random.Random(29)
    T = bytes(rng.choice(b"ACGT") for _ in range(1000))
    iso = [T, T[:150] + T[190:], T[:150] + T[190:400] + T[520:], T[:400] + T[520:]]
    seqs = [T] + [mutate(rng, iso[(i * 7) % 4], 0.08) for i in range(n)]
    return f"{n} reads of four isoforms on one 1000-base segment", seqs, [(1 + i, 0, 0, 0.2) for i in range(n)], [(0, 0)], [0] * n, dict(min_depth=3, min_alt=3, min_pct=25)


def main(calls, alleles_only):
    ctx = api.Context(0)
    for name, seqs, pairs, segs, sop, rule in (sliced(), two_variants(), four_isoforms()):
        ctx.align_set_pool(seqs)
        routes = {"align_pairs_alleles": lambda: ctx.align_pairs_alleles(pairs, 11, segs, sop, **rule)}
        if not alleles_only:
            routes["align_pairs_blocks"] = lambda: ctx.align_pairs_blocks(pairs, 11, segs, sop)
            routes["align_pairs_blocks, no rows"] = lambda: ctx.align_pairs_blocks(pairs, 11, segs, sop, rows=False)
        for fn in routes.values():
            fn(), fn()
        ms = {k: [] for k in routes}
        for _ in range(calls):
            for k, fn in routes.items():
                t0 = time.perf_counter()
                fn()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        print(f"{name}: {len(pairs)} pairs")
        print(f"  wall ms per call: median (min - max) over {calls} calls, the calls in turn")
        for k, v in ms.items():
            print(f"  {k:<28} {statistics.median(v):9.3f} ({min(v):.3f} - {max(v):.3f})")
        if alleles_only:
            continue
        got = routes["align_pairs_blocks"]()
        print("  records:", [tuple(int(v) for v in z) for z in got["seg"]][:3], "blocks of segment 0:", [(int(b["first"]), int(b["end"])) for b in got["blocks"][0]][:4])
        names = ("k_ops_pileup", "k_ops_project", "ms_blocks")
        dev = {k: [] for k in names}
        for _ in range(calls):
            _, text = traced(routes["align_pairs_blocks"])
            line = " ".join(ln.strip() for ln in text.splitlines() if "aligner: blocks:" in ln)
            for k in names:
                dev[k].append(float(re.search(re.escape(k) + r" ([0-9.]+) ms", line).group(1)))
        print(f"  {'kernel':<18} device ms: median (min - max) over {calls} calls")
        for k, v in dev.items():
            print(f"  {k:<18} {statistics.median(v):8.3f} ({min(v):.3f} - {max(v):.3f})")
    ctx.close()
    return 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--alleles-only"]
    sys.exit(main(int(args[0]) if args else 7, "--alleles-only" in sys.argv[1:]))
