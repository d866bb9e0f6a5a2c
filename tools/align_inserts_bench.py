#!/usr/bin/env python3
"""What the insertion sites cost (align_pairs_blocks_inserts), on the three batches of tools/align_blocks_bench.py and on one whose
representative lacks both exons, beside the call it extends: align_pairs_blocks, the same alignment, pile, projection and block
kernels without the length plane and the stage.

    tools/align_inserts_bench.py [CALLS=7] [--blocks-only]

Four batches — 192 pairs of 3 kb on 12 segments, 3000 reads of two variants of one 300-base segment, 1200 reads of four isoforms of
one 1000-base segment whose representative is the longest of them, and the same 1200 reads against the isoform that lacks both
exons (840 bases: two insertion sites and no block).  Per batch, after two warm-up calls of each route, CALLS rounds of the calls
in turn; wall milliseconds per call as median (min - max).  Then the device times from the IOC_TRACE line of the fused call:
k_ops_project_ilen and each of the eight kernels of ioc_read_inserts.hip on its own, beside k_ops_pileup, k_ops_project and
ms_blocks.  --blocks-only measures align_pairs_blocks alone: run from the root of a checkout of the parent commit, which has no
align_pairs_blocks_inserts, it gives the figure the fused call is held against.  profiles/read_inserts.txt holds the tables."""
import random
import re
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from isonclust2_amd import api  # noqa: E402
from align_blocks_bench import four_isoforms  # noqa: E402
from align_split_bench import mutate, sliced, traced  # noqa: E402
from align_split_polish_bench import two_variants  # noqa: E402

KERNELS = ("k_ins_bits", "k_ins_rows", "k_ins_list", "k_ins_states", "k_ins_lens", "k_ins_support", "k_ins_isoforms", "k_ins_record")


def short_representative(n=1200):
    rng = random.Random(29)
    T = bytes(rng.choice(b"ACGT") for _ in range(1000))
    iso = [T, T[:150] + T[190:], T[:150] + T[190:400] + T[520:], T[:400] + T[520:]]
    seqs = [iso[2]] + [mutate(rng, iso[(i * 7) % 4], 0.08) for i in range(n)]
    return f"{n} reads of four isoforms on the 840-base isoform that lacks both exons", seqs, [(1 + i, 0, 0, 0.2) for i in range(n)], [(0, 0)], [0] * n, {}


def main(calls, blocks_only):
    ctx = api.Context(0)
    for name, seqs, pairs, segs, sop, _ in (sliced(), two_variants(), four_isoforms(), short_representative()):
        ctx.align_set_pool(seqs)
        routes = {"align_pairs_blocks": lambda: ctx.align_pairs_blocks(pairs, 11, segs, sop)}
        if not blocks_only:
            routes["align_pairs_blocks_inserts"] = lambda: ctx.align_pairs_blocks_inserts(pairs, 11, segs, sop)
            routes["align_pairs_blocks_inserts, no rows"] = lambda: ctx.align_pairs_blocks_inserts(pairs, 11, segs, sop, rows=False)
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
            print(f"  {k:<36} {statistics.median(v):9.3f} ({min(v):.3f} - {max(v):.3f})")
        if blocks_only:
            continue
        got = routes["align_pairs_blocks_inserts"]()
        print("  block records:", [tuple(int(v) for v in z) for z in got["seg"]][:2], "insert records:", [tuple(int(v) for v in z) for z in got["inserts"]["seg"]][:2])
        print("  sites of segment 0:", [tuple(int(v) for v in s)[:7] for s in got["inserts"]["sites"][0]][:4])
        names = ("k_ops_pileup", "k_ops_project", "k_ops_project_ilen", "ms_blocks") + KERNELS
        dev = {k: [] for k in names}
        for _ in range(calls):
            _, text = traced(routes["align_pairs_blocks_inserts"])
            line = " ".join(ln.strip() for ln in text.splitlines() if "aligner: blocks inserts:" in ln)
            for k in names:
                dev[k].append(float(re.search(re.escape(k) + r" ([0-9.]+) ms", line).group(1)))
        print(f"  {'kernel':<20} device ms: median (min - max) over {calls} calls")
        for k, v in dev.items():
            print(f"  {k:<20} {statistics.median(v):8.3f} ({min(v):.3f} - {max(v):.3f})")
        print(f"  {'the eight together':<20} {sum(statistics.median(dev[k]) for k in KERNELS):8.3f}")
    ctx.close()
    return 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--blocks-only"]
    sys.exit(main(int(args[0]) if args else 7, "--blocks-only" in sys.argv[1:]))
