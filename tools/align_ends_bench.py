#!/usr/bin/env python3
"""What the alternative ends cost (align_pairs_blocks_ends), beside the call it extends: align_pairs_blocks, the same alignment,
pile, projection and block kernels without the stage and, where no statistics are asked, without k_ops_stats.

    tools/align_ends_bench.py [CALLS=6] [--blocks-only]

One batch: two segments of 1500 bases with 600 reads each, in the proportions of property case A of tests/ends_common.py — 10 in 33
reads of the whole representative, 10 of its first 1200 bases, 10 from base 250 on and 3 that start anywhere in the first 1000 —
mutated at 8 %.  After two warm-up calls of each route, CALLS rounds of the calls in turn; wall milliseconds per call as median (min
- max).  Then the device times from the IOC_TRACE line of the fused call: each of the eight kernels of ioc_read_ends.hip on its
own, beside k_ops_pileup, k_ops_project, ms_blocks and k_ops_stats.  --blocks-only measures align_pairs_blocks alone: run from the
root of a checkout of the parent commit, which has no align_pairs_blocks_ends, it gives the figure the fused call is held against.
profiles/read_ends.txt holds the tables."""
import random
import re
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from isonclust2_amd import api  # noqa: E402
from align_split_bench import mutate, traced  # noqa: E402

KERNELS = ("k_end_hist", "k_end_rows", "k_end_list", "k_end_class", "k_end_count", "k_end_support", "k_end_variants", "k_ends_record")


def two_segments(n=600):
    rng = random.Random(31)
    seqs, pairs, sop = [], [], []
    frames = [bytes(rng.choice(b"ACGT") for _ in range(1500)) for _ in range(2)]
    seqs += frames
    for g, R in enumerate(frames):
        for i in range(n):
            x = i % 33
            part = R if x < 10 else R[:1200] if x < 20 else R[250:] if x < 30 else R[rng.randrange(0, 1001):]
            pairs.append((len(seqs), g, 0, 0.2))
            seqs.append(mutate(rng, part, 0.08))
            sop.append(g)
    return f"{n} reads on each of two 1500-base segments, three classes of ends", seqs, pairs, [(0, 0), (1, 0)], sop


def main(calls, blocks_only):
    ctx = api.Context(0)
    name, seqs, pairs, segs, sop = two_segments()
    ctx.align_set_pool(seqs)
    routes = {"align_pairs_blocks": lambda: ctx.align_pairs_blocks(pairs, 11, segs, sop)}
    if not blocks_only:
        routes["align_pairs_blocks, stats"] = lambda: ctx.align_pairs_blocks(pairs, 11, segs, sop, stats=True)
        routes["align_pairs_blocks_ends"] = lambda: ctx.align_pairs_blocks_ends(pairs, 11, segs, sop)
        routes["align_pairs_blocks_ends, no rows"] = lambda: ctx.align_pairs_blocks_ends(pairs, 11, segs, sop, rows=False)
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
        ctx.close()
        return 0
    got = routes["align_pairs_blocks_ends"]()
    ends = got["ends"]
    print("  end records:", [tuple(int(v) for v in z) for z in ends["seg"]])
    print("  start sites of segment 0:", [tuple(int(v) for v in s)[:6] for s in ends["starts"][0]], "stop sites:", [tuple(int(v) for v in s)[:6] for s in ends["stops"][0]])
    print("  variants of segment 0:", ends["variants"][0].tolist())
    names = ("k_ops_pileup", "k_ops_project", "ms_blocks", "k_ops_stats") + KERNELS
    dev = {k: [] for k in names}
    for _ in range(calls):
        _, text = traced(routes["align_pairs_blocks_ends"])
        line = " ".join(ln.strip() for ln in text.splitlines() if "aligner: blocks ends:" in ln)
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
    sys.exit(main(int(args[0]) if args else 6, "--blocks-only" in sys.argv[1:]))
