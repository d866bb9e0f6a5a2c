#!/usr/bin/env python3
"""What the correction of every read costs (align_pairs_correct), on the read sets of tools/align_split_polish_bench.py, beside the
calls it shares its alignments' cost with: align_pairs_polish (the same pile without the planes and without the correction) and
align_pairs_split_polish (whose k_plane_pile and k_pile_call are the yardstick for a stage that reads the same planes and tables).

    tools/align_correct_bench.py [CALLS=7]

Two batches — 192 pairs of 3 kb on 12 segments and 3000 reads of two variants of one 300-base segment.  Per batch, after two
warm-up calls of each route, CALLS rounds of the three calls in turn; wall milliseconds per call as median (min - max).  Then the
device times from the IOC_TRACE lines: k_read_correct (both passes and the scan) of the correcting call, and k_plane_pile and
k_pile_call of align_pairs_split_polish on the same pairs.  profiles/read_correct.txt holds the tables."""
import re
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from isonclust2_amd import api  # noqa: E402
from align_split_bench import SPLIT, sliced, traced  # noqa: E402
from align_split_polish_bench import two_variants  # noqa: E402


def device_ms(fn, line, names, calls):
    dev = {k: [] for k in names}
    for _ in range(calls):
        _, text = traced(fn)
        lines = " ".join(ln.strip() for ln in text.splitlines() if any(w in ln for w in line))
        for k in names:
            dev[k].append(float(re.search(re.escape(k) + r" ([0-9.]+) ms", lines).group(1)))
    return dev


def main(calls):
    ctx = api.Context(0)
    for name, seqs, pairs, segs, sop, rule in (sliced(), two_variants()):
        ctx.align_set_pool(seqs)
        routes = {"align_pairs_correct": lambda: ctx.align_pairs_correct(pairs, 11, segs, sop),
                  "align_pairs_polish": lambda: ctx.align_pairs_polish(pairs, 11, segs, sop),
                  "align_pairs_split_polish": lambda: ctx.align_pairs_split_polish(pairs, 11, segs, sop, **rule, **SPLIT)}
        for fn in routes.values():
            fn(), fn()
        ms = {k: [] for k in routes}
        for _ in range(calls):
            for k, fn in routes.items():
                t0 = time.perf_counter()
                fn()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        got = routes["align_pairs_correct"]()
        total = {f: int(got["correct"][f].sum()) for f in api.CORRECT_STATS_FIELDS}
        print(f"{name}: {len(pairs)} pairs; the corrections' records summed: {total}")
        print(f"  wall ms per call: median (min - max) over {calls} calls, the three in turn")
        for k, v in ms.items():
            print(f"  {k:<26} {statistics.median(v):9.3f} ({min(v):.3f} - {max(v):.3f})")
        dev = device_ms(routes["align_pairs_correct"], ("aligner: correct:",), ("k_ops_pileup<ins>", "k_ops_project", "k_ops_project_ins", "k_read_correct"), calls)
        dev.update(device_ms(routes["align_pairs_split_polish"], ("aligner: split polish:",), ("k_plane_pile", "k_pile_call"), calls))
        print(f"  {'kernel':<18} device ms: median (min - max) over {calls} calls (k_plane_pile, k_pile_call: of align_pairs_split_polish)")
        for k, v in dev.items():
            print(f"  {k:<18} {statistics.median(v):8.3f} ({min(v):.3f} - {max(v):.3f})")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 7))
