#!/usr/bin/env python3
"""What the correction of every read against its own isoform costs (align_pairs_blocks_correct), on the two read sets of
tools/align_correct_bench.py, beside align_pairs_correct (k_read_correct: every read against its whole cluster) and beside the
route a caller had before the fused call: align_pairs_blocks_polish for the isoforms, the planes projected on the host from
align_pairs_ops' bytes, the tables of every isoform piled on the host, and planes_correct once per isoform.

    tools/align_iso_correct_bench.py [CALLS=7]

Two batches — 192 pairs of 3 kb on 12 segments and 3000 reads of two variants of one 300-base segment.  Per batch, after two
warm-up calls of each route, CALLS rounds of the calls in turn; wall milliseconds per call as median (min - max).  The earlier route
is timed once: its host projections take seconds.  Then the device times from the IOC_TRACE lines: k_iso_correct (both passes and
the scan) and k_group_pile of the fused call, k_read_correct of align_pairs_correct.  profiles/iso_correct.txt holds the tables."""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from isonclust2_amd import api  # noqa: E402
from align_correct_bench import device_ms  # noqa: E402
from align_split_bench import sliced  # noqa: E402
from align_split_polish_bench import two_variants  # noqa: E402


def earlier_route(ctx, seqs, pairs, segs, sop):
    """isoforms from align_pairs_blocks_polish, then planes_correct per isoform on tables piled from host planes"""
    got = ctx.align_pairs_blocks_polish(pairs, 11, segs, sop, rows=False)
    ops = ctx.align_pairs_ops(pairs, 11)[3]
    frames = [seqs[s[0]] for s in segs]
    base = [api.ops_project(o, seqs[p[0]], len(frames[g]))[0] for o, p, g in zip(ops, pairs, sop)]
    slots = [api.ops_project_ins(o, seqs[p[0]], len(frames[g])) for o, p, g in zip(ops, pairs, sop)]
    group, calls = got["reads"]["group"], 0
    for g, frame in enumerate(frames):
        for h in sorted(set(int(group[i]) for i in range(len(pairs)) if sop[i] == g)):
            mine = [i for i in range(len(pairs)) if sop[i] == g and int(group[i]) == h]
            cols, ins = np.zeros(len(frame) + 1, api.PILEUP_DTYPE), np.zeros(len(frame) + 1, api.PILEUP_INS_DTYPE)
            for i in mine:
                api.planes_pile(base[i], slots[i], cols=cols, ins=ins)
            ctx.planes_correct([frame], cols, ins, [0] * len(mine), [base[i] for i in mine], [slots[i] for i in mine])
            calls += 1
    return calls


def main(calls):
    ctx = api.Context(0)
    for name, seqs, pairs, segs, sop, _ in (sliced(), two_variants()):
        ctx.align_set_pool(seqs)
        routes = {"align_pairs_blocks_correct": lambda: ctx.align_pairs_blocks_correct(pairs, 11, segs, sop, rows=False),
                  "align_pairs_correct": lambda: ctx.align_pairs_correct(pairs, 11, segs, sop),
                  "align_pairs_blocks": lambda: ctx.align_pairs_blocks(pairs, 11, segs, sop, rows=False)}
        for fn in routes.values():
            fn(), fn()
        ms = {k: [] for k in routes}
        for _ in range(calls):
            for k, fn in routes.items():
                t0 = time.perf_counter()
                fn()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        got = routes["align_pairs_blocks_correct"]()
        total = {f: int(got["correct"][f].sum()) for f in api.ISO_CORRECT_STATS_FIELDS if f != "table"}
        print(f"{name}: {len(pairs)} pairs; {int((got['correct']['table'] >= 0).sum())} held against an isoform's table; the records summed: {total}")
        print(f"  wall ms per call: median (min - max) over {calls} calls, the three in turn")
        for k, v in ms.items():
            print(f"  {k:<28} {statistics.median(v):9.3f} ({min(v):.3f} - {max(v):.3f})")
        t0 = time.perf_counter()
        n = earlier_route(ctx, seqs, pairs, segs, sop)
        print(f"  the earlier route (blocks_polish, host planes and tables, {n} calls of planes_correct), once: {(time.perf_counter() - t0) * 1e3:9.1f} ms")
        dev = device_ms(routes["align_pairs_blocks_correct"], ("aligner: blocks correct:",),
                        ("k_ops_project_ins", "k_ops_project_ilen", "k_ops_project_qpos", "ms_blocks", "k_group_pile", "k_iso_correct"), calls)
        dev.update(device_ms(routes["align_pairs_correct"], ("aligner: correct:",), ("k_read_correct",), calls))
        print(f"  {'kernel':<18} device ms: median (min - max) over {calls} calls (k_read_correct: of align_pairs_correct)")
        for k, v in dev.items():
            print(f"  {k:<18} {statistics.median(v):8.3f} ({min(v):.3f} - {max(v):.3f})")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 7))
