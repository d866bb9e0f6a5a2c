#!/usr/bin/env python3
"""What the consensus of each side of a split costs when it is called from the reads' planes (align_pairs_split_polish) and when
it is reached the way the parent commit has it: align_pairs_split, then align_pairs_polish over the pairs of group 0 and over
those of group 1, which aligns every grouped read a second time.

    tools/align_split_polish_bench.py [CALLS=7]

Two batches — 192 pairs of 3 kb on 12 segments (the batch of profiles/align_split.txt) and 3000 reads of two variants of one
300-base segment.  Per batch, after two warm-up calls of each route, CALLS rounds of: the fused call, the two-call route, the
split alone, in turn; wall milliseconds per call as median (min - max).  Then the device times of k_ops_project,
k_ops_project_ins, k_plane_pile and k_pile_call from the fused call's IOC_TRACE lines.  The last fused call is held against the
two-call route's sequences.  profiles/align_split_polish.txt holds the tables."""
import random
import re
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from isonclust2_amd import api  # noqa: E402
from align_split_bench import SPLIT, mutate, sliced, traced  # noqa: E402


def two_variants(n=3000):
    rng = random.Random(19)
    ref = bytes(rng.choice(b"ACGT") for _ in range(300))
    alt = bytearray(ref)
    for p in range(20, 290, 45):
        alt[p] = next(b for b in b"ACGT" if b != ref[p])
    alt = bytes(alt[:150] + b"GATTACA"[:3] + alt[150:])
    seqs = [ref] + [mutate(rng, alt if i % 3 == 0 else ref, 0.05) for i in range(n)]
    return f"{n} reads of two variants on one 300-base segment", seqs, [(1 + i, 0, 0, 0.2) for i in range(n)], [(0, 0)], [0] * n, dict(min_depth=3, min_alt=3, min_pct=10)


def two_calls(ctx, pairs, segs, sop, rule):
    got = ctx.align_pairs_split(pairs, 11, segs, sop, **rule, **SPLIT)
    out = []
    for h in (0, 1):
        sub = [i for i in range(len(pairs)) if got["group"][i] == h]
        out.append(ctx.align_pairs_polish([pairs[i] for i in sub], 11, segs, [sop[i] for i in sub]))
    return got, out


def main(calls):
    ctx = api.Context(0)
    ok = True
    for name, seqs, pairs, segs, sop, rule in (sliced(), two_variants()):
        ctx.align_set_pool(seqs)
        routes = {"fused (align_pairs_split_polish)": lambda: ctx.align_pairs_split_polish(pairs, 11, segs, sop, **rule, **SPLIT),
                  "split, then polish per group": lambda: two_calls(ctx, pairs, segs, sop, rule),
                  "align_pairs_split alone": lambda: ctx.align_pairs_split(pairs, 11, segs, sop, **rule, **SPLIT)}
        for fn in routes.values():
            fn(), fn()
        ms = {k: [] for k in routes}
        for _ in range(calls):
            for k, fn in routes.items():
                t0 = time.perf_counter()
                fn()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        fused = routes["fused (align_pairs_split_polish)"]()
        split, per_group = routes["split, then polish per group"]()
        same = all(fused["gseq"][g][h] == per_group[h]["seq"][g] and fused["gqual"][g][h] == per_group[h]["qual"][g] for g in range(len(segs)) for h in (0, 1))
        ok = ok and same and fused["group"].tolist() == split["group"].tolist()
        groups = [int((fused["group"] == h).sum()) for h in (0, 1, api.SPLIT_NONE)]
        print(f"{name}: {len(pairs)} pairs; reads in group 0 / 1 / neither: {groups[0]} / {groups[1]} / {groups[2]}; "
              f"{int((fused['seg']['seed'] >= 0).sum())} of {len(segs)} segments split")
        print(f"  wall ms per call: median (min - max) over {calls} calls, the three in turn")
        for k, v in ms.items():
            print(f"  {k:<34} {statistics.median(v):9.3f} ({min(v):.3f} - {max(v):.3f})")
        print(f"  the fused call's sequences and qualities equal the two-call route's: {'yes' if same else 'NO'}")
        names = ("k_ops_pileup", "k_ops_project", "k_ops_project_ins", "k_plane_pile", "k_pile_call")
        dev = {k: [] for k in names}
        for _ in range(calls):
            _, text = traced(routes["fused (align_pairs_split_polish)"])
            lines = " ".join(ln.strip() for ln in text.splitlines() if "aligner: sites:" in ln or "aligner: split polish:" in ln)
            for k in names:
                dev[k].append(float(re.search(re.escape(k) + r" ([0-9.]+) ms", lines).group(1)))
        print(f"  {'kernel':<18} device ms: median (min - max) over {calls} calls")
        for k in names:
            print(f"  {k:<18} {statistics.median(dev[k]):8.3f} ({min(dev[k]):.3f} - {max(dev[k]):.3f})")
    ctx.close()
    return ok


if __name__ == "__main__":
    sys.exit(0 if main(int(sys.argv[1]) if len(sys.argv) > 1 else 7) else 1)
