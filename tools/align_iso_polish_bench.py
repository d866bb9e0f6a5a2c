#!/usr/bin/env python3
"""What the consensus of every isoform costs (align_pairs_blocks_polish), on the three batches of tools/align_blocks_bench.py.

    tools/align_iso_polish_bench.py [CALLS=7] [--blocks-only] [--no-kernels]

(a) and (b), per batch, after two warm-up calls of each route, CALLS rounds of the routes in turn; wall milliseconds per call as
median (min - max):
  align_pairs_blocks            the call without the new stage.  --blocks-only measures it alone: run from the root of a checkout
                                of the parent commit, which has no align_pairs_blocks_polish, it gives the figure (a) is held against;
  align_pairs_blocks_polish     the fused call;
  blocks, then polish per iso   the only route there was: align_pairs_blocks, then one align_pairs_polish per isoform over its
                                direct and assigned reads — every read of an isoform is aligned a second time.
Then the device times of the fused call's kernels from its IOC_TRACE line.
(c) k_group_pile with two groups against k_plane_pile on the same host planes (the host aligner and both host projections make
them once per batch; the groups are the variants the reads were drawn from): planes_polish and planes_polish_groups in turn,
two series of CALLS calls each, device milliseconds from their IOC_TRACE lines.  The difference between the two series of one
kernel is the run-to-run spread the other kernel's figure is held against.  --no-kernels leaves (c) out.
profiles/iso_polish.txt holds the tables."""
import random
import re
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from isonclust2_amd import api  # noqa: E402
from align_blocks_bench import four_isoforms  # noqa: E402
from align_split_bench import sliced, traced  # noqa: E402
from align_split_polish_bench import two_variants  # noqa: E402


def fmt(v):
    return f"{statistics.median(v):9.3f} ({min(v):.3f} - {max(v):.3f})"


def per_isoform(ctx, pairs, segs, sop):
    """the route without the stage: the blocks, then a polish call per isoform over its reads"""
    got = ctx.align_pairs_blocks(pairs, 11, segs, sop, rows=False)
    out = []
    for g in range(len(segs)):
        for h in range(int(got["seg"][g]["n_groups"])):
            mine = [x for x in range(len(pairs)) if sop[x] == g and int(got["reads"][x]["group"]) == h]
            out.append(ctx.align_pairs_polish([pairs[x] for x in mine], 11, [segs[g]], [0] * len(mine)))
    return got, out


def device_ms(fn, mark, names, calls):
    dev = {k: [] for k in names}
    for _ in range(calls):
        _, text = traced(fn)
        line = " ".join(ln.strip() for ln in text.splitlines() if mark in ln)
        for k in names:
            dev[k].append(float(re.search(re.escape(k) + r" ([0-9.]+) ms", line).group(1)))
    return dev


def host_planes(seqs, pairs, segs, sop):
    """every pair's planes through the host aligner and both host projections (the reference reverse-complemented where asked)"""
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    base, slots, seen = [], [], {}
    for q, r, rc, _ in pairs:
        if (q, r, rc) not in seen:   # (the first batch repeats its 24 pairs: the host aligner takes seconds for 3 kb)
            ref = seqs[r].translate(comp)[::-1] if rc else seqs[r]
            ops, _ = api.host_align_ops(seqs[q], ref)
            seen[q, r, rc] = api.ops_project(ops, seqs[q], len(ref))[0], api.ops_project_ins(ops, seqs[q], len(ref))
        base.append(seen[q, r, rc][0]), slots.append(seen[q, r, rc][1])
    frames = [seqs[r].translate(comp)[::-1] if rc else seqs[r] for r, rc in segs]
    return frames, base, slots


def main(calls, blocks_only, kernels):
    ctx = api.Context(0)
    batches = (sliced(), two_variants(), four_isoforms())
    # which of two groups a pair is in: the variant its read was drawn from (the first batch has none: odd and even pairs)
    two = (lambda i: i % 2, lambda i: int(i % 3 == 0), lambda i: ((i * 7) % 4) % 2)
    for (name, seqs, pairs, segs, sop, _), side in zip(batches, two):
        ctx.align_set_pool(seqs)
        routes = {"align_pairs_blocks": lambda: ctx.align_pairs_blocks(pairs, 11, segs, sop, rows=False)}
        if not blocks_only:
            routes["align_pairs_blocks_polish"] = lambda: ctx.align_pairs_blocks_polish(pairs, 11, segs, sop, rows=False)
            routes["blocks, then polish per iso"] = lambda: per_isoform(ctx, pairs, segs, sop)
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
            print(f"  {k:<30} {fmt(v)}")
        if blocks_only:
            continue
        got = routes["align_pairs_blocks_polish"]()
        print("  isoforms called per segment:", [len(s) for s in got["gseq"]][:12], "bytes:", sum(len(q) for s in got["gseq"] for q in s))
        names = ("k_ops_pileup", "k_ops_project", "k_ops_project_ins", "ms_blocks", "k_group_pile", "k_pile_call")
        print(f"  {'kernel':<18} device ms of the fused call: median (min - max) over {calls} calls")
        for k, v in device_ms(routes["align_pairs_blocks_polish"], "aligner: blocks polish:", names, calls).items():
            print(f"  {k:<18} {fmt(v)}")
        if not kernels:
            continue
        frames, base, slots = host_planes(seqs, pairs, segs, sop)
        group = [side(i) for i in range(len(pairs))]
        old = lambda: ctx.planes_polish(frames, sop, group, base, slots)
        new = lambda: ctx.planes_polish_groups(frames, sop, group, [2] * len(frames), base, slots)
        a, b = old(), new()
        assert a["gseq"] == b["gseq"] and a["gqual"] == b["gqual"]
        old(), new()
        print(f"  two groups a segment on the same planes, device ms: median (min - max) over {calls} calls, two series each, in turn")
        for series in (1, 2):
            print(f"  k_plane_pile  series {series}  {fmt(device_ms(old, 'planes polish:', ('k_plane_pile',), calls)['k_plane_pile'])}")
            print(f"  k_group_pile  series {series}  {fmt(device_ms(new, 'planes polish groups:', ('k_group_pile',), calls)['k_group_pile'])}")
    ctx.close()
    return 0


if __name__ == "__main__":
    flags = ("--blocks-only", "--no-kernels")
    args = [a for a in sys.argv[1:] if a not in flags]
    sys.exit(main(int(args[0]) if args else 7, "--blocks-only" in sys.argv[1:], "--no-kernels" not in sys.argv[1:]))
