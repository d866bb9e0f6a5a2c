#!/usr/bin/env python3
"""What the sequence of an inserted exon costs (align_pairs_blocks_inserts_seq), on the four batches of tools/align_inserts_bench.py,
beside the call it extends and beside the only other route to the exon there is.

    tools/align_insert_windows_bench.py [CALLS=7] [--inserts-only]

Per batch, after two warm-up calls of each route, CALLS rounds of the calls in turn; wall milliseconds per call of the Python
wrapper as median (min - max):
  (a) align_pairs_blocks_inserts (the call the fused one extends; --inserts-only measures it alone: run from the root of a checkout
      of the parent commit it gives the parent's figure) and align_pairs_blocks_inserts_seq;
  (b) align_pairs_blocks_inserts followed by align_pairs_blocks of the same reads with a CARRIER as the representative — the advice
      the insert stage gave: every pair aligned a second time.
Then (c) the device times from the IOC_TRACE line of the fused call: k_ops_project_qpos and each window kernel on its own, and with
IOC_WIN_SPLIT k_win_align as its fill and its walk.  profiles/insert_windows.txt holds the tables."""
import os
import re
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from isonclust2_amd import api  # noqa: E402
from align_blocks_bench import four_isoforms  # noqa: E402
from align_inserts_bench import short_representative  # noqa: E402
from align_split_bench import sliced, traced  # noqa: E402
from align_split_polish_bench import two_variants  # noqa: E402

KERNELS = ("k_ops_project_ilen", "k_ops_project_qpos", "k_win_bounds", "k_win_template", "k_win_align", "k_win_align_walk", "k_win_group_pile", "k_win_pile_call")


def device_times(fn, calls):
    dev = {k: [] for k in KERNELS}
    for _ in range(calls):
        _, text = traced(fn)
        line = " ".join(ln.strip() for ln in text.splitlines() if "aligner: blocks inserts seq:" in ln)
        for k in KERNELS:
            dev[k].append(float(re.search(re.escape(k) + r" ([0-9.]+) ms", line).group(1)))
    return dev


def main(calls, inserts_only):
    ctx = api.Context(0)
    for name, seqs, pairs, segs, sop, _ in (sliced(), two_variants(), four_isoforms(), short_representative()):
        carrier = list(seqs)
        if len(segs) == 1:
            carrier[segs[0][0]] = max((seqs[p[0]] for p in pairs), key=len)   # the longest read stands for "a carrier that holds all the exons"
        ctx.align_set_pool(seqs)
        routes = {"(a) align_pairs_blocks_inserts": lambda: ctx.align_pairs_blocks_inserts(pairs, 11, segs, sop)}
        if not inserts_only:
            routes["(a) align_pairs_blocks_inserts_seq"] = lambda: ctx.align_pairs_blocks_inserts_seq(pairs, 11, segs, sop)

            def second_pass():
                ctx.align_pairs_blocks_inserts(pairs, 11, segs, sop)
                ctx.align_set_pool(carrier)
                ctx.align_pairs_blocks(pairs, 11, segs, sop)
                ctx.align_set_pool(seqs)
            routes["(b) inserts, then blocks on a carrier (pool set twice)"] = second_pass
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
            print(f"  {k:<56} {statistics.median(v):9.3f} ({min(v):.3f} - {max(v):.3f})")
        if inserts_only:
            continue
        fused = routes["(a) align_pairs_blocks_inserts_seq"]
        w = fused()["insert_windows"]
        print("  windows:", [tuple(int(v) for v in x)[:7] for x in w["win"]][:4], "called bytes:", [len(s) for s in w["seq"]][:4])
        for split in (False, True):
            os.environ.pop("IOC_WIN_SPLIT", None)
            if split:
                os.environ["IOC_WIN_SPLIT"] = "1"
            dev = device_times(fused, calls)
            print(f"  device ms: median (min - max) over {calls} calls" + (", k_win_align as fill (k_win_align) and walk (k_win_align_walk)" if split else ""))
            for k, v in dev.items():
                print(f"  {k:<20} {statistics.median(v):8.3f} ({min(v):.3f} - {max(v):.3f})")
        os.environ.pop("IOC_WIN_SPLIT", None)
    ctx.close()
    return 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--inserts-only"]
    sys.exit(main(int(args[0]) if args else 7, "--inserts-only" in sys.argv[1:]))
