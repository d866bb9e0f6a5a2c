#!/usr/bin/env python3
"""What the isoforms' full-length sequences by variant cost (align_pairs_isoforms_full_variants) beside the two calls it joins, on the
batch of tools/align_isoforms_full_bench.py — 1200 reads of four isoforms against the 840-base representative, two sites of 600
voters, none of which splits — and on the batch of tools/align_insert_variants_bench.py that plants two exons at one junction.

    tools/align_isoforms_full_variants_bench.py [CALLS=7] [--existing-only]

Per batch, after two warm-up calls of each, CALLS rounds of the calls in turn; wall milliseconds per call of the Python wrapper as
median (min - max): align_pairs_blocks_inserts_seq, align_pairs_blocks_inserts_variants (the call this one extends),
align_pairs_isoforms_full and align_pairs_isoforms_full_variants.  --existing-only leaves the new call out: run from the root of a
checkout of the parent commit it gives the parent's figures for the calls that existed.  Then the device times from the IOC_TRACE
line of the full call and of the new one: k_ops_project_ins, k_group_pile over the isoforms, and the three splice launches —
k_splice_plan (its slot-aware instantiation in the new call), k_splice_call's count pass with the scan, its write pass.
profiles/iso_splice_variants.txt holds the tables."""
import re
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from isonclust2_amd import api  # noqa: E402
from align_insert_variants_bench import two_exons  # noqa: E402
from align_inserts_bench import short_representative  # noqa: E402
from align_split_bench import traced  # noqa: E402

KERNELS = ("k_ops_project_ins", "k_group_pile over the isoforms", "k_splice_plan", "k_splice_call<count> + scan", "k_splice_call<emit>")


def device_times(fn, calls):
    dev = {k: [] for k in KERNELS}
    for _ in range(calls):
        _, text = traced(fn)
        line = " ".join(ln.strip() for ln in text.splitlines() if "aligner: isoforms full" in ln)
        for k in KERNELS:
            dev[k].append(float(re.search(re.escape(k) + r" ([0-9.]+) ms", line).group(1)))
    return dev


def main(calls, existing_only):
    ctx = api.Context(0)
    for name, seqs, pairs, segs, sop, _ in (short_representative(), two_exons()):
        ctx.align_set_pool(seqs)
        routes = {"align_pairs_blocks_inserts_seq": lambda: ctx.align_pairs_blocks_inserts_seq(pairs, 11, segs, sop),
                  "align_pairs_blocks_inserts_variants": lambda: ctx.align_pairs_blocks_inserts_variants(pairs, 11, segs, sop),
                  "align_pairs_isoforms_full": lambda: ctx.align_pairs_isoforms_full(pairs, 11, segs, sop)}
        if not existing_only:
            routes["align_pairs_isoforms_full_variants"] = lambda: ctx.align_pairs_isoforms_full_variants(pairs, 11, segs, sop)
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
            print(f"  {k:<40} {statistics.median(v):9.3f} ({min(v):.3f} - {max(v):.3f})")
        for k in ("align_pairs_isoforms_full", "align_pairs_isoforms_full_variants"):
            if k not in routes:
                continue
            f = routes[k]()
            full = f["isoforms_full"]
            print(f"  {k}: isoforms", [[len(s) for s in g] for g in full["gseq"]][:4], "spliced bytes", [int(x) for x in full["sstats"]["spliced_bytes"]][:12],
                  "slot bytes uploaded", int(f["insert_variants"]["off"][-1]) if "insert_variants" in f else int(f["insert_windows"]["off"][-1]))
            print(f"  device ms of {k}: median (min - max) over {calls} calls")
            for kernel, v in device_times(routes[k], calls).items():
                print(f"    {kernel:<32} {statistics.median(v):8.3f} ({min(v):.3f} - {max(v):.3f})")
    ctx.close()
    return 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--existing-only"]
    sys.exit(main(int(args[0]) if args else 7, "--existing-only" in sys.argv[1:]))
