#!/usr/bin/env python3
"""What the isoforms' full-length sequences cost (align_pairs_isoforms_full) beside the call it extends, on the batch of
tools/align_insert_windows_bench.py that has carriers: 1200 reads of four isoforms against the 840-base representative, two sites of
600 voters.

    tools/align_isoforms_full_bench.py [CALLS=7]

After two warm-up calls of each, CALLS rounds of the two calls in turn; wall milliseconds per call of the Python wrapper as median
(min - max): align_pairs_blocks_inserts_seq (the parent's call) and align_pairs_isoforms_full.  Then the device times from the
IOC_TRACE lines of the fused call: k_ops_project_ins (the six slot planes the call projects beside the others), k_group_pile over the
combined isoforms, and the three splice launches — k_splice_plan, k_splice_call's count pass with the scan, its write pass.
profiles/iso_splice.txt holds the tables."""
import re
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from isonclust2_amd import api  # noqa: E402
from align_inserts_bench import short_representative  # noqa: E402
from align_split_bench import traced  # noqa: E402

KERNELS = ("k_ops_project_ins", "k_group_pile over the isoforms", "k_splice_plan", "k_splice_call<count> + scan", "k_splice_call<emit>")


def main(calls):
    ctx = api.Context(0)
    name, seqs, pairs, segs, sop, _ = short_representative()
    ctx.align_set_pool(seqs)
    routes = {"align_pairs_blocks_inserts_seq": lambda: ctx.align_pairs_blocks_inserts_seq(pairs, 11, segs, sop),
              "align_pairs_isoforms_full": lambda: ctx.align_pairs_isoforms_full(pairs, 11, segs, sop),
              "align_pairs_isoforms_full, max_sites 4, max_win 200": lambda: ctx.align_pairs_isoforms_full(pairs, 11, segs, sop, max_sites=4, max_win=200)}
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
    full = routes["align_pairs_isoforms_full"]
    f = full()["isoforms_full"]
    print("  isoforms:", [len(s) for s in f["gseq"][0]], "bytes; spliced:", [[(int(r["state"]), int(r["at"]), int(r["len"])) for r in rec] for rec in f["splice"]])
    dev = {k: [] for k in KERNELS}
    for _ in range(calls):
        _, text = traced(full)
        line = " ".join(ln.strip() for ln in text.splitlines() if "aligner: isoforms full:" in ln)
        for k in KERNELS:
            dev[k].append(float(re.search(re.escape(k) + r" ([0-9.]+) ms", line).group(1)))
    print(f"  device ms: median (min - max) over {calls} calls")
    for k, v in dev.items():
        print(f"  {k:<32} {statistics.median(v):8.3f} ({min(v):.3f} - {max(v):.3f})")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 7))
