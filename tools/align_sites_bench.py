#!/usr/bin/env python3
"""The device times of ioc_align_pairs_alleles' own kernels beside k_ops_pileup of the same call, from the call's IOC_TRACE line, and
what the call copies back beside what ioc_align_pairs_ops copies for the same pairs.

    tools/align_sites_bench.py [CALLS=5]

Two shapes, those of tests/test_gpu_align_alleles.py: 300 reads at 10 % divergence on one 300-base segment (every wave of
k_ops_project and k_ops_pileup on the same rows: the contended case of the atomics), and 192 pairs of 3 kb on 12 segments.  Two
warm-up calls, then CALLS calls under IOC_TRACE=1 with stderr caught; per kernel the median and the range over the calls.  The
alleles of the last call are checked against the host definitions over the ops call's bytes.  Writes profiles/align_sites.txt's
tables."""
import os
import random
import re
import statistics
import sys
import tempfile

import numpy as np

sys.path.insert(0, ".")
from isonclust2_amd import api  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 5
COMP = bytes.maketrans(b"ACGT", b"TGCA")
KERNELS = ("k_ops_pileup", "k_ops_project", "k_pile_sites", "k_site_alleles")


def mutate(rng, s, rate):
    out = bytearray()
    for ch in s:
        x = rng.random()
        if x < rate / 3:
            out.append(rng.choice(b"ACGT"))
        elif x < 2 * rate / 3:
            continue
        elif x < rate:
            out += bytes([ch, rng.choice(b"ACGT")])
        else:
            out.append(ch)
    return bytes(out)


def many_reads():
    rng = random.Random(17)
    ref = bytes(rng.choice(b"ACGT") for _ in range(300))
    seqs = [ref] + [mutate(rng, ref, 0.1) for _ in range(300)]
    return "300 reads on one 300-base segment", seqs, [(1 + i, 0, 0, 0.2) for i in range(300)], [(0, 0)], [0] * 300, dict(min_depth=3, min_alt=3, min_pct=2)


def sliced():
    rng = random.Random(23)
    base = bytes(rng.choice(b"ACGT") for _ in range(3000))
    seqs = [mutate(rng, base, 0.1) for _ in range(12)]
    pairs = [(i, (i + 1) % 12, i % 2, 0.2) for i in range(12)] * 8 + [((i + 5) % 12, (i + 1) % 12, i % 2, 0.2) for i in range(12)] * 8
    segs = [((i + 1) % 12, i % 2) for i in range(12)]
    return "192 pairs of 3 kb on 12 segments", seqs, pairs, segs, [segs.index((p[1], p[2])) for p in pairs], dict(min_depth=3, min_alt=3, min_pct=25)


def traced(fn):
    """fn() with the library's trace (the C stderr, file descriptor 2) caught: (result, text)."""
    os.environ["IOC_TRACE"] = "1"
    sys.stderr.flush()
    keep, tmp = os.dup(2), tempfile.TemporaryFile()
    os.dup2(tmp.fileno(), 2)
    try:
        out = fn()
    finally:
        os.dup2(keep, 2)
        os.close(keep)
        os.environ.pop("IOC_TRACE", None)
    tmp.seek(0)
    text = tmp.read().decode(errors="replace")
    tmp.close()
    return out, text


ctx = api.Context(0)
ok = True
for name, seqs, pairs, segs, sop, rule in (many_reads(), sliced()):
    ctx.align_set_pool(seqs)
    for _ in range(2):
        ctx.align_pairs_alleles(pairs, 11, segs, sop, **rule)
    ms = {k: [] for k in KERNELS}
    line = ""
    for _ in range(calls):
        got, text = traced(lambda: ctx.align_pairs_alleles(pairs, 11, segs, sop, **rule))
        line = next(ln for ln in text.splitlines() if "aligner: sites:" in ln).strip()
        for k in KERNELS:
            ms[k].append(float(re.search(re.escape(k) + r" ([0-9.]+) ms", line).group(1)))
    (_, _, _, ops), ops_text = traced(lambda: ctx.align_pairs_ops(pairs, 11))
    ops_line = next(ln for ln in ops_text.splitlines() if "operation bytes:" in ln).strip()
    for i, (pr, b, g) in enumerate(zip(pairs, ops, sop)):
        base, insf = api.ops_project(b, seqs[pr[0]], len(seqs[pr[1]]))
        ok = ok and np.array_equal(got["alleles"][i], api.site_alleles(base, insf, got["sites"][g]))
    kept = sum(len(s) for s in got["sites"])
    back = kept * 32 + sum(len(a) for a in got["alleles"]) + 8 * (2 * len(segs) + 1)
    print(f"{name}: {len(pairs)} pairs, {sum(len(b) for b in ops)} operation bytes; {kept} sites kept, {sum(len(a) for a in got['alleles'])} allele bytes; "
          f"sites + alleles + offsets copied back: {back} bytes")
    print(f"  {'kernel':<15} device ms: median (min - max) over {calls} calls")
    for k in KERNELS:
        print(f"  {k:<15} {statistics.median(ms[k]):8.3f} ({min(ms[k]):.3f} - {max(ms[k]):.3f})")
    print(f"  trace: {line}")
    print(f"  trace: {ops_line}")
    print(f"  alleles equal ioc_host_site_alleles of ioc_host_ops_project of the ops call's bytes: {'yes' if ok else 'NO'}")
ctx.close()
sys.exit(0 if ok else 1)
