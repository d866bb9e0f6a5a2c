#!/usr/bin/env python3
"""What the split by linked sites costs: the device times of its kernels beside k_site_alleles of the same call, from the call's
IOC_TRACE lines; the wall time of the fused call; and one large synthetic segment through ioc_alleles_split.

    tools/align_split_bench.py kernels [CALLS=5]     the batches of tools/align_sites_bench.py through align_pairs_split, and one
                                                     segment of 3000 reads x 4096 sites through alleles_split: per kernel the
                                                     median and the range over CALLS calls, and the bytes uploaded
    tools/align_split_bench.py wall split|alleles [CALLS=7]
                                                     the same batches: wall milliseconds per call of align_pairs_split or of
                                                     align_pairs_alleles, after two warm-up calls

The package is imported from the current directory, so that `wall alleles` can be run in a checkout of the parent commit and
`wall split` in this one, in turn.  profiles/align_split.txt holds the tables."""
import os
import random
import re
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, ".")
from isonclust2_amd import api  # noqa: E402

COMP = bytes.maketrans(b"ACGT", b"TGCA")
SPLIT_KERNELS = ("k_site_marks", "k_allele_bits", "k_site_link", "k_split_seed", "k_split_phase0", "k_split_vote", "k_group_bits", "k_split_rephase", "k_split_record")
SPLIT = dict(min_link=3, min_margin=1, rounds=2)


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


def table(ms, names, calls):
    print(f"  {'kernel':<16} device ms: median (min - max) over {calls} calls")
    for k in names:
        print(f"  {k:<16} {statistics.median(ms[k]):8.3f} ({min(ms[k]):.3f} - {max(ms[k]):.3f})")


def kernels(calls):
    ctx = api.Context(0)
    ok = True
    for name, seqs, pairs, segs, sop, rule in (many_reads(), sliced()):
        ctx.align_set_pool(seqs)
        for _ in range(2):
            ctx.align_pairs_split(pairs, 11, segs, sop, **rule, **SPLIT)
        names = ("k_site_alleles",) + SPLIT_KERNELS
        ms = {k: [] for k in names}
        for _ in range(calls):
            got, text = traced(lambda: ctx.align_pairs_split(pairs, 11, segs, sop, alleles=True, **rule, **SPLIT))
            sites_line = next(ln for ln in text.splitlines() if "aligner: sites:" in ln).strip()
            split_line = next(ln for ln in text.splitlines() if "aligner: split:" in ln).strip()
            for k in names:
                ms[k].append(float(re.search(re.escape(k) + r" ([0-9.]+) ms", sites_line + " " + split_line).group(1)))
        for g in range(len(segs)):   # the last call against the definition
            mem = got["members"][g]
            a = np.array([got["alleles"][i] for i in mem], np.uint8).reshape(len(mem), len(got["sites"][g]))
            host = api.alleles_split(got["sites"][g], a, **SPLIT)
            ok = ok and np.array_equal(got["group"][mem], host["group"]) and got["seg"][g].tobytes() == host["seg"].tobytes()
        print(f"{name}: {len(pairs)} pairs, {sum(len(s) for s in got['sites'])} sites kept, {sum(len(a) for a in got['alleles'])} allele bytes; "
              f"{int((got['seg']['seed'] >= 0).sum())} of {len(segs)} segments split; rule {SPLIT}")
        table(ms, names, calls)
        print(f"  trace: {split_line}")
        print(f"  groups and records equal ioc_host_alleles_split of the call's sites and alleles: {'yes' if ok else 'NO'}")
    # one synthetic segment: 3000 reads x 4096 sites, two planted groups, 20 % of the bytes uncovered, 10 % noise
    rng = np.random.default_rng(1)
    nr, ns = 3000, 4096
    major = rng.integers(0, 6, ns)
    minor = (major + 1 + rng.integers(0, 5, ns)) % 6
    side = rng.integers(0, 2, nr).astype(bool)
    a = np.where(side[:, None], minor[None, :], major[None, :]).astype(np.uint8)
    a[rng.random((nr, ns)) < 0.2] = 7
    noisy = rng.random((nr, ns)) < 0.1
    a[noisy] = rng.integers(0, 6, int(noisy.sum())).astype(np.uint8)
    sites = np.zeros(ns, api.PILE_SITE_DTYPE)
    sites["minor"], sites["major"], sites["row"] = minor, major, np.arange(ns)
    rows = list(a)
    for _ in range(2):
        ctx.alleles_split([sites], rows, [0] * nr, **SPLIT)
    ms = {k: [] for k in SPLIT_KERNELS}
    for _ in range(calls):
        got, text = traced(lambda: ctx.alleles_split([sites], rows, [0] * nr, **SPLIT))
        line = next(ln for ln in text.splitlines() if "[ioc]   split:" in ln).strip()
        for k in SPLIT_KERNELS:
            ms[k].append(float(re.search(re.escape(k) + r" ([0-9.]+) ms", line).group(1)))
    group = got["group"]
    agree = max(int((group == side).sum()), int((group == 1 - side.astype(np.uint8)).sum()))
    ok = ok and agree == nr
    print(f"one synthetic segment of {nr} reads x {ns} sites through ioc_alleles_split ({ns * (ns - 1) * ((nr + 63) // 64) * 4 / 1e9:.2f}e9 popcount-ands in "
          f"k_site_link); rule {SPLIT}")
    table(ms, SPLIT_KERNELS, calls)
    print(f"  trace: {line}")
    print(f"  reads on their planted side: {agree} of {nr}; record {got['seg'][0]}")
    ctx.close()
    return ok


def wall(which, calls):
    ctx = api.Context(0)
    for name, seqs, pairs, segs, sop, rule in (many_reads(), sliced()):
        ctx.align_set_pool(seqs)
        fn = (lambda: ctx.align_pairs_split(pairs, 11, segs, sop, **rule, **SPLIT)) if which == "split" else \
             (lambda: ctx.align_pairs_alleles(pairs, 11, segs, sop, **rule))
        for _ in range(2):
            fn()
        ms = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        print(f"wall {which:<8} {name}: median {statistics.median(ms):.3f} ms ({min(ms):.3f} - {max(ms):.3f}) over {calls} calls: "
              + " ".join(f"{x:.3f}" for x in ms))
    ctx.close()
    return True


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    if mode == "kernels":
        done = kernels(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    elif mode == "wall" and len(sys.argv) > 2 and sys.argv[2] in ("split", "alleles"):
        done = wall(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 7)
    else:
        sys.exit(__doc__)
    sys.exit(0 if done else 1)
