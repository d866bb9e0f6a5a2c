#!/usr/bin/env python3
"""The four forms of the batched GPU aligner on one batch, timed in one process: ioc_align_pairs (exact: no verdict threshold),
ioc_align_pairs_ops, ioc_align_pairs_stats and ioc_align_pairs_pileup with the pairs piled by reference.

    tools/align_pileup_bench.py [PAIRS=1622] [LENGTH=16700] [CALLS=7]

The batch is tools/align_stats_bench.py's (copies of one sequence at 10 % divergence, seed 1, every second pair against the
reverse complement: 32 references, each always taken in one frame).  Wall clock of the C call alone (buffers allocated before),
two warm-up calls of each form, then CALLS timed calls of each, the forms in turn.  The last pileup call runs under IOC_TRACE=1 with
stderr caught: k_ops_pileup's device time comes from its own line.  The table is checked against ioc_host_ops_pileup of the ops
call's bytes.  Exit status 1 unless every timed pileup call lies below every timed ops call.  Writes profiles/align_pileup.txt's
table."""
import ctypes as C
import os
import random
import re
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, ".")
from isonclust2_amd import _lib, api  # noqa: E402

npairs = int(sys.argv[1]) if len(sys.argv) > 1 else 1622
length = int(sys.argv[2]) if len(sys.argv) > 2 else 16700
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 7
rng = random.Random(1)
base = bytes(rng.choice(b"ACGT") for _ in range(length))


def mutate(s, rate=0.1):
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


seqs = [mutate(base) for _ in range(min(npairs, 32) + 1)]
pairs = [(i % (len(seqs) - 1), i % (len(seqs) - 1) + 1, i % 2, 0.2) for i in range(npairs)]
first, n_rows = {}, 0
for _, ri, rc, _ in pairs:  # one set of rows per reference
    if ri not in first:
        first[ri] = (n_rows, rc)
        n_rows += len(seqs[ri]) + 1
    assert first[ri][1] == rc
row_base = np.array([first[p[1]][0] for p in pairs], np.int64)
ctx = api.Context(0)
ctx.align_set_pool(seqs)
ctx.align_set_verdict_threshold(0.0)
L = _lib.load()
arr = ctx._aln_pairs(pairs)
bound = L.ioc_align_ops_bound(ctx.h, npairs, arr)
score, win, ratio = np.zeros(npairs, np.int32), np.zeros(npairs, np.int64), np.zeros(npairs, np.float64)
ops, off = np.zeros(bound, np.uint8), np.zeros(npairs + 1, np.int64)
stats = np.zeros(npairs, api.ALN_STATS_DTYPE)
cols = np.zeros(n_rows, api.PILEUP_DTYPE)
out3 = (score.ctypes.data_as(C.POINTER(C.c_int32)), win.ctypes.data_as(C.POINTER(C.c_int64)), ratio.ctypes.data_as(C.POINTER(C.c_double)))
forms = {
    "plain": lambda: L.ioc_align_pairs(ctx.h, npairs, arr, 11, 2, -2, 1, *out3),
    "ops": lambda: L.ioc_align_pairs_ops(ctx.h, npairs, arr, 11, 2, -2, 1, *out3, ops.ctypes.data, bound, off.ctypes.data_as(C.POINTER(C.c_int64))),
    "stats": lambda: L.ioc_align_pairs_stats(ctx.h, npairs, arr, 11, 2, -2, 1, *out3, stats.ctypes.data),
    "pileup": lambda: L.ioc_align_pairs_pileup(ctx.h, npairs, arr, 11, 2, -2, 1, *out3, None, row_base.ctypes.data_as(C.POINTER(C.c_int64)), n_rows,
                                               cols.ctypes.data),
}
wall = {f: [] for f in forms}
sums = {}
trace_text = ""
for rep in range(2 + calls):
    for f, call in forms.items():
        traced = f == "pileup" and rep == 1 + calls
        if traced:  # (the library writes its trace to the C stderr: file descriptor 2 goes to a file for this one call)
            os.environ["IOC_TRACE"] = "1"
            sys.stderr.flush()
            keep, tmp = os.dup(2), tempfile.TemporaryFile()
            os.dup2(tmp.fileno(), 2)
        t = time.perf_counter()
        rc = call()
        dt = (time.perf_counter() - t) * 1e3
        if traced:
            os.dup2(keep, 2)
            os.close(keep)
            os.environ.pop("IOC_TRACE", None)
            tmp.seek(0)
            trace_text = tmp.read().decode(errors="replace")
            tmp.close()
        assert rc == 0, (f, rc)
        sums.setdefault(f, set()).add((int(score.sum()), int(win.sum())))
        if rep >= 2:  # (the traced call is timed too: the trace is a handful of lines)
            wall[f].append(dt)

assert len(set().union(*sums.values())) == 1, sums
want = np.zeros(n_rows, api.PILEUP_DTYPE)
for i, (qi, ri, _, _) in enumerate(pairs):  # the device's table against the host's pileup of the emitting call's bytes
    api.ops_pileup(ops[off[i]:off[i + 1]].tobytes(), seqs[qi], len(seqs[ri]), cols=want[row_base[i]:row_base[i] + len(seqs[ri]) + 1])
assert np.array_equal(cols, want)
line = next((ln for ln in trace_text.splitlines() if "k_ops_pileup" in ln), "")
m = re.search(r"k_ops_pileup ([0-9.]+) ms", line)
k_ms = float(m.group(1)) if m else float("nan")
# one atomic word per '=' / 'X' / 'D' byte, one per piece of an 'I' run and one per run (pieces >= runs: a lower bound)
words = sum(int(cols[f].astype(np.int64).sum()) for f in ("a", "c", "g", "t", "other", "del")) + 2 * int(cols["ins_runs"].astype(np.int64).sum())
print(f"{npairs} pairs of ~{length} bases, k 11, exact counts; {calls} timed calls of each form after 2 warm-up calls, the forms in turn")
print(f"operation bytes: bound {bound / 1e6:.1f} MB, {int(off[npairs]) / 1e6:.1f} MB written (what the ops call copies and packs); "
      f"records: {stats.nbytes / 1e3:.1f} KB; pileup table: {n_rows} rows, {cols.nbytes / 1e6:.1f} MB, {len(first)} references")
print(f"sums of scores / windows, every call of every form: {sums['plain']}; the table equals ioc_host_ops_pileup of the ops call's bytes")
print(f"{'form':<7} wall ms: median (min - max)")
for f in forms:
    w = wall[f]
    print(f"{f:<7} {statistics.median(w):8.2f} ({min(w):.2f} - {max(w):.2f})")
print("wall, every call: " + "; ".join(f"{f} " + " ".join(f"{x:.1f}" for x in wall[f]) for f in forms))
print(f"trace: {line.strip()}")
print(f"k_ops_pileup: {k_ms:.3f} ms on the device for >= {words / 1e6:.2f} M atomic words = {words * 4 / 1e6:.1f} MB: {words * 4 / (k_ms * 1e-3) / 1e9:.1f} GB/s of added bytes")
print(f"pileup above stats: {statistics.median(wall['pileup']) - statistics.median(wall['stats']):+.2f} ms (medians)")
ok = max(wall["pileup"]) < min(wall["ops"])
print(f"every pileup call below every ops call: {'yes' if ok else 'NO'} (slowest pileup {max(wall['pileup']):.2f} ms, fastest ops {min(wall['ops']):.2f} ms)")
ctx.close()
sys.exit(0 if ok else 1)
