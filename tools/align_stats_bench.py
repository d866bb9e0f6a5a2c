#!/usr/bin/env python3
"""The three forms of the batched GPU aligner on one batch, timed in one process: ioc_align_pairs (exact: no verdict threshold),
ioc_align_pairs_ops and ioc_align_pairs_stats.

    tools/align_stats_bench.py [PAIRS=1622] [LENGTH=16700] [CALLS=7]

The batch is tools/align_bench.py's (copies of one sequence at 10 % divergence, seed 1, every second pair against the reverse
complement).  Wall clock of the C call alone (buffers allocated before), two warm-up calls of each form, then CALLS timed calls of
each, the three forms in turn; ms_align_fwd / ms_align_trace of ioc_timings beside it.  The last statistics call runs under
IOC_TRACE=1: its own line (records copied, k_ops_stats' device time) goes to stderr.  Writes profiles/align_stats.txt's table."""
import ctypes as C
import os
import random
import statistics
import sys
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
ctx = api.Context(0)
ctx.align_set_pool(seqs)
ctx.align_set_verdict_threshold(0.0)
L = _lib.load()
arr = ctx._aln_pairs(pairs)
bound = L.ioc_align_ops_bound(ctx.h, npairs, arr)
score, win, ratio = np.zeros(npairs, np.int32), np.zeros(npairs, np.int64), np.zeros(npairs, np.float64)
ops, off = np.zeros(bound, np.uint8), np.zeros(npairs + 1, np.int64)
stats = np.zeros(npairs, api.ALN_STATS_DTYPE)
out3 = (score.ctypes.data_as(C.POINTER(C.c_int32)), win.ctypes.data_as(C.POINTER(C.c_int64)), ratio.ctypes.data_as(C.POINTER(C.c_double)))
forms = {
    "plain": lambda: L.ioc_align_pairs(ctx.h, npairs, arr, 11, 2, -2, 1, *out3),
    "ops": lambda: L.ioc_align_pairs_ops(ctx.h, npairs, arr, 11, 2, -2, 1, *out3, ops.ctypes.data, bound, off.ctypes.data_as(C.POINTER(C.c_int64))),
    "stats": lambda: L.ioc_align_pairs_stats(ctx.h, npairs, arr, 11, 2, -2, 1, *out3, stats.ctypes.data),
}
wall = {f: [] for f in forms}
fwd = {f: [] for f in forms}
trace = {f: [] for f in forms}
sums = {}
for rep in range(2 + calls):
    for f, call in forms.items():
        if f == "stats" and rep == 1 + calls:
            os.environ["IOC_TRACE"] = "1"
        t0 = ctx.timings()
        t = time.perf_counter()
        rc = call()
        dt = (time.perf_counter() - t) * 1e3
        os.environ.pop("IOC_TRACE", None)
        assert rc == 0, (f, rc, ctx.last_error() if hasattr(ctx, "last_error") else "")
        t1 = ctx.timings()
        sums.setdefault(f, set()).add((int(score.sum()), int(win.sum())))
        if rep >= 2:
            wall[f].append(dt)
            fwd[f].append(t1["ms_align_fwd"] - t0["ms_align_fwd"])
            trace[f].append(t1["ms_align_trace"] - t0["ms_align_trace"])

assert len(set().union(*sums.values())) == 1, sums
for i in range(npairs):  # the device's records against the host's count of the emitting call's bytes
    want = api.ops_stats(ops[off[i]:off[i + 1]].tobytes())
    assert all(int(stats[k][i]) == v for k, v in want.items()), i
print(f"{npairs} pairs of ~{length} bases, k 11, exact counts; {calls} timed calls of each form after 2 warm-up calls, the forms in turn")
print(f"operation bytes: bound {bound / 1e6:.1f} MB (what k_ops_stats' slice buffer holds), {int(off[npairs]) / 1e6:.1f} MB written (what it reads); "
      f"records: {stats.nbytes / 1e3:.1f} KB")
print(f"sums of scores / windows, every call of every form: {sums['plain']}; every record equals ioc_host_ops_stats of the ops call's bytes")
print(f"{'form':<6} {'wall ms: median (min - max)':<32} {'forward ms: median':<20} {'traceback ms: median (min - max)'}")
for f in forms:
    w, a, b = wall[f], fwd[f], trace[f]
    print(f"{f:<6} {statistics.median(w):8.2f} ({min(w):.2f} - {max(w):.2f})          {statistics.median(a):8.2f}             "
          f"{statistics.median(b):8.3f} ({min(b):.3f} - {max(b):.3f})")
print("wall, every call: " + "; ".join(f"{f} " + " ".join(f"{x:.1f}" for x in wall[f]) for f in forms))
ctx.close()
