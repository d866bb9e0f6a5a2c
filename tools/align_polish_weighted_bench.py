#!/usr/bin/env python3
"""ioc_align_pairs_ops, ioc_align_pairs_polish and ioc_align_pairs_polish_weighted on one batch, timed in one process.

    tools/align_polish_weighted_bench.py [PAIRS=1622] [LENGTH=16700] [CALLS=7]

The batch is tools/align_polish_bench.py's (copies of one sequence at 10 % divergence, seed 1, every second pair against the
reverse complement: 32 references, each always taken in one frame) with one quality byte per base, drawn from 33 .. 126 (seed 2).
Wall clock of the C call alone (buffers allocated before), two warm-up calls of each form, then CALLS timed calls of each, the
forms in turn.  The last call of both polish forms runs under IOC_TRACE=1 with stderr caught: the device times of the pileup
variants and of the call kernels come from their own lines.  A last weighted call that asks for all three tables is checked
against the host definitions: the tables against ioc_host_ops_pileup / ioc_host_ops_pileup_weighted of the ops call's bytes, every
segment's sequence, qualities and record against ioc_host_pileup_call_weighted.  Exit status 1 unless every timed weighted call
lies below every timed ops call.  Writes profiles/align_polish_weighted.txt's table."""
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
MIN_DEPTH = 3
rng = random.Random(1)
base = bytes(rng.choice(b"ACGT") for _ in range(length))
COMP = bytes.maketrans(b"ACGT", b"TGCA")


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
first, segs, n_rows = {}, [], 0
for _, ri, rc, _ in pairs:  # one segment, one set of rows, per reference
    if ri not in first:
        first[ri] = (n_rows, rc, len(segs))
        segs.append((ri, rc))
        n_rows += len(seqs[ri]) + 1
    assert first[ri][1] == rc
row_base = np.array([first[p[1]][0] for p in pairs], np.int64)
seg_of_pair = np.array([first[p[1]][2] for p in pairs], np.int32)
ctx = api.Context(0)
ctx.align_set_pool(seqs)
qrng = np.random.default_rng(2)
quals = [qrng.integers(33, 127, len(s)).astype(np.uint8).tobytes() for s in seqs]
ctx.align_set_pool_qual(quals)
ctx.align_set_verdict_threshold(0.0)
L = _lib.load()
arr = ctx._aln_pairs(pairs)
sarr = (_lib.PolishSeg * len(segs))(*[_lib.PolishSeg(r, rc) for r, rc in segs])
bound = L.ioc_align_ops_bound(ctx.h, npairs, arr)
cap = sum(api.pileup_call_bound(len(seqs[r])) for r, _ in segs)
score, win, ratio = np.zeros(npairs, np.int32), np.zeros(npairs, np.int64), np.zeros(npairs, np.float64)
ops, off = np.zeros(bound, np.uint8), np.zeros(npairs + 1, np.int64)
pcols, wcols, wins = np.zeros(n_rows, api.PILEUP_DTYPE), np.zeros(n_rows, api.PILEUP_DTYPE), np.zeros(n_rows, api.PILEUP_INS_DTYPE)
out_seq, out_qual = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
out_off, pol = np.zeros(len(segs) + 1, np.int64), np.zeros(len(segs), api.POLISH_STATS_DTYPE)
p64 = C.POINTER(C.c_int64)
out3 = (score.ctypes.data_as(C.POINTER(C.c_int32)), win.ctypes.data_as(p64), ratio.ctypes.data_as(C.POINTER(C.c_double)))


def polish():
    return L.ioc_align_pairs_polish(ctx.h, npairs, arr, 11, 2, -2, 1, *out3, None, len(segs), sarr, seg_of_pair.ctypes.data_as(C.POINTER(C.c_int32)),
                                    MIN_DEPTH, out_seq.ctypes.data, out_qual.ctypes.data, cap, out_off.ctypes.data_as(p64), pol.ctypes.data, None, None)


def weighted(tables):
    return L.ioc_align_pairs_polish_weighted(ctx.h, npairs, arr, 11, 2, -2, 1, *out3, None, len(segs), sarr,
                                             seg_of_pair.ctypes.data_as(C.POINTER(C.c_int32)), MIN_DEPTH, out_seq.ctypes.data, out_qual.ctypes.data, cap,
                                             out_off.ctypes.data_as(p64), pol.ctypes.data, pcols.ctypes.data if tables else None,
                                             wcols.ctypes.data if tables else None, wins.ctypes.data if tables else None)


forms = {
    "ops": lambda: L.ioc_align_pairs_ops(ctx.h, npairs, arr, 11, 2, -2, 1, *out3, ops.ctypes.data, bound, off.ctypes.data_as(p64)),
    "polish": polish,
    "weighted": lambda: weighted(False),
}
wall = {f: [] for f in forms}
sums = {}
trace = {}
for rep in range(2 + calls):
    for f, call in forms.items():
        traced = f in ("polish", "weighted") and rep == 1 + calls
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
            trace[f] = tmp.read().decode(errors="replace")
            tmp.close()
        assert rc == 0, (f, rc)
        sums.setdefault(f, set()).add((int(score.sum()), int(win.sum())))
        if rep >= 2:  # (the traced call is timed too: the trace is a handful of lines)
            wall[f].append(dt)

assert len(set().union(*sums.values())) == 1, sums
lean = (out_seq.copy(), out_qual.copy(), out_off.copy(), pol.copy())
assert weighted(True) == 0
assert all(np.array_equal(a, b) for a, b in zip(lean, (out_seq, out_qual, out_off, pol))), "the call with the tables differs from the one without"
want_c, want_wc, want_wi = np.zeros(n_rows, api.PILEUP_DTYPE), np.zeros(n_rows, api.PILEUP_DTYPE), np.zeros(n_rows, api.PILEUP_INS_DTYPE)
for i, (qi, ri, _, _) in enumerate(pairs):  # the device's tables against the host's pileups of the emitting call's bytes
    rows = slice(row_base[i], row_base[i] + len(seqs[ri]) + 1)
    b = ops[off[i]:off[i + 1]].tobytes()
    api.ops_pileup(b, seqs[qi], len(seqs[ri]), cols=want_c[rows])
    api.ops_pileup_weighted(b, seqs[qi], quals[qi], len(seqs[ri]), wcols=want_wc[rows], wins=want_wi[rows])
assert np.array_equal(pcols, want_c) and np.array_equal(wcols, want_wc) and np.array_equal(wins, want_wi)
changed = 0
for g, (ri, rc) in enumerate(segs):  # every segment against the definition of the call
    frame = seqs[ri][::-1].translate(COMP) if rc else seqs[ri]
    rows = slice(first[ri][0], first[ri][0] + len(frame) + 1)
    seq, qual, st = api.pileup_call_weighted(want_c[rows], want_wc[rows], want_wi[rows], frame, MIN_DEPTH)
    assert out_seq[out_off[g]:out_off[g + 1]].tobytes() == seq and out_qual[out_off[g]:out_off[g + 1]].tobytes() == qual
    assert {k: int(pol[k][g]) for k in api.POLISH_STATS_FIELDS} == st
    changed += st["n_sub"] + st["n_del"] + st["n_ins"]


def trace_ms(text, what):
    line = next((ln for ln in text.splitlines() if what in ln), "")
    m = re.search(re.escape(what) + r" ([0-9.]+) ms", line)
    return line.strip(), float(m.group(1)) if m else float("nan")


pol_line, k_ins = trace_ms(trace["polish"], "k_ops_pileup<ins>")
_, k_call = trace_ms(trace["polish"], "k_pile_call")
w_line, k_w = trace_ms(trace["weighted"], "k_ops_pileup<weighted>")
_, k_wcall = trace_ms(trace["weighted"], "k_pile_call<weighted>")
events = int(sum(want_c[f].astype(np.int64).sum() for f in ("a", "c", "g", "t", "other", "del")))
print(f"{npairs} pairs of ~{length} bases, k 11, exact counts; {calls} timed calls of each form after 2 warm-up calls, the forms in turn")
print(f"operation bytes: bound {bound / 1e6:.1f} MB, {int(off[npairs]) / 1e6:.1f} MB written (what the ops call copies and packs); tables: {n_rows} rows, "
      f"{pcols.nbytes / 1e6:.1f} + {wins.nbytes / 1e6:.1f} MB on the device for polish, {pcols.nbytes / 1e6:.1f} + {wcols.nbytes / 1e6:.1f} + "
      f"{wins.nbytes / 1e6:.1f} MB for the weighted form, {len(segs)} segments; called bytes: {int(out_off[-1])} x 2 copied back (bound {cap}), "
      f"{changed} positions changed at min_depth {MIN_DEPTH}")
print(f"sums of scores / windows, every call of every form: {sums['ops']}; all three tables equal the host pileups of the ops call's bytes, every "
      "segment equals ioc_host_pileup_call_weighted of its rows")
print(f"{'form':<8} wall ms: median (min - max)")
for f in forms:
    w = wall[f]
    print(f"{f:<8} {statistics.median(w):8.2f} ({min(w):.2f} - {max(w):.2f})")
print("wall, every call: " + "; ".join(f"{f} " + " ".join(f"{x:.1f}" for x in wall[f]) for f in forms))
print(f"trace: {pol_line}")
print(f"trace: {w_line}")
print(f"k_ops_pileup<ins> {k_ins:.3f} ms, the weighted variant {k_w:.3f} ms ({events / 1e6:.2f} M more atomic words, one per base and 'D': {k_w - k_ins:+.3f} ms); "
      f"call kernels {k_call:.3f} ms, weighted {k_wcall:.3f} ms ({k_wcall - k_call:+.3f} ms) for {n_rows} rows")
print(f"weighted above polish: {statistics.median(wall['weighted']) - statistics.median(wall['polish']):+.2f} ms (medians)")
ok = max(wall["weighted"]) < min(wall["ops"])
print(f"every weighted call below every ops call: {'yes' if ok else 'NO'} (slowest weighted {max(wall['weighted']):.2f} ms, fastest ops {min(wall['ops']):.2f} ms)")
ctx.close()
sys.exit(0 if ok else 1)
