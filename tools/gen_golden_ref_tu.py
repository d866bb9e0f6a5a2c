#!/usr/bin/env python3
"""Regenerates tests/golden/reference_tu.npz: what the stand-alone reference TUs (oracle/_ref/libisonref.so, built by
oracle/Makefile where the reference tree is mounted) answer on the inputs of test_oracle_golden.py's cross-checks, inputs
stored beside the answers.  The tests compare the oracle with these answers on any machine, and with the live library
too where it was built.  Run in the build container:

    python tools/gen_golden_ref_tu.py

Arrays:
  kmer_k, kmer_seq, kmer_seq_off   per trial: k and the sequence (concatenated bytes, offsets)
  kmer_m, kmer_out, kmer_out_off   ref_kmer_encode: number of k-mers and their codes (concatenated, offsets)
  rc_rc, rc_out                    ref_revcomp: return code and the reverse complement (bytes at kmer_seq_off)
  round_x, round_y                 ref_round(x, 2)
  pmin_kw, pmin_size               (k, w) and ref_pmin_size
  pmin_e, pmin_lookup, pmin_err    ref_pmin_lookup on the pmin_e x pmin_e grid (NaN / err where the table is empty)
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from oracle import pyoracle as po  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "reference_tu.npz")
PMIN_KW = [(11, 15), (13, 20), (10, 12), (15, 19), (30, 32), (31, 40), (12, 200)]


def kmer_inputs():
    rng = np.random.default_rng(7)
    out = []
    for trial in range(300):
        n = int(rng.integers(0, 200))
        k = int(rng.integers(1, 20))
        alpha = b"ACGT" if trial % 5 else b"ACGTN"
        out.append((bytes(rng.choice(list(alpha), n).astype(np.uint8)), k))
    return out


def round_inputs():
    rng = np.random.default_rng(11)
    return np.array(list(rng.random(2000) * 0.3) + [0.005, 0.015, 0.025, 0.125, 0.145, 0.155, 0.0, 1.0], np.float64)


def main():
    R = po.ref()
    if R is None:
        sys.exit("oracle/_ref/libisonref.so is not built (oracle/Makefile builds it where the reference tree is mounted)")
    ks, seqs, ms, outs, rcs, rco = [], [], [], [], [], []
    for s, k in kmer_inputs():
        n = len(s)
        o = np.zeros(max(n, 1), np.uint32)
        m = R.ref_kmer_encode(s, n, k, o.ctypes.data_as(C.POINTER(C.c_uint32)))
        b = C.create_string_buffer(n + 1)
        rc = R.ref_revcomp(s, n, b)
        ks.append(k)
        seqs.append(s)
        ms.append(m)
        outs.append(o[:m])
        rcs.append(rc)
        rco.append(b.raw[:n])
    x = round_inputs()
    y = np.array([R.ref_round(float(v), 2) for v in x], np.float64)
    grid = np.linspace(0.0, 0.2, 41)
    sizes, looks, errs = [], [], []
    for k, w in PMIN_KW:
        h = R.ref_pmin_init(k, w)
        sizes.append(R.ref_pmin_size(h))
        lk = np.full((len(grid), len(grid)), np.nan)
        er = np.zeros((len(grid), len(grid)), np.int32)
        for i, e1 in enumerate(grid):
            for j, e2 in enumerate(grid):
                err = C.c_int(0)
                lk[i, j] = R.ref_pmin_lookup(h, float(e1), float(e2), C.byref(err))
                er[i, j] = err.value
        R.ref_pmin_free(h)
        looks.append(lk)
        errs.append(er)
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    ooff = np.zeros(len(outs) + 1, np.int64)
    ooff[1:] = np.cumsum([len(o) for o in outs])
    np.savez_compressed(
        PATH,
        kmer_k=np.array(ks, np.int32), kmer_seq=np.frombuffer(b"".join(seqs), np.uint8), kmer_seq_off=off,
        kmer_m=np.array(ms, np.int32), kmer_out=np.concatenate(outs).astype(np.uint32), kmer_out_off=ooff,
        rc_rc=np.array(rcs, np.int32), rc_out=np.frombuffer(b"".join(rco), np.uint8),
        round_x=x, round_y=y,
        pmin_kw=np.array(PMIN_KW, np.int32), pmin_size=np.array(sizes, np.int64),
        pmin_e=grid, pmin_lookup=np.stack(looks), pmin_err=np.stack(errs))
    print(f"wrote {PATH} ({os.path.getsize(PATH)} bytes)")


if __name__ == "__main__":
    main()
