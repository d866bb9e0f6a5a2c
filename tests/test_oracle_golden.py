"""Pins the CPU oracle: (1) against every known-answer vector the reference's own unit tests hold
for the hot path (tests/golden/reference_kat.json <- test/isONclust2_test.cpp), (2) function by
function against the stand-alone reference TUs' stored answers (tests/golden/reference_tu.npz), and against
oracle/_ref (those TUs compiled where they lie) when that library was built.
CPU only.
"""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest

from oracle import pyoracle as po


def ulps(a, b):
    ia = struct.unpack("<q", struct.pack("<d", a))[0]
    ib = struct.unpack("<q", struct.pack("<d", b))[0]
    return abs(ia - ib)


def assert_double_eq(a, b):
    """gtest EXPECT_DOUBLE_EQ = within 4 ULPs."""
    assert ulps(a, b) <= 4, (a, b)


def test_sorting_kat(kat):
    g = kat["sorting"]
    rs = po.ReadSet([r["seq"].encode() for r in g["reads"]], [r["qual"].encode() for r in g["reads"]])
    rs.score_sort(g["k"], g["w"])
    order, score, err = rs.order()
    names = [g["reads"][i]["name"] for i in order]
    assert names == g["expected_order"]
    assert np.all(np.diff(score) <= 0)


def test_minimizer_kat(kat):
    g = kat["minimizer"]
    km = po.kmer_encode(g["seq"].encode(), g["k"])
    assert len(km) == len(g["seq"]) - g["k"]  # the final k-mer is never produced (kmer_index.cpp:12)
    mn, ps, ix = po.minimizers(km, g["k"], g["w"])
    exp = g["expected"]
    assert list(mn) == [e["min"] for e in exp]
    assert list(ps) == [e["pos"] for e in exp]
    assert list(ix) == [e["index"] for e in exp]
    for e in exp:
        assert po.lib().orc_kmer_to_index(e["kmer"].encode(), g["k"]) == e["min"]


def test_hpc_kat(kat):
    g = kat["hpc"]
    s, q = po.hpc(g["seq"].encode(), g["qual"].encode())
    assert s.decode() == g["expected_seq"]
    assert q.decode() == g["expected_qual"]


def test_error_rate_kat(kat):
    g = kat["error_rate"]
    r = po.error_rate(g["qual"].encode(), nomin=False)
    assert_double_eq(r, g["expected_double_eq"])
    assert r == float.fromhex("0x1.a36e2eb1c432fp-14") or ulps(r, 0.0001) <= 4


def test_emp_prob_lookup_kat(kat):
    g = kat["emp_prob_lookup"]
    tab, filled = po.pmin_table(g["k"], g["w"])
    assert filled == 225
    assert_double_eq(po.pmin_lookup(tab, g["e1"], g["e2"]), g["expected_double_eq"])


def test_min_match_kat(kat):
    g = kat["min_match"]
    ref, read = g["ref"].encode(), g["read"].encode()
    top, pe, mr = C.c_uint32(0), C.c_double(0), C.c_double(0)
    rc = po.lib().orc_minmatch(ref, g["qual_char"].encode() * len(ref), len(ref), read,
                               g["qual_char"].encode() * len(read), len(read), g["k"], g["w"],
                               po.PMIN_BIN.encode(), g["min_prob_no_hits"], C.byref(top), C.byref(pe),
                               C.byref(mr))
    assert rc == 0
    assert top.value == g["expected_top_size"]
    assert_double_eq(pe.value, g["expected_p_error_double_eq"])
    assert_double_eq(mr.value, g["expected_mapped_ratio_double_eq"])


def test_kmer_transform_kat(kat):
    k = kat["kmer_transform"]["k"]
    L = po.lib()
    kmers = []
    for i in range(4 ** k):
        b = C.create_string_buffer(k + 1)
        L.orc_index_to_kmer(i, k, b)
        kmers.append(b.raw[:k])
    assert kmers == sorted(kmers)
    assert [L.orc_kmer_to_index(s, k) for s in kmers] == list(range(4 ** k))


def test_gap_limit_matches_pow_predicate():
    """The integer gap limit is exactly the reference predicate pow(pError, n) >= p0
    (cluster.cpp:333-347) for every cell of the (11,16) table and every n up to 4096."""
    tab, _ = po.pmin_table(11, 15)
    for a in range(15):
        for b in range(15):
            lim = po.lib().orc_gap_limit(tab[a, b], 0.1)
            pe = 1.0 - tab[a, b]
            for n in list(range(0, 64)) + [100, 1000, 4096]:
                assert (math.pow(pe, float(n)) >= 0.1) == (n <= lim), (a, b, n, lim)


# ---- cross-checks against the stand-alone reference TUs (oracle/_ref) ---------------------------
# Their answers, inputs beside them, are stored in tests/golden/reference_tu.npz (tools/gen_golden_ref_tu.py): the oracle is
# checked against those everywhere, and where oracle/_ref was built the stored answers are checked against the live library.
REF_TU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_tu.npz")


@pytest.fixture(scope="module")
def ref_tu():
    with np.load(REF_TU) as d:
        return {k: d[k] for k in d.files}


def test_ref_kmer_encode_and_revcomp(ref_tu):
    g = ref_tu
    R = po.ref()
    seq, off, oo = g["kmer_seq"].tobytes(), g["kmer_seq_off"], g["kmer_out_off"]
    for t in range(len(g["kmer_k"])):
        s, k = seq[off[t]:off[t + 1]], int(g["kmer_k"][t])
        n = len(s)
        m, ref_out = int(g["kmer_m"][t]), g["kmer_out"][oo[t]:oo[t + 1]]
        rc, ref_rc = int(g["rc_rc"][t]), g["rc_out"][off[t]:off[t + 1]].tobytes()
        if R is not None:
            out = np.zeros(max(n, 1), np.uint32)
            assert R.ref_kmer_encode(s, n, k, out.ctypes.data_as(C.POINTER(C.c_uint32))) == m
            assert np.array_equal(out[:m], ref_out)
            o = C.create_string_buffer(n + 1)
            assert R.ref_revcomp(s, n, o) == rc
            assert rc != 0 or o.raw[:n] == ref_rc
        mine = po.kmer_encode(s, k)
        assert m == len(mine)
        assert np.array_equal(ref_out, mine)
        if rc == 0:
            assert po.revcomp(s) == ref_rc
        else:
            with pytest.raises(ValueError):
                po.revcomp(s)


def test_ref_round_and_pmin_all_cells(ref_tu):
    g = ref_tu
    R = po.ref()
    for x, y in zip(g["round_x"], g["round_y"]):
        if R is not None:
            assert R.ref_round(float(x), 2) == y
        assert y == po.lib().orc_round(float(x), 2)
    grid = g["pmin_e"]
    for i, (k, w) in enumerate(g["pmin_kw"].tolist()):
        size, look, errs = int(g["pmin_size"][i]), g["pmin_lookup"][i], g["pmin_err"][i]
        if R is not None:
            h = R.ref_pmin_init(k, w)
            assert R.ref_pmin_size(h) == size
            for a, e1 in enumerate(grid):
                for b, e2 in enumerate(grid):
                    err = C.c_int(0)
                    r = R.ref_pmin_lookup(h, float(e1), float(e2), C.byref(err))
                    assert err.value == errs[a, b]
                    assert err.value != 0 or r == look[a, b]
            R.ref_pmin_free(h)
        tab, filled = po.pmin_table(k, w)
        assert size == filled
        if filled:
            for a, e1 in enumerate(grid):
                for b, e2 in enumerate(grid):
                    assert errs[a, b] == 0
                    assert look[a, b] == po.pmin_lookup(tab, float(e1), float(e2))
        else:
            assert (errs == -1).all()
            with pytest.raises(KeyError):
                po.pmin_lookup(tab, 0.05, 0.05)


def test_minimizers_equal_argmin_change_formulation():
    """the reference's sliding rule == 'emit when the leftmost argmin of the window
    changes'.  This is the formulation the HIP kernel uses; pin it against the oracle on
    tie-heavy random input."""
    rng = np.random.default_rng(3)
    for trial in range(400):
        k = int(rng.integers(2, 14))
        w = k + int(rng.integers(0, 8))
        n = int(rng.integers(w - k + 1, 300))
        km = rng.integers(0, int(rng.integers(2, 50)), n).astype(np.uint32)
        mn, ps, ix = po.minimizers(km, k, w)
        W = w - k + 1
        exp = []
        prev = -1
        for j in range(n - W + 1):
            a = j + int(np.argmin(km[j:j + W]))
            if a != prev:
                exp.append((int(km[a]), a))
                prev = a
        assert [(int(a), int(b)) for a, b in zip(mn, ps)] == exp
        assert list(ix) == list(range(len(exp)))
