"""ioc_host_ops_pileup — the definition of the per-position pileup (the device's k_ops_pileup is tested against it in
tests/test_gpu_align_pileup.py) — against a plain-Python restatement: hand-written strings for every rule of the definition, every
string the host aligner returns for the small random pairs of test_gpu_align_ops, the identities that tie a table to
ioc_host_ops_stats of the same string, and the three refusals.  Integers only, no tolerance."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests.align_ops_checks import revcomp
from tests.test_align_stats_host import HAND
from tests.test_gpu_align_ops import _small_pairs

FIELDS = ("a", "c", "g", "t", "other", "del", "ins_runs", "ins_bases")
BASES = ("a", "c", "g", "t", "other")


def lengths(ops):
    """(query bases, reference bases) an operation string consumes."""
    ops = bytes(ops)
    return sum(ops.count(b) for b in b"=XIi"), sum(ops.count(b) for b in b"=XDd")


def py_pileup(ops, query, rlen):
    """The walk of the definition, byte by byte."""
    cols = np.zeros(rlen + 1, api.PILEUP_DTYPE)
    r = q = 0
    ops = bytes(ops)
    for x, op in enumerate(ops):
        op = chr(op)
        if op == "d":
            r += 1
        elif op == "i":
            q += 1
        elif op in "=X":
            cols[{"A": "a", "C": "c", "G": "g", "T": "t"}.get(chr(query[q]), "other")][r] += 1
            r, q = r + 1, q + 1
        elif op == "D":
            cols["del"][r] += 1
            r += 1
        else:
            assert op == "I"
            cols["ins_bases"][r] += 1
            if x == 0 or ops[x - 1] != ord("I"):
                cols["ins_runs"][r] += 1
            q += 1
    assert (q, r) == (len(query), rlen)
    return cols


def _query(rng, n, letters=b"ACGT"):
    return bytes(rng.choice(letters) for _ in range(n))


MORE = [
    b"II==", b"I=", b"iII=X=",                       # 'I' before the first reference base
    b"=IID=", b"=DII=", b"=IDI=", b"=DID=",          # 'I' directly before and after 'D'
    b"==III", b"==IIIii", b"dd=II", b"III",          # a run of 'I' at row R
    b"=" * 70 + b"I" * 130 + b"D" * 3 + b"I" + b"=",
]


@pytest.mark.parametrize("ops", HAND + MORE, ids=lambda o: api.ops_to_cigar(o) or "empty")
def test_hand_written_strings(ops):
    rng = random.Random(len(ops))
    nq, nr = lengths(ops)
    for letters in (b"ACGT", b"ACGTNacgtRY-"):     # (letters other than ACGT: lower case is `other` too)
        q = _query(rng, nq, letters)
        got = api.ops_pileup(ops, q, nr)
        assert got.dtype == api.PILEUP_DTYPE and got.shape == (nr + 1,)
        assert np.array_equal(got, py_pileup(ops, q, nr)), (ops, q)
        check_identities(got, ops, nr)


def check_identities(cols, ops, rlen):
    """What ties a string's table to ioc_host_ops_stats of the same string."""
    st = api.ops_stats(ops)
    assert sum(int(cols[f].sum()) for f in BASES) == st["matches"] + st["mismatches"]
    assert int(cols["del"].sum()) == st["del"] and int(cols["ins_bases"].sum()) == st["ins"] and int(cols["ins_runs"].sum()) == st["ins_runs"]
    if st["columns"] == 0:
        return  # (no walk: the end gaps are all "leading", and the table is all zero anyway)
    depth = sum(cols[f].astype(np.int64) for f in BASES + ("del",))
    assert not depth[:st["lead_d"]].any() and not depth[rlen - st["trail_d"]:].any()
    assert not any(cols[f][rlen] for f in BASES + ("del",))  # row R can only ever hold insertion counts


def test_hand_written_values():
    """A few tables spelled out, so that the restatement above is not the only witness."""
    z = (0,) * 8
    def rows(c):
        return [tuple(int(v) for v in r) for r in c]
    assert api.PILEUP_DTYPE.names == FIELDS and api.PILEUP_DTYPE.itemsize == 32 and C.sizeof(_lib.PileupCol) == 32
    assert rows(api.ops_pileup(b"", b"", 0)) == [z]
    assert rows(api.ops_pileup(b"dd", b"", 2)) == [z, z, z]
    #                                                  a  c  g  t  o  D  Ir Ib
    assert rows(api.ops_pileup(b"=X=", b"ACN", 3)) == [(1, 0, 0, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 1, 0, 0, 0), z]
    assert rows(api.ops_pileup(b"II=D=III", b"GGTAGGG", 3)) == [(0, 0, 0, 1, 0, 0, 1, 2), (0, 0, 0, 0, 0, 1, 0, 0), (1, 0, 0, 0, 0, 0, 0, 0),
                                                                (0, 0, 0, 0, 0, 0, 1, 3)]
    assert rows(api.ops_pileup(b"d=IDI=i", b"CAAGT", 4)) == [z, (0, 1, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 1, 1, 1), (0, 0, 1, 0, 0, 0, 1, 1), z]


def test_host_aligner_output():
    """Every string ioc_host_align_ops returns for the small random pairs (lengths 0 .. 200, every gap-open class, half of them
    against the reverse complement)."""
    L = _lib.load()
    seqs, pairs = _small_pairs(13)
    seen_ins = seen_del = 0
    for qi, ri, rc, e in pairs:
        q, r = seqs[qi], revcomp(seqs[ri]) if rc else seqs[ri]
        ops, _ = api.host_align_ops(q, r, gap_open=L.ioc_host_gap_open(e))
        got = api.ops_pileup(ops, q, len(r))
        assert np.array_equal(got, py_pileup(ops, q, len(r))), (qi, ri, rc, e)
        check_identities(got, ops, len(r))
        seen_ins += int(got["ins_runs"].sum())
        seen_del += int(got["del"].sum())
    assert seen_ins > 20 and seen_del > 20


@pytest.mark.parametrize("case", ["byte", "query_short", "query_long", "ref_short", "ref_long", "len_2_31"])
def test_refusals_leave_the_table_untouched_and_calls_add_up(case):
    L = _lib.load()
    ops, q, nr = b"i=X=ID=d", b"TACGAC", 6
    assert lengths(ops) == (len(q), nr)
    cols = api.ops_pileup(ops, q, nr)
    once = cols.copy()
    args = {"byte": (b"i=X=QD=d", len(ops), q, len(q), nr), "query_short": (ops, len(ops), q, len(q) - 1, nr),
            "query_long": (ops, len(ops), q + b"A", len(q) + 1, nr), "ref_short": (ops, len(ops), q, len(q), nr - 1),
            "ref_long": (ops, len(ops), q, len(q), nr + 1), "len_2_31": (ops, 1 << 31, q, len(q), nr)}[case]
    room = np.zeros(nr + 2, api.PILEUP_DTYPE)  # (one row more than any of the cases may touch)
    room[:nr + 1] = cols
    before = room.copy()
    assert L.ioc_host_ops_pileup(*args, room.ctypes.data) == -1  # IOC_ERR_ARG
    assert np.array_equal(room, before)
    if case in ("byte", "ref_long"):
        with pytest.raises(ValueError):
            api.ops_pileup(args[0], args[2], args[4])
    # a second call adds onto the first
    assert api.ops_pileup(ops, q, nr, cols=cols) is cols
    for f in FIELDS:
        assert np.array_equal(cols[f], 2 * once[f])
    with pytest.raises(ValueError):
        api.ops_pileup(ops, q, nr, cols=np.zeros(nr, api.PILEUP_DTYPE))  # a table of the wrong length
