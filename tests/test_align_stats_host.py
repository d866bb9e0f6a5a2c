"""ioc_host_ops_stats — the definition of the alignment statistics (the device's k_ops_stats is tested against it in
tests/test_gpu_align_stats.py) — against a plain-Python restatement with regular expressions: hand-written strings for every
rule of the definition, and every string the host aligner returns for the small random pairs of test_gpu_align_ops.  Integers
only, no tolerance."""
import ctypes as C
import re

import pytest

from isonclust2_amd import _lib, api
from tests.align_ops_checks import revcomp
from tests.test_gpu_align_ops import _small_pairs

FIELDS = ("length", "columns", "matches", "mismatches", "ins", "del", "ins_runs", "del_runs", "longest_ins", "longest_del",
          "lead_i", "lead_d", "trail_i", "trail_d")


def py_stats(ops):
    """The definition once more: the walk is the part from the first to the last byte of "=XID"; what lies before it is leading,
    what lies behind it trailing, a string without a walk byte is all leading; a run is maximal over one byte value."""
    ops = bytes(ops)
    walk = [m.start() for m in re.finditer(rb"[=XID]", ops)]
    lead, trail = (ops[:walk[0]], ops[walk[-1] + 1:]) if walk else (ops, b"")
    runs_i = [len(m.group()) for m in re.finditer(rb"I+", ops)]
    runs_d = [len(m.group()) for m in re.finditer(rb"D+", ops)]
    return {"length": len(ops), "columns": len(walk), "matches": ops.count(b"="), "mismatches": ops.count(b"X"),
            "ins": sum(runs_i), "del": sum(runs_d), "ins_runs": len(runs_i), "del_runs": len(runs_d),
            "longest_ins": max(runs_i, default=0), "longest_del": max(runs_d, default=0),
            "lead_i": lead.count(b"i"), "lead_d": lead.count(b"d"), "trail_i": trail.count(b"i"), "trail_d": trail.count(b"d")}


def check_identities(st, ops, nq=None, nr=None):
    """What holds for every string; with the lengths of the two sequences for an aligner's string (every base in one column)."""
    assert st["length"] == len(ops)
    assert st["columns"] == st["matches"] + st["mismatches"] + st["ins"] + st["del"]
    if nq is not None:
        assert st["matches"] + st["mismatches"] + st["ins"] + st["lead_i"] + st["trail_i"] == nq
        assert st["matches"] + st["mismatches"] + st["del"] + st["lead_d"] + st["trail_d"] == nr


HAND = [
    b"", b"dddd", b"iiii", b"id",
    b"i" * 200 + b"=" * 100 + b"d" * 200,
    b"II==DD", b"I", b"D", b"iiII==DDdd", b"idI=Did",           # runs at the very first and the very last walk column
    b"==IIIDD==", b"=IDIDID=", b"=IIDDDIIII=",                  # 'I' directly followed by 'D'
    b"=I=II=III=IIII=D=DD=", b"==XX==X=", b"ddii=X=iidd",
    b"i" * 70 + b"I" * 130 + b"=" + b"D" * 64 + b"X" + b"I" * 63 + b"=" * 65 + b"d" * 3,
    b"=ii=", b"=d=i=",                                          # (no aligner writes these: end-gap bytes inside the walk count nowhere)
]


@pytest.mark.parametrize("ops", HAND, ids=lambda o: api.ops_to_cigar(o) or "empty")
def test_hand_written_strings(ops):
    st = api.ops_stats(ops)
    assert tuple(st) == FIELDS
    assert st == py_stats(ops)
    check_identities(st, ops)


def test_hand_written_values():
    """A few values spelled out, so that the restatement above is not the only witness."""
    z = dict.fromkeys(FIELDS, 0)
    assert api.ops_stats(b"") == z
    assert api.ops_stats(b"dddd") == {**z, "length": 4, "lead_d": 4}
    assert api.ops_stats(b"iiii") == {**z, "length": 4, "lead_i": 4}
    assert api.ops_stats(b"id") == {**z, "length": 2, "lead_i": 1, "lead_d": 1}
    assert api.host_align_ops(b"A", b"C")[0] == b"id"
    assert api.ops_stats(b"i" * 200 + b"=" * 100 + b"d" * 200) == {**z, "length": 500, "columns": 100, "matches": 100, "lead_i": 200,
                                                                    "trail_d": 200}
    assert api.ops_stats(b"iiII=XDDDdd") == {**z, "length": 11, "columns": 7, "matches": 1, "mismatches": 1, "ins": 2, "del": 3,
                                             "ins_runs": 1, "del_runs": 1, "longest_ins": 2, "longest_del": 3, "lead_i": 2,
                                             "trail_d": 2}
    assert api.ops_stats(b"=IIDDDIIII=")["ins_runs"] == 2 and api.ops_stats(b"=IIDDDIIII=")["longest_ins"] == 4


def test_structure_and_reserved_words():
    """64 bytes, the field order of the header, the reserved words written as 0 over whatever was there."""
    assert C.sizeof(_lib.AlnStats) == 64 and api.ALN_STATS_DTYPE.itemsize == 64
    assert [n for n, _ in _lib.AlnStats._fields_] == list(FIELDS) + ["reserved"]
    assert api.ALN_STATS_DTYPE.names == FIELDS + ("reserved",)
    st = _lib.AlnStats()
    C.memset(C.byref(st), 0xA5, 64)
    assert _lib.load().ioc_host_ops_stats(b"=I=", 3, C.byref(st)) == 0
    assert list(st.reserved) == [0, 0] and st.length == 3 and st.trail_d == 0


@pytest.mark.parametrize("ops", [b"==Q==", b"=\x00=", b"M", b"== ", b"iiN"])
def test_a_byte_that_is_no_operation(ops):
    st = _lib.AlnStats()
    assert _lib.load().ioc_host_ops_stats(ops, len(ops), C.byref(st)) == -1  # IOC_ERR_ARG, as ioc_host_ops_to_cigar
    with pytest.raises(ValueError):
        api.ops_stats(ops)
    with pytest.raises(ValueError):
        api.ops_to_cigar(ops)


def test_host_aligner_output():
    """Every string ioc_host_align_ops returns for the small random pairs (lengths 0 .. 200, every gap-open class, half of them
    against the reverse complement)."""
    L = _lib.load()
    seqs, pairs = _small_pairs(13)
    shapes = set()
    for qi, ri, rc, e in pairs:
        q, r = seqs[qi], revcomp(seqs[ri]) if rc else seqs[ri]
        ops, _ = api.host_align_ops(q, r, gap_open=L.ioc_host_gap_open(e))
        st = api.ops_stats(ops)
        assert st == py_stats(ops), (qi, ri, rc, e)
        check_identities(st, ops, len(q), len(r))
        shapes.add((st["columns"] > 0, st["ins_runs"] > 1, st["del_runs"] > 1, st["lead_i"] + st["lead_d"] > 0, st["trail_i"] + st["trail_d"] > 0))
    assert len(shapes) >= 6  # (the pairs do cover strings with and without a walk, with several gaps, with end gaps on either side)
