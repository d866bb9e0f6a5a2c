"""ioc_host_ops_project_ins and ioc_host_planes_pile, the two definitions the groups' consensus rests on, against a byte-by-byte
restatement in Python; and the relation the header states between the tables piled from a string's planes and its pileup: equal
in every field but ins_bases (at most IOC_PILE_INS_SLOTS per run) and `longer` (0), and the same consensus call from either.
Bytes and integers only, no tolerance.  No GPU."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import plane_pile_common as pp
from tests import polish_common as pc
from tests import sites_common as sc


def _aligned_strings():
    """(ops, read, frame) of the host aligner over the reads of polish_common.noisy() and sites_common.haplotypes()."""
    out = []
    T, rep, reads = pc.noisy()
    for rd in reads:
        out.append((api.host_align_ops(rd, rep, gap_open=pc.gap_open(0.1))[0], rd, rep))
    T, B, reads = sc.haplotypes()
    for rd in reads:
        out.append((api.host_align_ops(rd, T, gap_open=pc.gap_open(0.1))[0], rd, T))
        out.append((api.host_align_ops(rd, B, gap_open=pc.gap_open(0.1))[0], rd, B))
    return out


def _random_strings():
    rng = random.Random(77)
    return [sc.random_ops(rng, n) for n in (0, 1, 2, 7, 63, 64, 65, 300, 1000) for _ in range(3)]


def _long_runs():
    """Runs of 6, 7 and 70 'I' bytes, at the start, in the middle and at the end of a string."""
    rng = random.Random(5)
    out = []
    for run in (6, 7, 70):
        for ops in (b"I" * run + b"==X=", b"=X" + b"I" * run + b"D==", b"===" + b"I" * run, b"=" + b"I" * run + b"=" + b"I" * 2 + b"="):
            q = sum(ops.count(c) for c in b"=XIi")
            out.append((ops, bytes(rng.choice(b"ACGTN") for _ in range(q)), sum(ops.count(c) for c in b"=XDd")))
    return out


def _check_relation(ops, query, rlen, frame=None):
    """The header's relation, for a string with at most one run per row."""
    base, slots = pp.planes_of(ops, query, rlen)
    cols, ins = api.planes_pile(base, slots)
    want_c, want_i = api.ops_pileup(ops, query, rlen), api.ops_pileup_ins(ops, query, rlen)
    for f in ("a", "c", "g", "t", "other", "del", "ins_runs"):
        assert np.array_equal(cols[f], want_c[f]), f
    assert np.array_equal(ins["slot"], want_i["slot"]) and not ins["longer"].any() and not ins["reserved"].any()
    runs = pp.ins_run_lengths(ops)
    assert cols["ins_bases"].tolist() == [sum(min(x, pp.SLOTS) for x in runs.get(r, [])) for r in range(rlen + 1)]
    rng = random.Random(rlen)
    frame = bytes(rng.choice(b"ACGT") for _ in range(rlen)) if frame is None else frame
    for md in (1, 3):
        assert api.pileup_call(cols, ins, frame, md) == api.pileup_call(want_c, want_i, frame, md)


def test_project_ins_against_the_restatement():
    cases = _random_strings() + _long_runs() + [(o, r, len(f)) for o, r, f in _aligned_strings()]
    assert any(not pp.runs_per_row_at_most_one(o) for o, _, _ in cases)   # the walk is defined for any string
    for ops, query, rlen in cases:
        got = api.ops_project_ins(ops, query, rlen)
        assert got.shape == (pp.SLOTS, rlen + 1) and got.tolist() == pp.py_project_ins(ops, query, rlen), ops[:40]


def test_project_ins_by_hand():
    # d = X I I D = i: the run of two stands in front of row 3 and takes query[2], query[3]
    ops, query, rlen = sc.HAND_PROJECTION[:3]
    got = api.ops_project_ins(ops, query, rlen)
    want = np.zeros((pp.SLOTS, rlen + 1), np.uint8)
    want[0, 3], want[1, 3] = 1 + 2, 1 + 3   # G, T
    assert np.array_equal(got, want)
    # 'd' ends a run and moves on: III in front of row 0, I in front of row 1
    got = api.ops_project_ins(b"IIIdiI=", b"ACGTNA", 2)
    assert got[:, 1].tolist() == [1 + 4, 0, 0, 0, 0, 0] and got[:, 0].tolist() == [1 + 0, 1 + 1, 1 + 2, 0, 0, 0] and not got[:, 2].any()
    # 'i' ends a run without moving the row: the second run in front of row 0 overwrites slot 0 and clears nothing
    got = api.ops_project_ins(b"IIIiI=", b"ACGTNA", 1)
    assert got[:, 0].tolist() == [1 + 4, 1 + 1, 1 + 2, 0, 0, 0]


def test_planes_pile_against_the_restatement():
    rng = np.random.default_rng(3)
    for rows in (1, 2, 64, 65, 257):
        cols, ins = pc.random_tables(rng, rows, values=(0, 1, 2, 3, 2**31))
        want_c, want_i = cols.copy(), ins.copy()
        for _ in range(3):
            base = rng.choice(pp.BASE_BYTES, rows).astype(np.uint8)
            slots = rng.choice(pp.SLOT_BYTES, (pp.SLOTS, rows), p=(0.5, 0.1, 0.1, 0.1, 0.1, 0.1)).astype(np.uint8)
            api.planes_pile(base, slots, cols=cols, ins=ins)
            pp.py_planes_pile(base, slots, want_c, want_i)
        assert cols.tobytes() == want_c.tobytes() and ins.tobytes() == want_i.tobytes()


def test_the_stated_relation_on_aligned_strings():
    n = 0
    for ops, rd, frame in _aligned_strings():
        assert pp.runs_per_row_at_most_one(ops)
        _check_relation(ops, rd, len(frame), frame)
        n += 1
    assert n >= 30


def test_the_stated_relation_on_random_strings_and_long_runs():
    cases = [c for c in _random_strings() + _long_runs() if pp.runs_per_row_at_most_one(c[0])]
    assert len(cases) >= 12 and any(max(max(v) for v in pp.ins_run_lengths(o).values()) == 70 for o, _, _ in cases if pp.ins_run_lengths(o))
    for ops, query, rlen in cases:
        _check_relation(ops, query, rlen)


@pytest.mark.parametrize("run", [6, 7, 70])
def test_long_runs_keep_six(run):
    query = bytes(b"ACGTN"[i % 5] for i in range(run + 2))
    slots = api.ops_project_ins(b"=" + b"I" * run + b"=", query, 2)
    assert slots[:, 1].tolist() == [1 + (1 + j) % 5 for j in range(6)] and not slots[:, 0].any() and not slots[:, 2].any()
    cols, ins = api.planes_pile(api.ops_project(b"=" + b"I" * run + b"=", query, 2)[0], slots)
    assert int(cols["ins_bases"][1]) == 6 and int(cols["ins_runs"][1]) == 1 and not ins["longer"].any()
    assert int(api.ops_pileup_ins(b"=" + b"I" * run + b"=", query, 2)["longer"][1]) == run - 6


def test_the_sum_over_a_cluster_calls_what_the_pileup_calls():
    """The tables piled from every read's planes give the consensus ioc_host_pileup_call gives from the two pileups."""
    T, rep, reads = pc.noisy()
    cols, ins, strings = pc.host_tables(rep, reads)
    pc_, pi_ = np.zeros(len(rep) + 1, api.PILEUP_DTYPE), np.zeros(len(rep) + 1, api.PILEUP_INS_DTYPE)
    for ops, rd in zip(strings, reads):
        api.planes_pile(*pp.planes_of(ops, rd, len(rep)), cols=pc_, ins=pi_)
    assert api.pileup_call(pc_, pi_, rep, 3) == api.pileup_call(cols, ins, rep, 3)
    assert np.array_equal(pi_["slot"], ins["slot"])


def test_refusals_leave_the_outputs_untouched():
    L = _lib.load()
    slots = np.full((pp.SLOTS, 4), 0xA5, np.uint8)
    for ops, query, rlen in ((b"==Q", b"ACG", 3), (b"===", b"AC", 3), (b"===", b"ACG", 2), (b"=\0=", b"ACG", 3)):
        assert L.ioc_host_ops_project_ins(ops, len(ops), query, len(query), rlen, slots.ctypes.data) == -1
        with pytest.raises(ValueError):
            api.ops_project_ins(ops, query, rlen)
    assert L.ioc_host_ops_project_ins(b"===", 3, b"ACG", 3, 3, None) == -1 and L.ioc_host_ops_project_ins(b"===", -1, b"ACG", 3, 3, slots.ctypes.data) == -1
    assert (slots == 0xA5).all()
    cols, ins = np.zeros(3, api.PILEUP_DTYPE), np.zeros(3, api.PILEUP_INS_DTYPE)
    cols["a"], ins["longer"] = 9, 9
    before = cols.tobytes(), ins.tobytes()
    good_b, good_s = np.array([0, pp.DEL, pp.NONE], np.uint8), np.zeros((pp.SLOTS, 3), np.uint8)
    for bad_base in (6, 8, 255):
        b = good_b.copy()
        b[2] = bad_base   # (the last row: everything in front of it has been looked at by then)
        with pytest.raises(ValueError):
            api.planes_pile(b, good_s, cols=cols, ins=ins)
    for bad_slot in (6, 7, 255):
        s = good_s.copy()
        s[5, 2] = bad_slot
        with pytest.raises(ValueError):
            api.planes_pile(good_b, s, cols=cols, ins=ins)
    p = lambda a: a.ctypes.data
    assert L.ioc_host_planes_pile(p(good_b), p(good_s), -1, p(cols), p(ins)) == -1
    assert L.ioc_host_planes_pile(None, p(good_s), 2, p(cols), p(ins)) == -1 and L.ioc_host_planes_pile(p(good_b), None, 2, p(cols), p(ins)) == -1
    assert L.ioc_host_planes_pile(p(good_b), p(good_s), 2, None, p(ins)) == -1 and L.ioc_host_planes_pile(p(good_b), p(good_s), 2, p(cols), None) == -1
    assert (cols.tobytes(), ins.tobytes()) == before
    api.planes_pile(good_b, good_s, cols=cols, ins=ins)
    assert cols["a"].tolist() == [10, 9, 9] and cols["del"].tolist() == [0, 1, 0]
