"""The weight planes on the host alone: ioc_host_ops_project_weights and ioc_host_planes_pile_weighted against their plain-Python
restatements (iso_polish_weight_common) on hand strings and on the host aligner's strings of random reads under random quality
lines; the relation to ioc_host_ops_pileup_weighted (every field but `longer`); the weighted group call against the unweighted one
where the weights cannot decide; and the closed-form case in which they do."""
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import iso_polish_common as ic
from tests import iso_polish_weight_common as iw
from tests import plane_pile_common as pp
from tests import polish_weight_common as pw

SLOTS = pp.SLOTS
QUAL_BYTES = (0, 33, 34, 35, 126, 255)

# hand strings: the empty string, qlen 0 and 1, a 'D' at both ends of the query, runs of 5, 6, 7 and 13 'I', a run in front of row 0
# and one behind the last row, free end gaps, and two runs in front of one row (the second overwrites)
HAND = ["", "ddd", "DD", "=", "X", "I", "D=D", "DD=DD", "d=D", "=IIIII=", "=IIIIII=", "=IIIIIII=", "X" + "I" * 13 + "=D=", "III==", "==III", "ii=D=I=dd",
        "iiII=", "IIiI=X", "=DDD=IIIIIII=X=D", "=D" + "I" * 13 + "D=", "IIIIIIIDIIIII="]


def _string(rng, ops, quals=QUAL_BYTES):
    qlen, rlen = sum(ops.count(c) for c in "=XIi"), sum(ops.count(c) for c in "=XDd")
    return ops.encode(), bytes(rng.choice(b"ACGTN") for _ in range(qlen)), bytes(rng.choice(quals) for _ in range(qlen)), rlen


def _same_projection(ops, query, qual, rlen):
    wbase, wslots = api.ops_project_weights(ops, query, qual, rlen)
    pb, ps = iw.py_project_weights(ops, query, qual, rlen)
    assert wbase.tolist() == pb and wslots.tolist() == ps, ops
    return wbase, wslots


def _relation(ops, query, qual, rlen):
    """the tables piled from the four planes against ioc_host_ops_pileup_weighted of the string: every field but `longer`"""
    base, slots, wbase, wslots = iw.planes_of(ops, query, qual, rlen)
    wcols, wins = api.planes_pile_weighted(base, slots, wbase, wslots)
    pcols, pins = iw.py_planes_pile_weighted(base, slots, wbase, wslots, np.zeros(rlen + 1, api.PILEUP_DTYPE), np.zeros(rlen + 1, api.PILEUP_INS_DTYPE))
    assert wcols.tobytes() == pcols.tobytes() and wins.tobytes() == pins.tobytes()
    want_cols, want_ins = api.ops_pileup_weighted(ops, query, qual, rlen)
    assert wcols.tobytes() == want_cols.tobytes()
    assert wins["slot"].tobytes() == want_ins["slot"].tobytes() and not wins["longer"].any()
    return want_ins


def test_hand_strings_against_the_restatement_and_the_weighted_pileup():
    rng = random.Random(5)
    longer = 0
    for ops in HAND:
        for _ in range(4):
            o, query, qual, rlen = _string(rng, ops)
            wbase, wslots = _same_projection(o, query, qual, rlen)
            assert wbase.max(initial=0) <= 93 and wslots.max(initial=0) <= 93
            if pp.runs_per_row_at_most_one(o):
                longer += int(_relation(o, query, qual, rlen)["longer"].sum())
    assert longer > 0   # (the runs of 7 and 13: the one field the relation leaves out was not 0)
    # spelled out: weights 1 (bytes 0, 33, 34), 2 (35), 93 (126, 255); the 'D's take the smaller neighbour, at the ends the only one
    wbase, wslots = api.ops_project_weights(b"D=D", b"A", bytes([126]), 3)
    assert wbase.tolist() == [93, 93, 93, 0] and not wslots.any()
    wbase, wslots = api.ops_project_weights(b"=D=I=", b"ACGT", bytes([35, 255, 0, 34]), 4)
    assert wbase.tolist() == [2, 2, 93, 1, 0] and wslots[0].tolist() == [0, 0, 0, 1, 0] and not wslots[1:].any()
    wbase, wslots = api.ops_project_weights(b"DD", b"", b"", 2)
    assert wbase.tolist() == [1, 1, 0]
    wbase, wslots = api.ops_project_weights(b"IIiI=X", b"ACGTAC", bytes([35, 36, 37, 38, 39, 40]), 2)   # the second run overwrites slot 0
    assert wslots[0].tolist() == [5, 0, 0] and wslots[1].tolist() == [3, 0, 0] and wbase.tolist() == [6, 7, 0]


def test_the_host_aligner_strings_of_random_reads():
    rng, nrng = random.Random(17), np.random.default_rng(17)
    for length in (1, 7, 90, 300):
        frame = bytes(rng.choice(b"ACGT") for _ in range(length))
        reads = [_mutate(rng, frame, 0.12) for _ in range(6)]
        for lo, hi in ((33, 126), (0, 255), (30, 36)):
            quals = pw.random_quals(nrng, reads, lo, hi)
            cols, ins, wcols, wins, strings = pw.host_tables_w(frame, reads, quals)
            gw, gi = np.zeros(length + 1, api.PILEUP_DTYPE), np.zeros(length + 1, api.PILEUP_INS_DTYPE)
            for rd, ql, ops in zip(reads, quals, strings):
                assert pp.runs_per_row_at_most_one(ops)
                _same_projection(ops, rd, ql, length)
                _relation(ops, rd, ql, length)
                api.planes_pile_weighted(*iw.planes_of(ops, rd, ql, length), wcols=gw, wins=gi)
            assert gw.tobytes() == wcols.tobytes() and gi["slot"].tobytes() == wins["slot"].tobytes()


def _mutate(rng, seq, rate):
    out = bytearray()
    for b in seq:
        x = rng.random()
        if x < rate / 3:
            continue
        if x < 2 * rate / 3:
            out += bytes(rng.choice(b"ACGT") for _ in range(rng.choice((1, 1, 2, 7))))
        out.append(rng.choice(b"ACGT") if x > 1 - rate / 3 else b)
    return bytes(out)


def test_sums_are_modulo_2_32_and_the_other_fields_are_never_touched():
    base, slots = np.array([0, pp.DEL, pp.NONE], np.uint8), np.zeros((SLOTS, 3), np.uint8)
    slots[0, 0], slots[5, 2] = 3, 5
    wbase, wslots = np.array([93, 7, 50], np.uint8), np.full((SLOTS, 3), 9, np.uint8)
    wcols, wins = np.zeros(3, api.PILEUP_DTYPE), np.zeros(3, api.PILEUP_INS_DTYPE)
    wcols["a"][0], wcols["ins_runs"][:], wcols["ins_bases"][:], wins["longer"][:], wins["slot"][2, 5, 4] = 2**32 - 3, 11, 12, 13, 2**32 - 9
    api.planes_pile_weighted(base, slots, wbase, wslots, wcols=wcols, wins=wins)
    assert wcols["a"].tolist() == [90, 0, 0] and wcols["del"].tolist() == [0, 7, 0]   # (row 2 is not covered: its weight byte counts for nothing)
    assert wcols["ins_runs"].tolist() == [11] * 3 and wcols["ins_bases"].tolist() == [12] * 3 and wins["longer"].tolist() == [13] * 3
    assert int(wins["slot"][0, 0, 2]) == 9 and int(wins["slot"][2, 5, 4]) == 0 and int(wins["slot"].astype(np.int64).sum()) == 9


def test_refusals_leave_the_outputs_untouched():
    L = _lib.load()
    wb, ws = np.full(8, 0xA5, np.uint8), np.full(SLOTS * 8, 0xA5, np.uint8)
    d = lambda a: a.ctypes.data

    def project(ops=b"=I=D", n=None, query=b"ACG", qual=b"III", qlen=3, rlen=3, wbase=d(wb), wslots=d(ws)):
        return L.ioc_host_ops_project_weights(ops, len(ops) if n is None and ops is not None else n, query, qual, qlen, rlen, wbase, wslots)

    for bad in (dict(n=-1), dict(ops=None, n=4), dict(qlen=-1), dict(rlen=-1), dict(query=None), dict(qual=None), dict(wbase=None), dict(wslots=None),
                dict(ops=b"=I=M"), dict(ops=b"=I\0D", n=4), dict(qlen=2), dict(rlen=2), dict(rlen=4), dict(ops=b"=I=DI"), dict(n=2**31)):
        assert project(**bad) == -1, bad
    assert (wb == 0xA5).all() and (ws == 0xA5).all()
    assert project() == 0 and wb[:4].tolist() == [40, 40, 40, 0] and (wb[4:] == 0xA5).all() and ws[:4].tolist() == [0, 40, 0, 0]
    with pytest.raises(ValueError):
        api.ops_project_weights(b"==", b"AC", b"I", 2)
    with pytest.raises(ValueError):
        api.ops_project_weights(b"=Q", b"AC", b"II", 2)

    base, slots = np.zeros(4, np.uint8), np.zeros(SLOTS * 4, np.uint8)
    wbase, wslots = np.full(4, 9, np.uint8), np.full(SLOTS * 4, 9, np.uint8)
    wcols, wins = np.full(4 * 8, 0xA5A5A5A5, np.uint32), np.full(4 * 32, 0xA5A5A5A5, np.uint32)

    def pile(base_=base, slots_=slots, wbase_=d(wbase), wslots_=d(wslots), rlen=3, wcols_=d(wcols), wins_=d(wins)):
        return L.ioc_host_planes_pile_weighted(d(base_) if base_ is not None else None, d(slots_) if slots_ is not None else None, wbase_, wslots_, rlen, wcols_, wins_)

    six, eight, s6 = base.copy(), base.copy(), slots.copy()
    six[3], eight[0], s6[SLOTS * 4 - 1] = 6, 8, 6
    for bad in (dict(rlen=-1), dict(base_=None), dict(slots_=None), dict(wbase_=None), dict(wslots_=None), dict(wcols_=None), dict(wins_=None), dict(base_=six),
                dict(base_=eight), dict(slots_=s6)):
        assert pile(**bad) == -1, bad
    assert (wcols == 0xA5A5A5A5).all() and (wins == 0xA5A5A5A5).all()
    assert pile() == 0 and wcols[0] == (0xA5A5A5A5 + 9) % 2**32
    with pytest.raises(ValueError):
        api.planes_pile_weighted(six, slots.reshape(SLOTS, 4), wbase, wslots.reshape(SLOTS, 4))


def _groups(seed=3):
    """two segments, three and two groups, reads through the host aligner: what both definitions take, without the weights"""
    rng = random.Random(seed)
    frames = [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in (120, 61)]
    reads, sop, group = [], [], []
    for g, (frame, sizes) in enumerate(zip(frames, ((5, 4, 0), (7, 3)))):
        for h, count in enumerate(sizes):
            own = _mutate(rng, frame, 0.06)   # the group's own sequence, which its reads follow
            for _ in range(count):
                reads.append(_mutate(rng, own, 0.05)), sop.append(g), group.append(h)
        reads.append(_mutate(rng, frame, 0.05)), sop.append(g), group.append(-1)
    return frames, reads, sop, group, [3, 2]


@pytest.mark.parametrize("quals", ["equal_I", "equal_5", "at_most_34"])
@pytest.mark.parametrize("min_depth", [1, 3])
def test_where_the_weights_cannot_decide_the_call_is_the_unweighted_one(quals, min_depth):
    frames, reads, sop, group, ng = _groups()
    nrng = np.random.default_rng(4)
    lines = {"equal_I": [b"I" * len(r) for r in reads], "equal_5": [b"5" * len(r) for r in reads], "at_most_34": pw.random_quals(nrng, reads, 0, 34)}[quals]
    planes = [iw.host_planes(frames[g], [rd], [ql]) for g, rd, ql in zip(sop, reads, lines)]
    base, slots, wbase, wslots = ([p[x][0] for p in planes] for x in range(4))
    weighted = iw.host_groups_polish_weighted(frames, sop, group, ng, base, slots, wbase, wslots, min_depth)
    plain = ic.host_groups_polish(frames, sop, group, ng, base, slots, min_depth)
    ic.same_groups(weighted, plain, tables=False)
    assert weighted["gcols"].tobytes() == plain["gcols"].tobytes()
    assert any(int(p["n_sub"]) + int(p["n_del"]) + int(p["n_ins"]) > 0 for pol in plain["gpolish"] for p in pol)   # (something was called)
    assert weighted["gseq"][0][2] == frames[0] and weighted["gqual"][0][2] == b"!" * len(frames[0])               # the empty group: its frame at quality 0


def test_the_closed_form_case_the_weights_decide():
    T, edited, reads, quals = pw.closed_form(300, 300)
    reads, quals = list(reads) + [T] * 5, list(quals) + [b"I" * len(T)] * 5
    group = [0] * 5 + [1] * 5
    base, slots, wbase, wslots = iw.host_planes(T, reads, quals)
    weighted = iw.host_groups_polish_weighted([T], [0] * 10, group, [2], base, slots, wbase, wslots, 3)
    plain = ic.host_groups_polish([T], [0] * 10, group, [2], base, slots, 3)
    # 3 : 2 by count, 6 : 80 by weight (polish_weight_common.closed_form)
    assert weighted["gseq"][0][0] == T and plain["gseq"][0][0] == edited and edited != T
    assert weighted["gseq"][0][1] == T and plain["gseq"][0][1] == T
    assert tuple(int(weighted["gpolish"][0][0][f]) for f in ("n_sub", "n_del", "n_ins")) == (0, 0, 0)
    assert tuple(int(plain["gpolish"][0][0][f]) for f in ("n_sub", "n_del", "n_ins")) == (1, 1, 1)
