"""The host definitions of the quality-weighted pileup and call — ioc_host_qual_weight, ioc_host_ops_pileup_weighted and
ioc_host_pileup_call_weighted — against the plain-Python restatement of tests/polish_weight_common.py, against tables and outputs
spelled out by hand, against the two equivalences with the unweighted call, and on the closed-form case in which the weights and
not the counts decide.  The kernels are tested against these functions (test_gpu_pile_call_weighted.py,
test_gpu_align_polish_weighted.py).  Integers and bytes, no tolerance."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from isonclust2_amd.api import ops_pileup_weighted, pileup_call_weighted, qual_weight  # (the names this feature adds)
from tests import polish_common as pc
from tests import polish_weight_common as pw
from tests.test_align_pileup_host import HAND, MORE, lengths
from tests.test_pile_call_host import RUNS

# 'D' with both neighbours, with q == 0 and with q == qlen, alone, and a run of 8 'I' (six slots and `longer`)
DELS = [b"=D=", b"D=", b"=D", b"D", b"DD==", b"==DD", b"dD=", b"iD=", b"=Di", b"=DI=", b"=ID=", b"=" + b"I" * 8 + b"=", b"I" * 8, b"id"]
CLAMPS = bytes([0, 33, 34, 35, 126, 255])


def _query(rng, n, letters=b"ACGT"):
    return bytes(rng.choice(letters) for _ in range(n))


def test_weight_of_every_byte():
    for b in range(256):
        assert qual_weight(b) == pw.py_weight(b) and 1 <= qual_weight(b) <= 93
    assert [qual_weight(b) for b in CLAMPS] == [1, 1, 1, 2, 93, 93]
    assert qual_weight(ord("#")) == 2 and qual_weight(ord("I")) == 40


@pytest.mark.parametrize("ops", HAND + MORE + RUNS + DELS, ids=lambda o: api.ops_to_cigar(o) or "empty")
def test_weighted_tables_of_hand_written_strings(ops):
    rng = random.Random(len(ops))
    nq, nr = lengths(ops)
    for letters, quals in ((b"ACGT", CLAMPS), (b"ACGTNacgtRY-", bytes(range(256)))):
        q, ql = _query(rng, nq, letters), _query(rng, nq, quals)
        wcols, wins = ops_pileup_weighted(ops, q, ql, nr)
        wc, wi = pw.py_pileup_weighted(ops, q, ql, nr)
        assert np.array_equal(wcols, wc) and np.array_equal(wins, wi), (ops, q, ql)
        assert not wcols["ins_runs"].any() and not wcols["ins_bases"].any() and not wins["reserved"].any()
        # every event carries a weight of 1 .. 93: the weights lie between the counts and 93 times the counts
        cols, ins = api.ops_pileup(ops, q, nr), api.ops_pileup_ins(ops, q, nr)
        for f in pc.COL_FIELDS:
            assert ((cols[f] <= wcols[f]) & (wcols[f] <= 93 * cols[f])).all()
        assert ((ins["slot"] <= wins["slot"]) & (wins["slot"] <= 93 * ins["slot"])).all()


def test_weighted_table_values():
    """Tables spelled out, so that the restatement is not the only witness."""
    #            q:  0    1    2    3              weights 2, 40, 93, 1
    q, ql = b"ACGT", bytes([35, 73, 126, 0])
    wcols, wins = ops_pileup_weighted(b"=D=I=D", q, ql, 5)  # rows: A, D, C, (I: G) T, D, -
    assert [int(wcols["a"][0]), int(wcols["del"][1]), int(wcols["c"][2]), int(wcols["t"][3]), int(wcols["del"][4])] == [2, 2, 40, 1, 1]
    assert int(wins["slot"][3, 0, 2]) == 93 and wins["slot"].sum() == 93 and sum(int(wcols[f].sum()) for f in pc.COL_FIELDS) == 46
    # 'D' in front of the first base takes that base's weight, behind the last one the last one's, alone in the world 1
    assert int(ops_pileup_weighted(b"D=", b"A", b"I", 2)[0]["del"][0]) == 40
    assert int(ops_pileup_weighted(b"=D", b"A", b"+", 2)[0]["del"][1]) == 10
    assert int(ops_pileup_weighted(b"D", b"", b"", 1)[0]["del"][0]) == 1
    # ... and between a heavy and a light base the light one's, whichever side it is on
    assert int(ops_pileup_weighted(b"=D=", b"AC", b"I#", 3)[0]["del"][1]) == 2 == int(ops_pileup_weighted(b"=D=", b"AC", b"#I", 3)[0]["del"][1])
    # free end gaps add nothing, and do not count as neighbours that are missing: q runs over them
    wcols, wins = ops_pileup_weighted(b"iidd=D=ii", b"GGACTT", b"~~I5~~", 5)
    assert int(wcols["a"][2]) == 40 and int(wcols["del"][3]) == 20 and int(wcols["c"][4]) == 20
    assert sum(int(wcols[f].sum()) for f in pc.COL_FIELDS) == 80 and not wins["slot"].any()
    # a run of 8: six slots by base, two bases in `longer`
    wcols, wins = ops_pileup_weighted(b"=" + b"I" * 8 + b"=", b"A" + b"ACGTACGT" + b"A", b"I" + bytes(range(34, 42)) + b"I", 2)
    want = np.zeros((3, 6, 5), np.uint32)
    for j, (ch, w) in enumerate(zip([0, 1, 2, 3, 0, 1], [1, 2, 3, 4, 5, 6])):
        want[1, j, ch] = w
    assert np.array_equal(wins["slot"], want) and list(wins["longer"]) == [0, 7 + 8, 0]


def test_sums_wrap_modulo_2_32():
    wcols = np.zeros(2, api.PILEUP_DTYPE)
    wins = np.zeros(2, api.PILEUP_INS_DTYPE)
    wcols["a"][0], wins["slot"][0, 0, 1] = pc.M32 - 5, pc.M32
    ops_pileup_weighted(b"I=", b"CA", b"II", 1, wcols=wcols, wins=wins)
    assert int(wcols["a"][0]) == 34 and int(wins["slot"][0, 0, 1]) == 39


@pytest.mark.parametrize("case", ["byte", "query_short", "query_long", "ref_short", "ref_long", "len_2_31", "qual_null", "wcols_null"])
def test_refusals_leave_both_tables_untouched_and_calls_add_up(case):
    L = _lib.load()
    ops, q, ql, nr = b"i=X=IID=d", b"TACGAAC", b"I#5~!+I", 6
    assert lengths(ops) == (len(q), nr)
    wcols, wins = ops_pileup_weighted(ops, q, ql, nr)
    once_c, once_i = wcols.copy(), wins.copy()
    args = {"byte": (b"i=X=IQD=d", len(ops), q, ql, len(q), nr), "query_short": (ops, len(ops), q, ql, len(q) - 1, nr),
            "query_long": (ops, len(ops), q + b"A", ql + b"I", len(q) + 1, nr), "ref_short": (ops, len(ops), q, ql, len(q), nr - 1),
            "ref_long": (ops, len(ops), q, ql, len(q), nr + 1), "len_2_31": (ops, 1 << 31, q, ql, len(q), nr),
            "qual_null": (ops, len(ops), q, None, len(q), nr), "wcols_null": (ops, len(ops), q, ql, len(q), nr)}[case]
    room_c, room_i = np.zeros(nr + 2, api.PILEUP_DTYPE), np.zeros(nr + 2, api.PILEUP_INS_DTYPE)
    room_c[:nr + 1], room_i[:nr + 1] = wcols, wins
    before_c, before_i = room_c.copy(), room_i.copy()
    assert L.ioc_host_ops_pileup_weighted(*args, None if case == "wcols_null" else room_c.ctypes.data, room_i.ctypes.data) == -1  # IOC_ERR_ARG
    assert np.array_equal(room_c, before_c) and np.array_equal(room_i, before_i)
    got = ops_pileup_weighted(ops, q, ql, nr, wcols=wcols, wins=wins)
    assert got[0] is wcols and got[1] is wins
    for f in pc.COL_FIELDS:
        assert np.array_equal(wcols[f], 2 * once_c[f])
    assert np.array_equal(wins["slot"], 2 * once_i["slot"]) and np.array_equal(wins["longer"], 2 * once_i["longer"])
    # wins may be NULL: the first table alone
    alone = np.zeros(nr + 1, api.PILEUP_DTYPE)
    assert L.ioc_host_ops_pileup_weighted(ops, len(ops), q, ql, len(q), nr, alone.ctypes.data, None) == 0 and np.array_equal(alone, once_c)
    with pytest.raises(ValueError):
        ops_pileup_weighted(ops, q, ql[:-1], nr)
    with pytest.raises(ValueError):
        ops_pileup_weighted(ops, q, ql, nr, wcols=np.zeros(nr, api.PILEUP_DTYPE))


@pytest.mark.parametrize("case", pw.HAND_CALLS_W, ids=lambda c: c[0])
def test_weighted_call_of_hand_written_tables(case):
    frame, cols, wcols, wins, md, seq, qual, st = pw.hand_case_w(case)
    assert pw.py_call_weighted(cols, wcols, wins, frame, md) == (seq, qual, st), "the restatement"
    assert pileup_call_weighted(cols, wcols, wins, frame, md) == (seq, qual, st)


@pytest.mark.parametrize("case", pc.HAND_CALLS, ids=lambda c: c[0])
def test_weighted_call_of_one_table_is_the_majority_call(case):
    """The tables of weights equal to the counts: every hand case of the majority call holds as it stands."""
    frame, cols, ins, md, seq, qual, st = pc.hand_case(case)
    assert pileup_call_weighted(cols, cols, ins, frame, md) == (seq, qual, st) == pw.py_call_weighted(cols, cols, ins, frame, md)


def test_weighted_call_of_random_tables_equals_the_restatement():
    rng = np.random.default_rng(19)
    for t in range(60):
        rlen = int(rng.integers(0, 40))
        cols, wcols, wins = pw.random_tables_w(rng, rlen + 1) if t % 2 else pw.random_tables_w(rng, rlen + 1, values=(0, 1, 2, 3, 4, 5))
        if t % 2 == 0:
            cols, _ = pc.random_tables(rng, rlen + 1, values=(0, 1, 2, 3))
        frame = bytes(rng.choice(list(b"ACGTNacgtR"), rlen).astype(np.uint8))
        for md in (1, 3):
            assert pileup_call_weighted(cols, wcols, wins, frame, md) == pw.py_call_weighted(cols, wcols, wins, frame, md), (t, md)


def test_weighted_call_refusals():
    frame, cols, wcols, wins, md, seq, qual, st = pw.hand_case_w(pw.HAND_CALLS_W[5])
    L = _lib.load()
    bound = api.pileup_call_bound(len(frame))
    out_s, out_q = C.create_string_buffer(b"\xA5" * bound, bound), C.create_string_buffer(b"\xA5" * bound, bound)
    rec = _lib.PolishStats(out_len=-7)
    tabs = (cols.ctypes.data, wcols.ctypes.data, wins.ctypes.data)
    assert L.ioc_host_pileup_call_weighted(*tabs, frame, len(frame), 0, out_s, out_q, bound, C.byref(rec)) == -1       # min_depth < 1
    assert L.ioc_host_pileup_call_weighted(*tabs, frame, -1, 1, out_s, out_q, bound, C.byref(rec)) == -1
    assert L.ioc_host_pileup_call_weighted(tabs[0], None, tabs[2], frame, len(frame), 1, out_s, out_q, bound, C.byref(rec)) == -1
    assert L.ioc_host_pileup_call_weighted(*tabs, frame, len(frame), 1, out_s, out_q, bound - 1, C.byref(rec)) == -4   # IOC_ERR_CAPACITY
    assert out_s.raw == b"\xA5" * bound == out_q.raw and rec.out_len == -7
    assert L.ioc_host_pileup_call_weighted(*tabs, frame, len(frame), 1, out_s, out_q, bound, None) == len(seq)          # (the record may be NULL)
    assert out_s.raw[:len(seq)] == seq and out_s.raw[len(seq):] == b"\xA5" * (bound - len(seq))
    with pytest.raises(api.IocError):
        pileup_call_weighted(cols, wcols, wins, frame, 0)
    with pytest.raises(api.IocError):
        pileup_call_weighted(cols, wcols, wins, frame, 1, cap=bound - 1)


@pytest.mark.parametrize("qual_byte", [0, 33, 34, ord('"'), ord("#"), ord("I"), 126, 255])
def test_constant_qualities_give_the_majority_call(qual_byte):
    """Every quality byte <= 34: the tables of weights ARE the counts.  Every byte one constant c: they are w(c) times the counts,
    and the call, qualities included, is the majority call."""
    T, rep, reads = pc.noisy()
    quals = [bytes([qual_byte]) * len(r) for r in reads]
    cols, ins, wcols, wins, _ = pw.host_tables_w(rep, reads, quals)
    w = pw.py_weight(qual_byte)
    for f in pc.COL_FIELDS:
        assert np.array_equal(wcols[f], w * cols[f])
    assert np.array_equal(wins["slot"], w * ins["slot"]) and np.array_equal(wins["longer"], w * ins["longer"])
    for md in (1, 3):
        assert pileup_call_weighted(cols, wcols, wins, rep, md) == api.pileup_call(cols, ins, rep, md)


def test_low_qualities_mixed_give_the_majority_call():
    """Bytes 0 .. 34 mixed at random all weigh 1."""
    T, rep, reads = pc.noisy()
    quals = pw.random_quals(np.random.default_rng(3), reads, 0, 34)
    cols, ins, wcols, wins, _ = pw.host_tables_w(rep, reads, quals)
    assert all(np.array_equal(wcols[f], cols[f]) for f in pc.COL_FIELDS) and np.array_equal(wins, ins)
    assert pileup_call_weighted(cols, wcols, wins, rep, 3) == api.pileup_call(cols, ins, rep, 3)


def test_random_qualities_equal_the_restatement():
    T, rep, reads = pc.noisy()
    quals = pw.random_quals(np.random.default_rng(4), reads)
    cols, ins, wcols, wins, strings = pw.host_tables_w(rep, reads, quals)
    wc, wi = np.zeros_like(wcols), np.zeros_like(wins)
    for rd, ql, ops in zip(reads, quals, strings):
        pw.py_pileup_weighted(ops, rd, ql, len(rep), wc, wi)
    assert np.array_equal(wcols, wc) and np.array_equal(wins, wi)
    for md in (1, 3):
        assert pileup_call_weighted(cols, wcols, wins, rep, md) == pw.py_call_weighted(cols, wcols, wins, rep, md)


def test_closed_form_the_weights_decide():
    """Three reads of five carry a substitution, a deletion and an insertion, each under quality '#'; two reads equal T under 'I'.
    The majority call follows the three; the weighted call returns exactly T."""
    T, edited, reads, quals = pw.closed_form()
    assert len(T) == 300 and len(edited) == 300 and edited != T
    # the edits align as one X, one D and one I at their places: the construction rests on it
    ops, _ = api.host_align_ops(edited, T, gap_open=pc.gap_open(0.1))
    assert ops == b"=" * 100 + b"X" + b"=" * 79 + b"D" + b"=" * 59 + b"I" + b"=" * 60
    assert bytes(quals[0][x] for x in (97, 98, 102, 103, 177, 178, 182, 183, 236, 237, 241, 242)) == b"I##I" * 3
    cols, ins, wcols, wins, _ = pw.host_tables_w(T, reads, quals)
    seq, qual, st = api.pileup_call(cols, ins, T, 3)
    assert seq == edited and (st["n_sub"], st["n_del"], st["n_ins"], st["n_low"]) == (1, 1, 1, 0)
    seq, qual, st = pileup_call_weighted(cols, wcols, wins, T, 3)
    assert seq == T and st == dict(out_len=300, n_sub=0, n_del=0, n_ins=0, n_low=0)
    # the three contested columns: 80 of 86 by weight, 40 * 80 / 86 = 37; everywhere else unanimous
    assert qual == b"".join(bytes([33 + (37 if p in (100, 180) else 40)]) for p in range(300))
    assert (seq, qual, st) == pw.py_call_weighted(cols, wcols, wins, T, 3)
