"""The two host definitions behind the polished consensus — ioc_host_ops_pileup_ins (what the reads insert, per row, by index in
the run and by base) and ioc_host_pileup_call (the majority call over both tables) — against the plain-Python restatement of
tests/polish_common.py, against tables and outputs spelled out by hand, and against a closed-form anchor that needs neither.  The
kernels are tested against these two functions (test_gpu_pile_call.py, test_gpu_align_polish.py).  Integers and bytes, no tolerance."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import polish_common as pc
from tests.test_align_pileup_host import HAND, MORE, lengths

RUNS = [b"=" * 3 + b"I" * n + b"=" * 2 for n in (1, 5, 6, 7, 130)] + [b"I" * 7, b"==" + b"I" * 130, b"=IIIIIIID" + b"I" * 8 + b"="]


def _query(rng, n, letters=b"ACGT"):
    return bytes(rng.choice(letters) for _ in range(n))


def check_identities(ops, query, rlen, ins):
    """Per row: the sum over slot[0] is ins_runs, the sum over all slots plus `longer` is ins_bases."""
    cols = api.ops_pileup(ops, query, rlen)
    assert np.array_equal(ins["slot"][:, 0, :].sum(axis=1), cols["ins_runs"])
    assert np.array_equal(ins["slot"].reshape(rlen + 1, -1).sum(axis=1) + ins["longer"], cols["ins_bases"])
    assert not ins["reserved"].any()


@pytest.mark.parametrize("ops", HAND + MORE + RUNS, ids=lambda o: api.ops_to_cigar(o) or "empty")
def test_ins_table_of_hand_written_strings(ops):
    rng = random.Random(len(ops))
    nq, nr = lengths(ops)
    for letters in (b"ACGT", b"ACGTNacgtRY-"):
        q = _query(rng, nq, letters)
        got = api.ops_pileup_ins(ops, q, nr)
        assert got.dtype == api.PILEUP_INS_DTYPE and got.shape == (nr + 1,)
        assert np.array_equal(got, pc.py_pileup_ins(ops, q, nr)), (ops, q)
        check_identities(ops, q, nr, got)


def test_ins_table_values():
    """Tables spelled out, so that the restatement is not the only witness."""
    assert api.PILEUP_INS_DTYPE.itemsize == 128 == C.sizeof(_lib.PileupIns) and api.POLISH_STATS_DTYPE.itemsize == 32 == C.sizeof(_lib.PolishStats)
    t = api.ops_pileup_ins(b"II=D=III", b"GGTAGNG", 3)
    want = np.zeros((4, 6, 5), np.uint32)
    want[0, 0, 2] = want[0, 1, 2] = 1                    # GG in front of row 0
    want[3, 0, 2] = want[3, 1, 4] = want[3, 2, 2] = 1    # GNG behind the last base
    assert np.array_equal(t["slot"], want) and not t["longer"].any()
    t = api.ops_pileup_ins(b"=" + b"I" * 9 + b"=", b"A" + b"ACGTACGTA" + b"A", 2)
    want = np.zeros((3, 6, 5), np.uint32)
    for j, ch in enumerate([0, 1, 2, 3, 0, 1]):
        want[1, j, ch] = 1
    assert np.array_equal(t["slot"], want) and list(t["longer"]) == [0, 3, 0]
    # a run interrupted by 'D' starts anew, in front of the next row
    t = api.ops_pileup_ins(b"=IDI=", b"ACTA", 3)
    assert t["slot"][1, 0, 1] == 1 and t["slot"][2, 0, 3] == 1 and t["slot"].sum() == 2


@pytest.mark.parametrize("case", ["byte", "query_short", "query_long", "ref_short", "ref_long", "len_2_31"])
def test_ins_refusals_leave_the_table_untouched_and_calls_add_up(case):
    L = _lib.load()
    ops, q, nr = b"i=X=IID=d", b"TACGAAC", 6
    assert lengths(ops) == (len(q), nr)
    ins = api.ops_pileup_ins(ops, q, nr)
    once = ins.copy()
    args = {"byte": (b"i=X=IQD=d", len(ops), q, len(q), nr), "query_short": (ops, len(ops), q, len(q) - 1, nr),
            "query_long": (ops, len(ops), q + b"A", len(q) + 1, nr), "ref_short": (ops, len(ops), q, len(q), nr - 1),
            "ref_long": (ops, len(ops), q, len(q), nr + 1), "len_2_31": (ops, 1 << 31, q, len(q), nr)}[case]
    room = np.zeros(nr + 2, api.PILEUP_INS_DTYPE)
    room[:nr + 1] = ins
    before = room.copy()
    assert L.ioc_host_ops_pileup_ins(*args, room.ctypes.data) == -1  # IOC_ERR_ARG
    assert np.array_equal(room, before)
    assert api.ops_pileup_ins(ops, q, nr, ins=ins) is ins
    assert np.array_equal(ins["slot"], 2 * once["slot"]) and np.array_equal(ins["longer"], 2 * once["longer"])
    with pytest.raises(ValueError):
        api.ops_pileup_ins(ops, q, nr, ins=np.zeros(nr, api.PILEUP_INS_DTYPE))


@pytest.mark.parametrize("case", pc.HAND_CALLS, ids=lambda c: c[0])
def test_call_of_hand_written_tables(case):
    frame, cols, ins, md, seq, qual, st = pc.hand_case(case)
    assert pc.py_call(cols, ins, frame, md) == (seq, qual, st), "the restatement"
    assert api.pileup_call(cols, ins, frame, md) == (seq, qual, st)


def test_call_of_random_tables_equals_the_restatement():
    """Tables no aligner would produce, counts up to 2^32 - 1 in every channel, frames with other letters, both depths."""
    rng = np.random.default_rng(9)
    for t in range(60):
        rlen = int(rng.integers(0, 40))
        cols, ins = pc.random_tables(rng, rlen + 1, values=(0, 1, 2, 3, 2**31, pc.M32) if t % 2 else (0, 1, 2, 3, 4, 5))
        frame = bytes(rng.choice(list(b"ACGTNacgtR"), rlen).astype(np.uint8))
        for md in (1, 3):
            assert api.pileup_call(cols, ins, frame, md) == pc.py_call(cols, ins, frame, md), (t, md)


def test_call_refusals():
    frame, cols, ins, md, seq, qual, st = pc.hand_case(pc.HAND_CALLS[4])
    L = _lib.load()
    bound = api.pileup_call_bound(len(frame))
    assert bound == len(frame) + 6 * (len(frame) + 1)
    out_s, out_q = C.create_string_buffer(b"\xA5" * bound, bound), C.create_string_buffer(b"\xA5" * bound, bound)
    rec = _lib.PolishStats(out_len=-7)
    args = (cols.ctypes.data, ins.ctypes.data, frame, len(frame))
    assert L.ioc_host_pileup_call(*args, 0, out_s, out_q, bound, C.byref(rec)) == -1       # min_depth < 1
    assert L.ioc_host_pileup_call(cols.ctypes.data, ins.ctypes.data, frame, -1, 1, out_s, out_q, bound, C.byref(rec)) == -1
    assert L.ioc_host_pileup_call(*args, 1, out_s, out_q, bound - 1, C.byref(rec)) == -4   # IOC_ERR_CAPACITY
    assert out_s.raw == b"\xA5" * bound == out_q.raw and rec.out_len == -7
    assert L.ioc_host_pileup_call(*args, 1, out_s, out_q, bound, None) == len(seq)          # (the record may be NULL)
    assert out_s.raw[:len(seq)] == seq and out_s.raw[len(seq):] == b"\xA5" * (bound - len(seq))
    with pytest.raises(api.IocError):
        api.pileup_call(cols, ins, frame, 0)
    with pytest.raises(api.IocError):
        api.pileup_call(cols, ins, frame, 1, cap=bound - 1)


def test_identical_reads_closed_form():
    """The anchor that needs neither the restatement nor a table written by hand: five identical reads equal to T correct a
    representative with one substitution, a 2-base deletion and a 1-base insertion back to exactly T."""
    T, rep = pc.anchor()
    assert len(T) == 300 and len(rep) == 299 and rep != T
    cols, ins, _ = pc.host_tables(rep, [T] * 5)
    seq, qual, st = api.pileup_call(cols, ins, rep, 3)
    assert seq == T
    assert (st["n_sub"], st["n_del"], st["n_ins"], st["n_low"], st["out_len"]) == (1, 1, 2, 0, 300)
    assert qual == bytes([33 + 40]) * 300


def test_noisy_reads_bring_the_representative_closer():
    """15 reads of 400 bases, each mutated independently at 6 %, on a representative damaged at 12 % (seed 11): the polished
    sequence is strictly closer to T than the representative was.  Values tried through the host definitions alone when the
    builder was fixed, as (reads, length, rate, seed): distance before -> after.  (15, 400, 0.06, 11): 38 -> 0, the one asserted;
    (15, 400, 0.06, 12): 53 -> 0; (15, 400, 0.06, 13): 38 -> 1; (15, 1000, 0.06, 11): 103 -> 1; (5, 400, 0.06, 11): 38 -> 1;
    (5, 400, 0.15, 11): 91 -> 25."""
    T, rep, reads = pc.noisy()
    cols, ins, _ = pc.host_tables(rep, reads)
    seq, qual, st = api.pileup_call(cols, ins, rep, 3)
    before, after = pc.distance(rep, T), pc.distance(seq, T)
    assert st["n_sub"] + st["n_del"] + st["n_ins"] > 0 and len(qual) == len(seq)
    assert after < before, (after, before)
