"""What the tests of the polished consensus share (test_pile_call_host.py, test_gpu_pile_call.py, test_gpu_align_polish.py,
test_cli_polish.py): a plain-Python restatement of the two definitions — ioc_host_ops_pileup_ins byte by byte, ioc_host_pileup_call
row by row, in Python's unbounded integers — which is the independent witness for the host functions and, through them, for the
kernels; tables spelled out by hand with the output they must give; and the builders of the closed-form anchor and of the noisy
case."""
import random

import numpy as np

from isonclust2_amd import _lib, api

SLOTS = 6
CH = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
COL_FIELDS = ("a", "c", "g", "t", "other", "del")
LETTER = b"ACGTN"
M32 = 2**32 - 1


def py_pileup_ins(ops, query, rlen):
    """The walk of ioc_host_ops_pileup_ins, byte by byte."""
    ins = np.zeros(rlen + 1, api.PILEUP_INS_DTYPE)
    r = q = j = 0
    for op in bytes(ops):
        op = chr(op)
        if op == "I":
            if j < SLOTS:
                ins["slot"][r, j, CH.get(query[q], 4)] += 1
            else:
                ins["longer"][r] += 1
            j, q = j + 1, q + 1
            continue
        j = 0
        q += op in "=Xi"
        r += op in "=XDd"
    assert (q, r) == (len(query), rlen)
    return ins


def _depth(row):
    return sum(int(row[f]) for f in COL_FIELDS)


def py_call(cols, ins, frame, min_depth):
    """ioc_host_pileup_call, row by row: (sequence, qualities, {out_len, n_sub, n_del, n_ins, n_low})."""
    rlen = len(frame)
    assert len(cols) == len(ins) == rlen + 1 and min_depth >= 1
    seq, qual = bytearray(), bytearray()
    st = dict(out_len=0, n_sub=0, n_del=0, n_ins=0, n_low=0)
    for p in range(rlen + 1):
        D = _depth(cols[p]) if p < rlen else (_depth(cols[rlen - 1]) if rlen else 0)
        for s in range(SLOTS):
            slot = [int(v) for v in ins["slot"][p][s]]
            n = sum(slot)
            if not (D >= min_depth and 2 * n > D):
                break
            seq.append(LETTER[slot.index(max(slot))])
            qual.append(33 + min(40, 40 * max(slot) // D))
            st["n_ins"] += 1
        if p == rlen:
            break
        d = _depth(cols[p])
        if d < min_depth:
            seq.append(frame[p])
            qual.append(33)
            st["n_low"] += 1
            continue
        cnt = [int(cols[p][f]) for f in COL_FIELDS]
        m = max(cnt)
        fch = CH.get(frame[p], 4)
        who = fch if cnt[fch] == m else cnt.index(m)
        if who == 5:
            st["n_del"] += 1
            continue
        if who == fch:
            seq.append(frame[p])
        else:
            seq.append(LETTER[who])
            st["n_sub"] += 1
        qual.append(33 + min(40, 40 * m // d))
    st["out_len"] = len(seq)
    return bytes(seq), bytes(qual), st


def table(rows):
    """cols from rows of (a, c, g, t, other, del)."""
    t = np.zeros(len(rows), api.PILEUP_DTYPE)
    for p, r in enumerate(rows):
        for f, v in zip(COL_FIELDS, r):
            t[f][p] = v
    return t


def ins_table(n_rows, slots):
    """ins from {(row, slot): (a, c, g, t, other)}; the ins_runs / ins_bases of cols are not read by the call."""
    t = np.zeros(n_rows, api.PILEUP_INS_DTYPE)
    for (p, s), v in slots.items():
        t["slot"][p, s] = v
    return t


def q(*vals):
    return bytes(33 + v for v in vals)


Z = (0, 0, 0, 0, 0, 0)
# (name, frame, rows of cols, {(row, slot): counts}, min_depth, sequence, qualities, (n_sub, n_del, n_ins, n_low)), every expected
# value worked out by hand from the rules in include/isonclust2_hip.h
HAND_CALLS = [
    ("tie_frame_wins", b"G", [(2, 0, 2, 0, 0, 0), Z], {}, 1, b"G", q(20), (0, 0, 0, 0)),
    ("tie_frame_wins_over_del", b"T", [(0, 0, 0, 2, 0, 2), Z], {}, 1, b"T", q(20), (0, 0, 0, 0)),
    ("tie_without_frame_first_in_order", b"T", [(0, 2, 2, 1, 0, 0), Z], {}, 1, b"C", q(16), (1, 0, 0, 0)),
    ("tie_other_before_del", b"A", [(0, 0, 0, 0, 3, 3), Z], {}, 1, b"N", q(20), (1, 0, 0, 0)),
    ("del_wins", b"ACA", [(4, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 3), (4, 0, 0, 0, 0, 0), Z], {}, 1, b"AA", q(40, 40), (0, 1, 0, 0)),
    ("frame_other_kept_as_it_is", b"r", [(1, 0, 0, 0, 2, 0), Z], {}, 1, b"r", q(26), (0, 0, 0, 0)),
    # 2n == D: no insertion; 2n == D + 1: insertion
    ("two_n_equals_d", b"A", [(4, 0, 0, 0, 0, 0), Z], {(0, 0): (0, 2, 0, 0, 0)}, 1, b"A", q(40), (0, 0, 0, 0)),
    ("two_n_equals_d_plus_1", b"A", [(5, 0, 0, 0, 0, 0), Z], {(0, 0): (0, 2, 1, 0, 0)}, 1, b"CA", q(16, 40), (0, 0, 1, 0)),
    # slot 1 fails (2 * 2 == 4), slot 2 would pass: the row stops at slot 1
    ("slots_stop_at_first_failure", b"A", [(4, 0, 0, 0, 0, 0), Z], {(0, 0): (0, 0, 0, 3, 0), (0, 1): (2, 0, 0, 0, 0), (0, 2): (0, 0, 4, 0, 0)}, 1,
     b"TA", q(30, 40), (0, 0, 1, 0)),
    ("six_slots", b"C", [(0, 3, 0, 0, 0, 0), Z], {(0, s): (0, 0, 0, 0, 3) for s in range(6)}, 1, b"NNNNNNC", q(40, 40, 40, 40, 40, 40, 40), (0, 0, 6, 0)),
    # row rlen is held against depth(rlen - 1) = 4: 3 of 4 insert behind the last base
    ("row_rlen_uses_depth_before", b"AC", [(9, 0, 0, 0, 0, 0), (0, 4, 0, 0, 0, 0), Z], {(2, 0): (0, 0, 3, 0, 0), (2, 1): (2, 0, 0, 0, 0)}, 1,
     b"ACG", q(40, 40, 30), (0, 0, 1, 0)),
    ("rlen_0", b"", [Z], {(0, 0): (5, 0, 0, 0, 0)}, 1, b"", b"", (0, 0, 0, 0)),
    # counts of 2^32 - 1: depth 3 * (2^32 - 1), quality 40 / 3 = 13; the insertion's n = 2 * (2^32 - 1) > D / 2, quality 13
    ("counts_2_32", b"C", [(M32, M32, 0, 0, 0, M32), Z], {(0, 0): (0, 0, M32, M32, 0)}, 3, b"GC", q(13, 13), (0, 0, 1, 0)),
    ("counts_2_32_every_channel", b"T", [(M32,) * 6, Z], {}, 1, b"T", q(6), (0, 0, 0, 0)),
    # n > D: 40 * 7 / 2 clamps at 40
    ("n_above_d_clamps", b"A", [(2, 0, 0, 0, 0, 0), Z], {(0, 0): (0, 0, 0, 7, 0)}, 1, b"TA", q(40, 40), (0, 0, 1, 0)),
    # the same table under min_depth 1 and 3: depth 2 is called or kept as it is
    ("min_depth_1", b"AG", [(0, 2, 0, 0, 0, 0), (0, 0, 3, 0, 0, 0), Z], {(0, 0): (0, 0, 0, 2, 0)}, 1, b"TCG", q(40, 40, 40), (1, 0, 1, 0)),
    ("min_depth_3", b"AG", [(0, 2, 0, 0, 0, 0), (0, 0, 3, 0, 0, 0), Z], {(0, 0): (0, 0, 0, 2, 0)}, 3, b"AG", q(0, 40), (0, 0, 0, 1)),
]


def hand_case(case):
    name, frame, rows, slots, md, seq, qual, (n_sub, n_del, n_ins, n_low) = case
    st = dict(out_len=len(seq), n_sub=n_sub, n_del=n_del, n_ins=n_ins, n_low=n_low)
    return frame, table(rows), ins_table(len(rows), slots), md, seq, qual, st


def gap_open(e):
    return _lib.load().ioc_host_gap_open(e)


def host_tables(frame, reads, e=0.1):
    """Both host pileups of `reads` on `frame` through the host aligner: (cols, ins, [operation strings])."""
    cols, ins, strings = np.zeros(len(frame) + 1, api.PILEUP_DTYPE), np.zeros(len(frame) + 1, api.PILEUP_INS_DTYPE), []
    for rd in reads:
        ops, _ = api.host_align_ops(rd, frame, gap_open=gap_open(e))
        api.ops_pileup(ops, rd, len(frame), cols=cols)
        api.ops_pileup_ins(ops, rd, len(frame), ins=ins)
        strings.append(ops)
    return cols, ins, strings


def anchor():
    """The closed-form case: T, 300 random bases; the representative is T with one substitution (at 60), a deletion of 2 bases
    (T[140:142] missing) and an insertion of 1 base (in front of T[220]), every edit at least 50 bases from the ends and from each
    other.  Five identical reads equal to T vote unanimously at every column, so whichever of the equally good places the aligner
    gives a gap, the call is T itself.  Returns (T, representative)."""
    rng = random.Random(300)
    T = bytes(rng.choice(b"ACGT") for _ in range(300))
    rep = bytearray(T[:140] + T[142:220] + bytes([next(b for b in b"ACGT" if b not in (T[219], T[220]))]) + T[220:])
    rep[60] = next(b for b in b"ACGT" if b != T[60])
    return T, bytes(rep)


def mutate(rng, s, rate):
    out = bytearray()
    for b in s:
        u = rng.random()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            out.append(rng.choice(b"ACGT"))
        out.append(rng.choice(b"ACGT") if u > 1 - rate / 3 else b)
    return bytes(out)


def noisy(n_reads=15, length=400, rate=0.06, seed=11):
    """(T, a representative damaged at 2 * rate, n_reads reads mutated independently at `rate`)."""
    rng = random.Random(seed)
    T = bytes(rng.choice(b"ACGT") for _ in range(length))
    return T, mutate(rng, T, 2 * rate), [mutate(rng, T, rate) for _ in range(n_reads)]


def distance(a, b):
    """mismatches + ins + del of the host alignment of a against b."""
    st = api.ops_stats(api.host_align_ops(a, b, gap_open=gap_open(0.1))[0])
    return st["mismatches"] + st["ins"] + st["del"]


def random_tables(rng, n_rows, values=(0, 1, 2, 3, 2**31, M32), p_zero_ins=0.5):
    """Tables no aligner would produce: every counter drawn from `values`."""
    cols = np.zeros(n_rows, api.PILEUP_DTYPE)
    ins = np.zeros(n_rows, api.PILEUP_INS_DTYPE)
    for f in api.PILEUP_FIELDS:
        cols[f] = rng.choice(values, n_rows)
    slot = rng.choice(values, (n_rows, SLOTS, 5))
    slot[rng.random((n_rows, SLOTS)) < p_zero_ins] = 0
    ins["slot"] = slot
    ins["longer"] = rng.choice(values, n_rows)
    return cols, ins
