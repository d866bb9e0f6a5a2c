"""What the tests of the quality-weighted pileup and call share (test_pile_weight_host.py, test_gpu_pile_call_weighted.py,
test_gpu_align_polish_weighted.py, test_cli_polish_weighted.py): a plain-Python restatement of the two definitions —
ioc_host_ops_pileup_weighted byte by byte, ioc_host_pileup_call_weighted row by row, in Python's unbounded integers (reduced
modulo 2^32 where the definition wraps) — as the independent witness; tables spelled out by hand with the output they must give;
and the closed-form case in which the weights, and not the counts, decide."""
import random

import numpy as np

from isonclust2_amd import api

from tests import polish_common as pc

SLOTS, CH, COL_FIELDS, LETTER, M32 = pc.SLOTS, pc.CH, pc.COL_FIELDS, pc.LETTER, pc.M32


def py_weight(b):
    """w(b): 1 for b <= 34, else min(b - 33, 93)."""
    return 1 if b <= 34 else min(b - 33, 93)


def py_pileup_weighted(ops, query, qual, rlen, wcols=None, wins=None):
    """The walk of ioc_host_ops_pileup_weighted, byte by byte; ADDS (modulo 2^32) to the tables given, else to zeros."""
    wcols = np.zeros(rlen + 1, api.PILEUP_DTYPE) if wcols is None else wcols
    wins = np.zeros(rlen + 1, api.PILEUP_INS_DTYPE) if wins is None else wins
    qlen = len(query)
    assert len(qual) == qlen
    r = q = j = 0

    def add(arr, idx, w):
        arr[idx] = (int(arr[idx]) + w) & M32

    for op in bytes(ops):
        op = chr(op)
        if op == "I":
            w = py_weight(qual[q])
            if j < SLOTS:
                add(wins["slot"], (r, j, CH.get(query[q], 4)), w)
            else:
                add(wins["longer"], r, w)
            j, q = j + 1, q + 1
            continue
        j = 0
        if op in "=X":
            add(wcols[COL_FIELDS[CH.get(query[q], 4)]], r, py_weight(qual[q]))
        elif op == "D":
            near = ([py_weight(qual[q - 1])] if q > 0 else []) + ([py_weight(qual[q])] if q < qlen else [])
            add(wcols["del"], r, min(near) if near else 1)
        q += op in "=Xi"
        r += op in "=XDd"
    assert (q, r) == (qlen, rlen)
    return wcols, wins


def _depth(row):
    return sum(int(row[f]) for f in COL_FIELDS)


def py_call_weighted(cols, wcols, wins, frame, min_depth):
    """ioc_host_pileup_call_weighted, row by row: (sequence, qualities, {out_len, n_sub, n_del, n_ins, n_low})."""
    rlen = len(frame)
    assert len(cols) == len(wcols) == len(wins) == rlen + 1 and min_depth >= 1
    seq, qual = bytearray(), bytearray()
    st = dict(out_len=0, n_sub=0, n_del=0, n_ins=0, n_low=0)
    for p in range(rlen + 1):
        at = p if p < rlen else rlen - 1
        Dc, Dw = (_depth(cols[at]), _depth(wcols[at])) if at >= 0 else (0, 0)
        for s in range(SLOTS):
            slot = [int(v) for v in wins["slot"][p][s]]
            n = sum(slot)
            if not (Dc >= min_depth and Dw > 0 and 2 * n > Dw):
                break
            seq.append(LETTER[slot.index(max(slot))])
            qual.append(33 + min(40, 40 * max(slot) // Dw))
            st["n_ins"] += 1
        if p == rlen:
            break
        if Dc < min_depth or Dw == 0:
            seq.append(frame[p])
            qual.append(33)
            st["n_low"] += 1
            continue
        wt = [int(wcols[p][f]) for f in COL_FIELDS]
        m = max(wt)
        fch = CH.get(frame[p], 4)
        who = fch if wt[fch] == m else wt.index(m)
        if who == 5:
            st["n_del"] += 1
            continue
        if who == fch:
            seq.append(frame[p])
        else:
            seq.append(LETTER[who])
            st["n_sub"] += 1
        qual.append(33 + min(40, 40 * m // Dw))
    st["out_len"] = len(seq)
    return bytes(seq), bytes(qual), st


Z = pc.Z
q = pc.q
# (name, frame, rows of cols, rows of wcols, {(row, slot): weights}, min_depth, sequence, qualities, (n_sub, n_del, n_ins, n_low)),
# every expected value worked out by hand from the rules in include/isonclust2_hip.h
HAND_CALLS_W = [
    # three reads say C (weight 2 each), two say A, the frame (40 each): 40 * 80 / 86 = 37
    ("counts_sub_weights_frame", b"A", [(2, 3, 0, 0, 0, 0), Z], [(80, 6, 0, 0, 0, 0), Z], {}, 3, b"A", q(37), (0, 0, 0, 0)),
    # ... and the other way round: the weights call the substitution the counts would not
    ("counts_frame_weights_sub", b"A", [(3, 2, 0, 0, 0, 0), Z], [(6, 80, 0, 0, 0, 0), Z], {}, 3, b"C", q(37), (1, 0, 0, 0)),
    ("weight_tie_frame_wins", b"G", [(3, 0, 1, 0, 0, 0), Z], [(30, 0, 30, 0, 0, 0), Z], {}, 1, b"G", q(20), (0, 0, 0, 0)),
    ("weight_tie_frame_wins_over_del", b"T", [(0, 0, 0, 1, 0, 5), Z], [(0, 0, 0, 7, 0, 7), Z], {}, 1, b"T", q(20), (0, 0, 0, 0)),
    ("weight_tie_without_frame_first_in_order", b"T", [(0, 1, 1, 1, 0, 0), Z], [(0, 9, 9, 2, 0, 0), Z], {}, 1, b"C", q(18), (1, 0, 0, 0)),
    ("del_wins_by_weight", b"ACA", [(4, 0, 0, 0, 0, 0), (0, 3, 0, 0, 0, 1), (4, 0, 0, 0, 0, 0), Z],
     [(160, 0, 0, 0, 0, 0), (0, 6, 0, 0, 0, 40), (160, 0, 0, 0, 0, 0), Z], {}, 1, b"AA", q(40, 40), (0, 1, 0, 0)),
    # Dc = 2 < 3 under heavy weights: kept as the frame has it; the insertion in front of it is not made either
    ("dc_below_min_depth_is_low", b"A", [(0, 2, 0, 0, 0, 0), Z], [(0, 186, 0, 0, 0, 0), Z], {(0, 0): (0, 0, 186, 0, 0)}, 3, b"A", q(0), (0, 0, 0, 1)),
    # Dw == 0 with Dc >= min_depth (tables that no pileup gives: every weight is at least 1): low, and no insertion
    ("dw_zero_is_low", b"C", [(0, 5, 0, 0, 0, 0), Z], [Z, Z], {(0, 0): (0, 0, 9, 0, 0)}, 3, b"C", q(0), (0, 0, 0, 1)),
    # 2n == Dw: no insertion; 2n == Dw + 1: insertion, quality 40 * 20 / 41 = 19
    ("two_n_equals_dw", b"A", [(4, 0, 0, 0, 0, 0), Z], [(40, 0, 0, 0, 0, 0), Z], {(0, 0): (0, 20, 0, 0, 0)}, 1, b"A", q(40), (0, 0, 0, 0)),
    ("two_n_equals_dw_plus_1", b"A", [(4, 0, 0, 0, 0, 0), Z], [(41, 0, 0, 0, 0, 0), Z], {(0, 0): (0, 20, 1, 0, 0)}, 1, b"CA", q(19, 40), (0, 0, 1, 0)),
    # slot 1 fails (2 * 20 == 40), slot 2 would pass: the row stops at slot 1
    ("slots_stop_at_first_failure", b"A", [(4, 0, 0, 0, 0, 0), Z], [(40, 0, 0, 0, 0, 0), Z],
     {(0, 0): (0, 0, 0, 30, 0), (0, 1): (20, 0, 0, 0, 0), (0, 2): (0, 0, 40, 0, 0)}, 1, b"TA", q(30, 40), (0, 0, 1, 0)),
    # row rlen is held against row rlen - 1 of BOTH tables: Dc = 4, Dw = 40, 30 of 40 insert behind the last base
    ("row_rlen_uses_row_before", b"AC", [(9, 0, 0, 0, 0, 0), (0, 4, 0, 0, 0, 0), Z], [(90, 0, 0, 0, 0, 0), (0, 40, 0, 0, 0, 0), Z],
     {(2, 0): (0, 0, 30, 0, 0), (2, 1): (20, 0, 0, 0, 0)}, 1, b"ACG", q(40, 40, 30), (0, 0, 1, 0)),
    # ... and its gate is the count of that row: Dc = 2 < 3, nothing behind the last base (which is low itself)
    ("row_rlen_gated_by_counts_before", b"AC", [(9, 0, 0, 0, 0, 0), (0, 2, 0, 0, 0, 0), Z], [(90, 0, 0, 0, 0, 0), (0, 40, 0, 0, 0, 0), Z],
     {(2, 0): (0, 0, 30, 0, 0)}, 3, b"AC", q(40, 0), (0, 0, 0, 1)),
    ("rlen_0", b"", [Z], [Z], {(0, 0): (5, 0, 0, 0, 0)}, 1, b"", b"", (0, 0, 0, 0)),
    # counters of 2^32 - 1 in every channel of both tables: quality 40 / 6 = 6; the slot's n = 2 (2^32 - 1) is not above Dw / 2
    ("counters_2_32_every_channel", b"T", [(M32,) * 6, Z], [(M32,) * 6, Z], {(0, 0): (0, 0, M32, M32, 0)}, 1, b"T", q(6), (0, 0, 0, 0)),
    # ... and with five of the slot's channels full: 2 * 5 > 6, the first maximal channel, quality 40 / 6
    ("counters_2_32_insertion", b"T", [(M32,) * 6, Z], [(M32,) * 6, Z], {(0, 0): (M32,) * 5}, 3, b"AT", q(6, 6), (0, 0, 1, 0)),
]


def hand_case_w(case):
    name, frame, rows, wrows, slots, md, seq, qual, (n_sub, n_del, n_ins, n_low) = case
    st = dict(out_len=len(seq), n_sub=n_sub, n_del=n_del, n_ins=n_ins, n_low=n_low)
    return frame, pc.table(rows), pc.table(wrows), pc.ins_table(len(rows), slots), md, seq, qual, st


def random_tables_w(rng, n_rows, values=(0, 1, 2, 3, 40, 93, 2**31, M32)):
    """All three tables with every counter drawn from `values`: (cols, wcols, wins)."""
    cols, _ = pc.random_tables(rng, n_rows, values=(0, 1, 2, 3, 2**31, M32))
    wcols, wins = pc.random_tables(rng, n_rows, values=values)
    return cols, wcols, wins


def host_tables_w(frame, reads, quals, e=0.1):
    """The count tables and the weight tables of `reads` on `frame` through the host aligner: (cols, ins, wcols, wins, strings)."""
    cols, ins, strings = pc.host_tables(frame, reads, e)
    wcols, wins = np.zeros(len(frame) + 1, api.PILEUP_DTYPE), np.zeros(len(frame) + 1, api.PILEUP_INS_DTYPE)
    for rd, ql, ops in zip(reads, quals, strings):
        api.ops_pileup_weighted(ops, rd, ql, len(frame), wcols=wcols, wins=wins)
    return cols, ins, wcols, wins, strings


def random_quals(rng, reads, lo=33, hi=126):
    """One random quality line per read, bytes lo .. hi (rng: a numpy Generator)."""
    return [rng.integers(lo, hi + 1, len(r)).astype(np.uint8).tobytes() for r in reads]


def closed_form(length=300, seed=300):
    """The case the feature is for.  T: `length` random bases, the frame.  Three reads carry the same substitution (at length / 3),
    the same deletion (of T[0.6 length]) and the same inserted base (in front of T[0.8 length]); T is drawn so that the deleted
    and the inserted base differ from both their neighbours, which makes the placement of each gap unique.  Those three reads
    have quality '#' (weight 2) on the five bases around each edit and 'I' (weight 40) elsewhere; two more reads equal T, 'I'
    throughout.  By count the edits win 3 : 2, by weight they lose 6 : 80 (the deletion, whose weight is the smaller of its
    neighbours': 6 : 80 as well).  Returns (T, the edited sequence, [5 reads], [5 quality lines])."""
    rng = random.Random(seed)
    sub, dele, insp = length // 3, (length * 3) // 5, (length * 4) // 5
    while True:
        T = bytes(rng.choice(b"ACGT") for _ in range(length))
        if T[dele] not in (T[dele - 1], T[dele + 1]) and T[insp - 1] != T[insp]:
            break
    new = next(b for b in b"ACGT" if b not in (T[insp - 1], T[insp]))
    edited = bytearray(T[:dele] + T[dele + 1:insp] + bytes([new]) + T[insp:])
    edited[sub] = next(b for b in b"ACGT" if b != T[sub])
    edited = bytes(edited)
    ql = bytearray(b"I" * len(edited))
    # positions in the edited read: the substitution, the two bases around the deletion, the inserted base (shifted by the deletion)
    for centre in (sub, dele, insp - 1):
        for x in range(centre - 2, centre + 3):
            ql[x] = ord("#")
    reads = [edited] * 3 + [T] * 2
    quals = [bytes(ql)] * 3 + [b"I" * length] * 2
    return T, edited, reads, quals
