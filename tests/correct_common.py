"""What the tests of the read correction share (test_read_correct_host.py, test_gpu_planes_correct.py, test_gpu_align_correct.py,
test_cli_correct.py): a plain-Python restatement of ioc_host_read_correct — row by row, the runs measured end to end, in Python's
unbounded integers — which is the independent witness for the host function and, through it, for k_read_correct; tables and
planes spelled out by hand with the output they must give; and the builders of the property case (two haplotypes and an isoform
that lacks 40 bases) and of the planted shapes of the GPU test."""
import random

import numpy as np

from isonclust2_amd import api
from tests import polish_common as pc
from tests import sites_common as sc

SLOTS, NONE, DEL = 6, 7, 5
LETTER = b"ACGTN"
FIELDS = ("out_len", "n_sub", "n_fill", "n_remove", "n_ins_add", "n_ins_drop", "n_low", "n_guarded")
DEFAULT = dict(min_depth=3, min_alt=3, min_pct=25, max_run=10)


def _need(D, min_alt, min_pct):
    return max(min_alt, (min_pct * D + 99) // 100)


def py_decisions(base, cols, frame, min_depth=3, min_alt=3, min_pct=25):
    """The rows' decisions before the run guard: None (not covered, and row rlen), or (kind, winner)."""
    rlen = len(frame)
    cnt = [[int(cols[f][p]) for f in pc.COL_FIELDS] for p in range(rlen + 1)]
    dec = [None] * (rlen + 1)
    for p in range(rlen):
        own, depth = int(base[p]), sum(cnt[p])
        if not 0 <= own <= DEL:
            continue
        if depth < min_depth:
            dec[p] = ("low", None)
        elif cnt[p][own] >= _need(depth, min_alt, min_pct):
            dec[p] = ("keep", None)
        else:
            m = max(cnt[p])
            fch = pc.CH.get(frame[p], 4)
            w = fch if cnt[p][fch] == m else cnt[p].index(m)
            dec[p] = ("keep", None) if w == own else ("fill", w) if own == DEL else ("remove", None) if w == DEL else ("sub", w)
    return dec


def runs(dec, kind):
    """The maximal runs of `kind` among the decisions: [(first row, rows)]."""
    out, p = [], 0
    while p < len(dec):
        e = p
        while e < len(dec) and dec[e] and dec[e][0] == kind:
            e += 1
        if e > p:
            out.append((p, e - p))
        p = max(e, p + 1)
    return out


def py_correct(base, slots, cols, ins, frame, min_depth=3, min_alt=3, min_pct=25, max_run=10):
    """ioc_host_read_correct: (sequence, qualities, {FIELDS})."""
    rlen = len(frame)
    assert len(base) == len(cols) == len(ins) == rlen + 1 and np.shape(slots) == (SLOTS, rlen + 1)
    cnt = [[int(cols[f][p]) for f in pc.COL_FIELDS] for p in range(rlen + 1)]
    depth = [sum(c) for c in cnt]
    covers = lambda b: 0 <= int(b) <= DEL
    # 1. the rows' decisions
    dec = py_decisions(base, cols, frame, min_depth, min_alt, min_pct)
    # 2. the run guard
    st = dict.fromkeys(FIELDS, 0)
    p = 0
    while p < rlen:
        kind = dec[p][0] if dec[p] else None
        e = p + 1
        if kind in ("fill", "remove"):
            while e < rlen and dec[e] and dec[e][0] == kind:
                e += 1
            if e - p > max_run:
                for x in range(p, e):
                    dec[x] = ("keep", None)
                st["n_guarded"] += e - p
        p = e
    # 3. emission
    seq, qual = bytearray(), bytearray()

    def put(ch, q):
        seq.append(LETTER[ch])
        qual.append(33 + min(40, q))

    for p in range(rlen + 1):
        pi = p if p < rlen else rlen - 1
        if pi >= 0 and covers(base[pi]):
            D = depth[pi]
            own_slots = [int(slots[j][p]) if 1 <= int(slots[j][p]) <= 5 else 0 for j in range(SLOTS)]
            if D < min_depth:
                for s in own_slots:
                    if s:
                        put(s - 1, 0)
            else:
                need, cons = _need(D, min_alt, min_pct), True
                for j, s in enumerate(own_slots):
                    slot = [int(v) for v in ins["slot"][p][j]]
                    n = sum(slot)
                    cons = cons and 2 * n > D
                    who = slot.index(max(slot))
                    if s and slot[s - 1] >= need:
                        put(s - 1, 40 * slot[s - 1] // D)
                    elif s and cons:
                        put(who, 40 * slot[who] // D)
                        st["n_sub"] += 1
                    elif s:
                        st["n_ins_drop"] += 1
                    elif cons and max(D - n, 0) < need:
                        put(who, 40 * slot[who] // D)
                        st["n_ins_add"] += 1
        if dec[p] is None:
            continue
        kind, w = dec[p]
        own = int(base[p])
        if kind == "low":
            st["n_low"] += 1
            if own != DEL:
                put(own, 0)
        elif kind == "remove":
            st["n_remove"] += 1
        else:
            ch = own if kind == "keep" else w
            st["n_sub"] += kind == "sub"
            st["n_fill"] += kind == "fill"
            if ch != DEL:
                put(ch, 40 * cnt[p][ch] // depth[p])
    st["out_len"] = len(seq)
    return bytes(seq), bytes(qual), st


def slots_of(rows, own=None):
    """The slot planes of a read of `rows` rows from {(row, slot): byte}."""
    s = np.zeros((SLOTS, rows), np.uint8)
    for (p, j), v in (own or {}).items():
        s[j, p] = v
    return s


q = pc.q
Z = pc.Z
A10 = (10, 0, 0, 0, 0, 0)
# (name, frame, base plane, {(row, slot): own byte}, rows of cols, {(row, slot): counts}, rule overrides, sequence, qualities,
#  {the record's non-zero counters}), every expected value worked out by hand from the rules in include/isonclust2_hip.h;
#  need(D) = max(min_alt, ceil(min_pct * D / 100)): 3 at D = 10 and 25 %, 5 at D = 20, 6 at D = 21
HAND = [
    # own C with 3 of 10: kept, quality 40 * 3 / 10; with 2 of 10: the winner A, 40 * 8 / 10
    ("need_by_min_alt_at_equality", b"A", [1, NONE], {}, [(7, 3, 0, 0, 0, 0), Z], {}, {}, b"C", q(12), {}),
    ("need_by_min_alt_one_below", b"A", [1, NONE], {}, [(8, 2, 0, 0, 0, 0), Z], {}, {}, b"A", q(32), {"n_sub": 1}),
    ("need_by_min_pct_at_equality", b"A", [1, NONE], {}, [(15, 5, 0, 0, 0, 0), Z], {}, {}, b"C", q(10), {}),
    ("need_by_min_pct_one_below", b"A", [1, NONE], {}, [(17, 4, 0, 0, 0, 0), Z], {}, {}, b"A", q(32), {"n_sub": 1}),
    # A and G tie at 4, own C has 2: the frame G wins the tie; without the frame among the largest, the first (A)
    ("winner_tie_goes_to_frame", b"G", [1, NONE], {}, [(4, 2, 4, 0, 0, 0), Z], {}, {}, b"G", q(16), {"n_sub": 1}),
    ("winner_tie_first_in_order", b"T", [1, NONE], {}, [(4, 2, 4, 0, 0, 0), Z], {}, {}, b"A", q(16), {"n_sub": 1}),
    # own A has 2 of 9, below need 3, but nothing has more: kept, and written by channel (the frame's lower case is not)
    ("own_is_winner_although_unsupported", b"a", [4, NONE], {}, [(1, 2, 2, 2, 2, 0), Z], {}, {"min_depth": 1}, b"N", q(8), {}),
    # depth 2 < 3: the read's own, quality 0; a deletion stays one; the insertion is its own too
    ("low_depth", b"AC", [2, DEL, NONE], {(0, 0): 4, (0, 1): 9, (0, 2): 1}, [(0, 0, 2, 0, 0, 0), (0, 0, 0, 0, 0, 2), Z], {}, {}, b"TAG", q(0, 0, 0),
     {"n_low": 2}),
    # deletions at rows 1, 2 of a read against 10 x the base: filled (run 2 <= 2), and left (run 2 > 1)
    ("fill_run_at_max_run", b"ACGT", [0, DEL, DEL, 3, NONE], {}, [A10, (0, 10, 0, 0, 0, 0), (0, 0, 10, 0, 0, 0), (0, 0, 0, 10, 0, 0), Z], {},
     {"max_run": 2}, b"ACGT", q(40, 40, 40, 40), {"n_fill": 2}),
    ("fill_run_above_max_run", b"ACGT", [0, DEL, DEL, 3, NONE], {}, [A10, (0, 10, 0, 0, 0, 0), (0, 0, 10, 0, 0, 0), (0, 0, 0, 10, 0, 0), Z], {},
     {"max_run": 1}, b"AT", q(40, 40), {"n_guarded": 2}),
    # bases at rows 1, 2 that 9 of 10 delete: removed, and left at their own support 1 of 10
    ("remove_run_at_max_run", b"ACGT", [0, 1, 2, 3, NONE], {}, [A10, (0, 1, 0, 0, 0, 9), (0, 0, 1, 0, 0, 9), (0, 0, 0, 10, 0, 0), Z], {},
     {"max_run": 2}, b"AT", q(40, 40), {"n_remove": 2}),
    ("remove_run_above_max_run", b"ACGT", [0, 1, 2, 3, NONE], {}, [A10, (0, 1, 0, 0, 0, 9), (0, 0, 1, 0, 0, 9), (0, 0, 0, 10, 0, 0), Z], {},
     {"max_run": 1}, b"ACGT", q(40, 4, 4, 40), {"n_guarded": 2}),
    # a fill and a remove side by side are two runs of 1; a sub is never guarded
    ("fill_and_remove_are_guarded_apart", b"AC", [DEL, 1, NONE], {}, [A10, (0, 1, 0, 0, 0, 9), Z], {}, {"max_run": 1}, b"A", q(40),
     {"n_fill": 1, "n_remove": 1}),
    ("max_run_0", b"ACG", [DEL, 1, 3, NONE], {}, [A10, (0, 1, 0, 0, 0, 9), (0, 0, 9, 1, 0, 0), Z], {}, {"max_run": 0}, b"CG", q(4, 36),
     {"n_guarded": 2, "n_sub": 1}),
    # an uncovered row between two fills: two runs of 1
    ("run_ended_by_uncovered_row", b"AAA", [DEL, NONE, DEL, NONE], {}, [A10, A10, A10, Z], {}, {"max_run": 1}, b"AA", q(40, 40), {"n_fill": 2}),
    ("run_not_ended", b"AAA", [DEL, DEL, DEL, NONE], {}, [A10, A10, A10, Z], {}, {"max_run": 2}, b"", b"", {"n_guarded": 3}),
    # the slot rule, D = 10, need 3.  own G with 3: kept at 12
    ("slot_own_supported", b"A", [0, NONE], {(0, 0): 3}, [A10, Z], {(0, 0): (0, 0, 3, 0, 0)}, {}, b"GA", q(12, 40), {}),
    # own G with 2 where 6 of 10 insert (T 4): the slot's letter T at 16; where only 5 do: dropped
    ("slot_own_unsupported_consensus", b"A", [0, NONE], {(0, 0): 3}, [A10, Z], {(0, 0): (0, 0, 2, 4, 0)}, {}, b"TA", q(16, 40), {"n_sub": 1}),
    ("slot_own_unsupported_dropped", b"A", [0, NONE], {(0, 0): 3}, [A10, Z], {(0, 0): (0, 0, 2, 3, 0)}, {}, b"A", q(40), {"n_ins_drop": 1}),
    # nothing of its own where 8 of 10 insert C: 10 - 8 = 2 < 3, added at 32; where 7 do, 3 reads without are an allele: not added
    ("slot_added", b"A", [0, NONE], {}, [A10, Z], {(0, 0): (0, 8, 0, 0, 0)}, {}, b"CA", q(32, 40), {"n_ins_add": 1}),
    ("slot_not_added_absence_supported", b"A", [0, NONE], {}, [A10, Z], {(0, 0): (0, 7, 0, 0, 0)}, {}, b"A", q(40), {}),
    # slot 0 has 8, slot 1 only 5 (2 * 5 == 10 stops the prefix), slot 2 has 9: own T at slot 2 with 2 is dropped, slot 2 not added
    ("prefix_rule_stops_at_a_slot", b"A", [0, NONE], {(0, 2): 4}, [A10, Z], {(0, 0): (8, 0, 0, 0, 0), (0, 1): (5, 0, 0, 0, 0), (0, 2): (7, 0, 0, 2, 0)}, {},
     b"AA", q(32, 40), {"n_ins_add": 1, "n_ins_drop": 1}),
    # row rlen = 1 is held against depth(0) = 4 and spans where row 0 is covered: 3 of 4 insert G, 4 - 3 = 1 < 3: added at 30
    ("row_rlen_uses_depth_before", b"A", [0, NONE], {}, [(4, 0, 0, 0, 0, 0), Z], {(1, 0): (0, 0, 3, 0, 0)}, {}, b"AG", q(40, 30), {"n_ins_add": 1}),
    ("row_rlen_not_spanned", b"A", [NONE, NONE], {(1, 0): 1}, [(4, 0, 0, 0, 0, 0), Z], {(1, 0): (0, 0, 3, 0, 0)}, {}, b"", b"", {}),
    ("rlen_0", b"", [NONE], {(0, 0): 1}, [Z], {(0, 0): (5, 0, 0, 0, 0)}, {}, b"", b"", {}),
    ("covers_nothing", b"AC", [NONE, NONE, NONE], {(0, 0): 2, (1, 0): 2, (2, 0): 2}, [A10, A10, Z], {(1, 0): (0, 9, 0, 0, 0)}, {}, b"", b"", {}),
    # bytes neither projection writes: base 6 and 200 are "not covered" (row 1's insertion is not spanned), slot byte 6 is none
    ("illegal_plane_bytes", b"AAA", [6, 200, 0, NONE], {(1, 0): 2, (2, 0): 6, (2, 1): 255}, [A10, A10, A10, Z], {}, {}, b"A", q(40), {}),
]


def hand_case(case):
    name, frame, base, own, rows, slot_counts, rule, seq, qual, counters = case
    st = dict.fromkeys(FIELDS, 0)
    st.update(counters, out_len=len(seq))
    return (frame, np.array(base, np.uint8), slots_of(len(base), own), pc.table(rows), pc.ins_table(len(rows), slot_counts), {**DEFAULT, **rule}, seq, qual, st)


def random_case(rng, rlen, values=(0, 1, 2, 3, 5, 9), p_bad=0.02):
    """(frame, base, slots, cols, ins) no aligner would produce: small counters, so that every branch of the rule is taken, runs
    of deletions and of covered rows, up to two stretches of up to 150 rows that most reads fill or most reads delete (runs of one
    decision that cross the 64-row steps), a few bytes outside the legal set."""
    frame = bytes(rng.choice(list(b"ACGTN")) for _ in range(rlen))
    cols, ins = pc.random_tables(rng, rlen + 1, values=values, p_zero_ins=0.4)
    base = np.full(rlen + 1, NONE, np.uint8)
    p = 0
    while p < rlen:
        n = int(rng.integers(1, 30))
        kind = rng.integers(0, 4)
        base[p:min(p + n, rlen)] = NONE if kind == 0 else DEL if kind == 1 else rng.integers(0, 5, min(p + n, rlen) - p)
        p += n
    for _ in range(int(rng.integers(0, 3))):   # stretches of one table row and one read byte: long runs of one decision
        a = int(rng.integers(0, rlen + 1))
        e = min(a + int(rng.integers(5, 150)), rlen)
        fill = rng.random() < 0.5
        for f in pc.COL_FIELDS:
            cols[f][a:e] = 0
        cols["a"][a:e], cols["del"][a:e] = (9, 0) if fill else (1, 9)
        base[a:e] = DEL if fill else 0
    slots = np.where(rng.random((SLOTS, rlen + 1)) < 0.3, rng.integers(1, 6, (SLOTS, rlen + 1)), 0).astype(np.uint8)
    bad = rng.random(rlen + 1) < p_bad
    base[bad] = rng.choice([6, 8, 200, 255], int(bad.sum()))
    slots[rng.random((SLOTS, rlen + 1)) < p_bad] = 6
    return frame, base, slots, cols, ins


# ---- the property case ----
CUT = (150, 190)  # the bases of T the isoform lacks
# The seed of the property case: the first of 0, 1, 2, .. at which every noisy B read carries B's allele at every site of
# sites_common.SITES_ON_T before anything is corrected (one seed in a few hundred: 75 (read, site) pairs at 8 % errors) — chosen on
# the host aligner and the host projection alone.  A read whose own copy of a site is a sequencing error has no allele to keep.
SEED = 1638


def shows_b_alleles(seq, T, B):
    """`seq` aligned against T by the host aligner shows B's allele at every site of SITES_ON_T: B's base at 40, the deletion of
    T[120:123], the insertion in front of T[200]."""
    ops = api.host_align_ops(seq, T, gap_open=pc.gap_open(0.1))[0]
    base, insf = api.ops_project(ops, seq, len(T))
    want = {(40, sc.BASE): pc.CH[B[40]], (120, sc.BASE): DEL, (121, sc.BASE): DEL, (122, sc.BASE): DEL, (200, sc.INS): 1}
    assert sorted(want) == sorted(sc.SITES_ON_T)
    return all((int(base[row]) if kind == sc.BASE else int(insf[row])) == allele for (row, kind), allele in want.items())


def isoform_case(seed, rate=0.08):
    """(T, reads, truths): sites_common.noisy_haplotypes' 20 reads of T and 15 of its haplotype B, and two reads of T without
    T[150:190], all mutated independently at `rate`; truths[i] is what read i was mutated from."""
    T, B, _ = sc.haplotypes()
    _, reads = sc.noisy_haplotypes(seed, rate)
    rng = random.Random(seed + 1000)
    iso = T[:CUT[0]] + T[CUT[1]:]
    return T, reads + [pc.mutate(rng, iso, rate) for _ in range(2)], [T] * 20 + [B] * 15 + [iso] * 2


def host_planes(frame, reads, e=0.1):
    """Through the host aligner and the host projections: (cols, ins, [base plane per read], [slot planes per read], [ops]), the
    tables added up from the planes (ioc_host_planes_pile)."""
    cols, ins = np.zeros(len(frame) + 1, api.PILEUP_DTYPE), np.zeros(len(frame) + 1, api.PILEUP_INS_DTYPE)
    bases, slots, strings = [], [], []
    for rd in reads:
        ops, _ = api.host_align_ops(rd, frame, gap_open=pc.gap_open(e))
        bases.append(api.ops_project(ops, rd, len(frame))[0])
        slots.append(api.ops_project_ins(ops, rd, len(frame)))
        api.planes_pile(bases[-1], slots[-1], cols=cols, ins=ins)
        strings.append(ops)
    return cols, ins, bases, slots, strings


def host_correct_all(frame, reads, e=0.1, **rule):
    """Every read corrected by the host definition: ([sequence], [qualities], [record], (cols, ins, bases, slots, ops))."""
    laid = host_planes(frame, reads, e)
    cols, ins, bases, slots, _ = laid
    out = [api.read_correct(b, s, cols, ins, frame, **{**DEFAULT, **rule}) for b, s in zip(bases, slots)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], laid


def aligned_part(read, ops):
    """The bases of `read` between its free end gaps (what a correction replaces)."""
    st = api.ops_stats(ops)
    return read[st["lead_i"]:len(read) - st["trail_i"]]


# ---- the planted shapes of the GPU test (tests/test_gpu_planes_correct.py) ----
# (rlen, pairs): the lengths around the 64 rows of a wave's step, the pair counts around the four waves of a workgroup
SHAPES = [(0, 1), (1, 3), (63, 4), (64, 5), (65, 0), (127, 130), (128, 3), (129, 5), (600, 130)]
# rows that most reads delete, by segment length — (first row, rows): a read with bases there is a run of "remove" as long: runs of
# 10, 11, 64, 65 and 130 rows, starts at rows 0, 62, 63, 64 and 127, ends at row rlen - 1, and 130 rows that span a whole step of a
# wave (rows 320 .. 383) and both its neighbours
DEL_REGIONS = {127: [(0, 10), (62, 65)], 128: [(0, 11), (63, 64)], 129: [(64, 10), (127, 2)], 600: [(300, 130), (536, 64)]}
# where a read's own deletions are planted, runs of "fill", by segment length: the same lengths and starts, ends at row rlen - 1
# (the short segments), and two runs of 130 rows that span whole steps (rows 64 .. 127, 128 .. 191) and their neighbours.  No row
# under any of them is of low depth or in a region above — either would end the run
FILL_RUNS = {63: [(53, 10)], 64: [(54, 10), (53, 11), (0, 64)], 127: [(20, 10), (35, 11)],
             600: [(0, 10), (0, 11), (0, 64), (62, 10), (62, 11), (62, 130), (63, 64), (63, 65), (64, 64), (64, 65), (127, 10), (127, 130)]}
RUN_LENGTHS, RUN_STARTS = {10, 11, 64, 65, 130}, {0, 62, 63, 64, 127}


def planted_case(seed=12):
    """(frames, cols, ins, seg_of_pair, base planes, slot planes) of SHAPES, the segments' pairs interleaved.  The tables say "the
    frame, 10 deep" except in DEL_REGIONS (9 of 10 delete), at rows of depth 2 (none under a planted run), at rows with a second
    allele of 3 or of 2 reads, and have insertions most reads share in front of row 0, of row rlen and of a few others.  A read
    follows the frame with a few bases of its own, covers all or a part, has one to three FILL_RUNS of deletions — each between
    two bases, none touching another — and insertions of its own; a segment's first read is the frame itself from end to end."""
    rng = random.Random(seed)
    frames, tables, pairs = [], [], []
    for g, (rlen, count) in enumerate(SHAPES):
        frame = bytes(rng.choice(b"ACGTN") for _ in range(rlen))
        fch = [pc.CH.get(b, 4) for b in frame]
        fits = FILL_RUNS.get(rlen, [])
        planted = {p for a, n in fits for p in range(a, a + n)}
        rows, slot_counts = [], {}
        for p in range(rlen):
            r = [0] * 6
            u = rng.random()
            if u < 0.04 and p not in planted:
                r[fch[p]] = 2                                     # low depth
            elif u < 0.10:
                r[fch[p]], r[(fch[p] + 1) % 5] = 7, 3             # a second allele at need
            elif u < 0.16:
                r[fch[p]], r[(fch[p] + 2) % 5] = 8, 2             # ... and one below
            else:
                r[fch[p]] = 10
            rows.append(r)
        for first, n in DEL_REGIONS.get(rlen, []):
            assert not planted & set(range(first, first + n))
            for p in range(first, first + n):
                rows[p] = [0] * 6
                rows[p][fch[p]], rows[p][DEL] = 1, 9
        rows.append([0] * 6)
        for p in sorted({0, rlen} | {rng.randrange(rlen + 1) for _ in range(rlen // 12)}):
            for j in range(rng.choice((1, 1, 2, 6))):
                slot_counts[(p, j)] = rng.choice([(0, 8, 0, 0, 0), (0, 0, 7, 0, 0), (3, 0, 0, 5, 0), (0, 0, 0, 0, 9), (2, 3, 0, 0, 0)])
        frames.append(frame)
        tables.append((pc.table([tuple(r) for r in rows]), pc.ins_table(rlen + 1, slot_counts)))
        for k in range(count):
            base = np.full(rlen + 1, NONE, np.uint8)
            slots = np.zeros((SLOTS, rlen + 1), np.uint8)
            first, last = (0, rlen) if k < 4 or rng.random() < 0.7 else sorted((rng.randrange(rlen + 1), rng.randrange(rlen + 1)))
            for p in range(first, last):
                base[p] = rng.choice((0, 1, 2, 3, 4, DEL)) if k > 0 and rng.random() < 0.05 else fch[p]
            # read k's first run is FILL_RUNS' k-th, so that every one of them is some read's; then up to two more
            taken = []
            for a, n in ([fits[(k - 1) % len(fits)]] + rng.sample(fits, min(len(fits), rng.randrange(0, 3))) if fits and k > 0 else []):
                if a < first or a + n > last or any(a <= b + m and b <= a + n for b, m in taken):
                    continue
                taken.append((a, n))
                base[a:a + n] = DEL
                for edge in (a - 1, a + n):                       # (a base either side: the run is as long as planted)
                    if 0 <= edge < rlen and base[edge] == DEL:
                        base[edge] = fch[edge]
            for p in range(first, last + 1):
                if p in (0, rlen) and rng.random() < 0.5 or rng.random() < 0.1:
                    for j in range(rng.randrange(1, 7)):
                        slots[j, p] = rng.randrange(1, 6)
            pairs.append((g, base, slots))
    rng.shuffle(pairs)
    return (frames, np.concatenate([t[0] for t in tables]), np.concatenate([t[1] for t in tables]), [p[0] for p in pairs], [p[1] for p in pairs],
            [p[2] for p in pairs])


def planted_runs(case, kind):
    """The maximal runs of `kind` ("fill" / "remove") over every pair of a planted case, at the default thresholds: [(rlen, first
    row, rows)], a run per pair that has it."""
    frames, cols, ins, sop, base, slots = case
    row0 = np.concatenate([[0], np.cumsum([len(f) + 1 for f in frames])]).astype(int)
    return [(len(frames[g]), a, n) for i, g in enumerate(sop) for a, n in runs(py_decisions(base[i], cols[row0[g]:row0[g + 1]], frames[g]), kind)]


def host_correct_planes(frames, cols, ins, seg_of_pair, base, slots, **rule):
    """ioc_host_read_correct pair by pair over the tables of many segments: ([sequence], [qualities], records as an array)."""
    row0 = np.concatenate([[0], np.cumsum([len(f) + 1 for f in frames])]).astype(int)
    seqs, quals, recs = [], [], np.zeros(len(base), api.CORRECT_STATS_DTYPE)
    for i, g in enumerate(seg_of_pair):
        rows = slice(row0[g], row0[g + 1])
        s, q_, st = api.read_correct(base[i], slots[i], cols[rows], ins[rows], frames[g], **{**DEFAULT, **rule})
        seqs.append(s), quals.append(q_)
        recs[i] = tuple(st[f] for f in FIELDS)
    return seqs, quals, recs
