"""What the tests of the read correction by isoform share (test_iso_correct_host.py, test_gpu_planes_correct_groups.py,
test_gpu_align_blocks_correct.py, test_cli_isoforms_correct.py): a plain-Python restatement of ioc_host_read_correct_long — the
decisions and the runs are correct_common's (py_decisions, runs), the emission is written out row by row with the long rows in it,
in Python's unbounded integers — and of the choice of the table a pair is held against, with the tables piled by
plane_pile_common.py_planes_pile; hand planes with long rows at the 64-row steps; and the builder of the GPU test's segments."""
import numpy as np

from isonclust2_amd import api
from tests import correct_common as cc
from tests import plane_pile_common as pp
from tests import polish_common as pc

SLOTS, NONE, DEL = cc.SLOTS, cc.NONE, cc.DEL
FIELDS = cc.FIELDS + ("table", "n_long_runs", "n_long_bases", "flags")
UNRESOLVED = 1
DEFAULT = cc.DEFAULT


def py_correct_long(base, slots, ilen, qpos, cols, ins, frame, query, min_depth=3, min_alt=3, min_pct=25, max_run=10):
    """ioc_host_read_correct_long: (sequence, qualities, {FIELDS}) — `table` is the batched calls' to set, 0 here."""
    rlen = len(frame)
    assert len(base) == len(cols) == len(ins) == len(ilen) == len(qpos) == rlen + 1 and np.shape(slots) == (SLOTS, rlen + 1)
    st = dict.fromkeys(FIELDS, 0)
    covers = lambda b: 0 <= int(b) <= DEL
    spans = lambda p: (p if p < rlen else rlen - 1) >= 0 and covers(base[p if p < rlen else rlen - 1])
    long_rows = [p for p in range(rlen + 1) if int(ilen[p]) > SLOTS]
    if any(int(v) == 255 for v in ilen) or any(int(qpos[p]) + int(ilen[p]) > len(query) or not spans(p) for p in long_rows) or \
            sum(int(ilen[p]) for p in long_rows) > len(query):   # (the last: runs that overlap, which the bound on cap rules out)
        st["flags"] = UNRESOLVED
        return b"", b"", st
    cnt = [[int(cols[f][p]) for f in pc.COL_FIELDS] for p in range(rlen + 1)]
    depth = [sum(c) for c in cnt]
    dec = cc.py_decisions(base, cols, frame, min_depth, min_alt, min_pct)
    for kind in ("fill", "remove"):   # the run guard: long rows neither start nor end a run
        for first, n in cc.runs(dec[:rlen], kind):
            if n > max_run:
                dec[first:first + n] = [("keep", None)] * n
                st["n_guarded"] += n
    seq, qual = bytearray(), bytearray()

    def put(ch, q):
        seq.append(cc.LETTER[ch])
        qual.append(33 + min(40, q))

    for p in range(rlen + 1):
        if p in long_rows:   # the run as the read has it, quality 0, whatever the depth; no slot rule
            a, n = int(qpos[p]), int(ilen[p])
            seq += query[a:a + n]
            qual += b"!" * n
            st["n_long_runs"] += 1
            st["n_long_bases"] += n
        elif spans(p):
            D = depth[p if p < rlen else rlen - 1]
            own = [int(slots[j][p]) if 1 <= int(slots[j][p]) <= 5 else 0 for j in range(SLOTS)]
            if D < min_depth:
                for s in own:
                    if s:
                        put(s - 1, 0)
            else:
                need, cons = cc._need(D, min_alt, min_pct), True
                for j, s in enumerate(own):
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


def py_tables_of(seg_of_pair, group, n_groups, min_depth):
    """Which table every pair is held against: (gseg_off, [table name per pair]) — gseg_off[g] + group where the pair's group has at
    least min_depth members, else -1 - segment."""
    ns = len(n_groups)
    gseg_off = [0]
    for g in range(ns):
        gseg_off.append(gseg_off[-1] + int(n_groups[g]))
    members = {}
    for g, h in zip(seg_of_pair, group):
        if h >= 0:
            members[(int(g), int(h))] = members.get((int(g), int(h)), 0) + 1
    return gseg_off, [gseg_off[g] + h if h >= 0 and members[(int(g), int(h))] >= min_depth else -1 - int(g) for g, h in zip(seg_of_pair, group)]


def py_correct_groups(frames, seg_of_pair, group, n_groups, queries, base, slots, ilen, qpos, **rule):
    """ioc_planes_correct_groups from the restatements: ([sequence per pair], [qualities per pair], [{FIELDS} per pair]) — the tables
    piled by py_planes_pile, T(g, h) from the pairs of segment g in group h and T(g, *) from all of them; `queries` the reads."""
    rule = {**DEFAULT, **rule}
    _, names = py_tables_of(seg_of_pair, group, n_groups, rule["min_depth"])
    piled = {}

    def tables(g, h):
        if (g, h) not in piled:
            cols, ins = np.zeros(len(frames[g]) + 1, api.PILEUP_DTYPE), np.zeros(len(frames[g]) + 1, api.PILEUP_INS_DTYPE)
            for i in range(len(base)):
                if seg_of_pair[i] == g and (h is None or group[i] == h):
                    pp.py_planes_pile(base[i], slots[i], cols, ins)
            piled[(g, h)] = cols, ins
        return piled[(g, h)]

    seqs, quals, stats = [], [], []
    for i in range(len(base)):
        g = int(seg_of_pair[i])
        cols, ins = tables(g, int(group[i]) if names[i] >= 0 else None)
        s, q, st = py_correct_long(base[i], slots[i], ilen[i], qpos[i], cols, ins, frames[g], queries[i], **rule)
        st["table"] = names[i]
        seqs.append(s), quals.append(q), stats.append(st)
    return seqs, quals, stats


def stats_dicts(arr):
    """the records of a call as a list of {FIELDS}"""
    return [{f: int(r[f]) for f in FIELDS} for r in arr]


# ---- hand planes: long rows at the 64-row steps ----
def hand_read(rlen, long_rows, seed=0, depth=10):
    """A read that agrees with its frame on every row of a table of `depth` reads that do, with the long insertions {row: length} in
    it: (frame, base, slots, ilen, qpos, cols, ins, query, want) — want the sequence it must come back as, the read itself (every
    base is supported, nothing is inserted by the others: the long runs are all that differs from the frame)."""
    rng = np.random.default_rng(seed)
    frame = bytes(rng.choice(list(b"ACGT"), rlen).tolist())
    base = np.array([pc.CH[c] for c in frame] + [NONE], np.uint8)
    slots, ilen, qpos = np.zeros((SLOTS, rlen + 1), np.uint8), np.zeros(rlen + 1, np.uint8), np.zeros(rlen + 1, np.uint32)
    cols, ins = np.zeros(rlen + 1, api.PILEUP_DTYPE), np.zeros(rlen + 1, api.PILEUP_INS_DTYPE)
    for p, c in enumerate(frame):
        cols[pc.COL_FIELDS[pc.CH[c]]][p] = depth
    query = bytearray()
    for p in range(rlen + 1):
        qpos[p] = len(query)
        n = long_rows.get(p, 0)
        if n:
            run = bytes(rng.choice(list(b"ACGT"), n).tolist())
            query += run
            ilen[p] = n
            for j in range(min(n, SLOTS)):
                slots[j, p] = 1 + pc.CH[run[j]]
        if p < rlen:
            query.append(frame[p])
    return frame, base, slots, ilen, qpos, cols, ins, bytes(query), bytes(query)


# (name, rlen, {row: length}): rows 0, 63, 64 and rlen, of 7, 8 and 254 bases, and two in one 64-row chunk
HAND_LONG = [
    ("row_0_len_7", 130, {0: 7}),
    ("row_63_len_8", 130, {63: 8}),
    ("row_64_len_254", 130, {64: 254}),
    ("row_rlen_len_7", 130, {130: 7}),
    ("row_rlen_len_254_at_a_step", 128, {128: 254}),
    ("two_in_one_chunk", 130, {70: 254, 75: 8}),
    ("all_steps", 200, {0: 8, 63: 254, 64: 7, 127: 9, 128: 254, 200: 8}),
    ("short_rows_stay_with_the_slot_rule", 70, {10: 6, 20: 7}),
]


# ---- the segments of the GPU test ----
def grouped_case(seed=7, min_depth=3):
    """Two segments of 130 and 200 rows and some 40 pairs that no aligner made but every one could have: reads that follow their
    frame with a few substitutions and short insertions, isoforms that skip a stretch across a 64-row step (a run of deletions of
    at most max_run rows in the reads of a group), groups of min_depth - 1 and of exactly min_depth members, an empty group and
    pairs in no group, long rows of 7, 8 and 254 bases at rows 0, 63, 64 and rlen and two in one chunk, and one pair for each way
    of being unresolved.  Returns a dict: frames, seg_of_pair, group, n_groups, queries (the reads, which are the pool), base,
    slots, ilen, qpos (lists per pair)."""
    rng = np.random.default_rng(seed)
    frames = [bytes(rng.choice(list(b"ACGT"), n).tolist()) for n in (130, 200)]
    # (segment, group): the rows its reads lack — 8 rows across a step in a group of exactly min_depth, too few reads for the whole
    # segment to keep; 12 rows in the two reads of segment 1 that are in no group: above max_run 10, the guard keeps them
    skip = {(0, 2): (60, 68), (1, 0): (120, 130), (1, 1): (10, 14), (1, -1): (100, 112)}
    # (segment, group, reads): group 3 of segment 0 stays empty; -1: in no group
    plan = [(0, 0, 9), (0, 1, min_depth - 1), (0, 2, min_depth), (0, -1, 3), (1, 0, 6), (1, 1, 12), (1, -1, 2)]
    long_at = {2: {0: 7}, 4: {63: 8}, 5: {64: 254}, 7: {130: 7}, 9: {70: 254, 75: 8}, 10: {129: 9, 130: 254},
               20: {0: 254, 63: 7, 64: 8}, 22: {127: 254, 128: 254}, 25: {200: 8}, 30: {192: 7, 199: 254, 200: 254}}
    out = dict(frames=frames, seg_of_pair=[], group=[], n_groups=[4, 2], queries=[], base=[], slots=[], ilen=[], qpos=[])
    i = 0
    for g, h, n in plan:
        frame, rlen = frames[g], len(frames[g])
        for _ in range(n):
            base = np.array([pc.CH[c] for c in frame] + [NONE], np.uint8)
            sub = rng.random(rlen) < 0.04
            base[:rlen][sub] = rng.integers(0, 4, int(sub.sum()))
            base[:rlen][rng.random(rlen) < 0.02] = DEL
            if (g, h) in skip:
                base[skip[(g, h)][0]:skip[(g, h)][1]] = DEL
            first, end = int(rng.integers(0, 4)), rlen - int(rng.integers(0, 4))   # (free ends: not covered)
            if i in long_at:
                first, end = 0, rlen
            base[:first], base[end:rlen] = NONE, NONE
            slots, ilen, qpos = np.zeros((SLOTS, rlen + 1), np.uint8), np.zeros(rlen + 1, np.uint8), np.zeros(rlen + 1, np.uint32)
            query = bytearray()
            for p in range(rlen + 1):
                qpos[p] = len(query)
                n_ins = long_at.get(i, {}).get(p, 0)
                spanned = first < p <= end and (p == rlen or base[p] != NONE)
                if not n_ins and spanned and rng.random() < 0.05:
                    n_ins = int(rng.integers(1, SLOTS + 1))
                if n_ins:
                    run = bytes(rng.choice(list(b"ACGT"), n_ins).tolist())
                    query += run
                    ilen[p] = n_ins
                    for j in range(min(n_ins, SLOTS)):
                        slots[j, p] = 1 + pc.CH[run[j]]
                if p < rlen and base[p] <= 4:
                    query.append(b"ACGTN"[base[p]])
            out["seg_of_pair"].append(g), out["group"].append(h), out["queries"].append(bytes(query))
            out["base"].append(base), out["slots"].append(slots), out["ilen"].append(ilen), out["qpos"].append(qpos)
            i += 1
    # the unresolved ones: the plane's cap, a run that leaves the read, a long row the read does not span
    out["ilen"][1][40] = 255
    out["ilen"][15][50], out["qpos"][15][50] = 100, len(out["queries"][15]) - 99
    out["ilen"][27][100], out["base"][27][100] = 9, NONE
    out["unresolved"] = [1, 15, 27]
    return out


# ---- the planted case of the fused call (tests/test_gpu_align_blocks_correct.py) ----
EXON = (150, 170)      # the rows of the representative the minority isoform skips: 20, at most PLANTED_RULE's max_run
INSERT_AT, INSERT_LEN = 300, 40   # where the carriers have an exon the representative lacks, and its length
PLANTED_BLOCKS = dict(min_gap=10, min_block=10, min_pct=15)   # (low enough for the block search to find 4 reads of 19 skipping 20 rows)
PLANTED_RULE = dict(min_depth=3, min_alt=3, min_pct=25, max_run=24)
PLANTED_SIZES = (12, 4, 3)   # reads of the representative's isoform, of the minority's, carriers: need(19) = 5 > 4 >= min_alt, min_depth
PLANTED_SEED = 3


def planted_isoforms(seed=PLANTED_SEED, q=(12.0, 18.0)):
    """(T, reads, truths) built with tests/structured_reads.py's noise: 12 reads of T (400 bases), 4 of T without EXON — fewer than
    need(depth), so that a correction against the whole cluster pastes the exon back — and 3 of T with 40 bases inserted in front of
    row 300; all on the forward strand (a read of the reverse strand is turned back), at qualities drawn from `q`.  truths[i] is what
    read i was read from."""
    from tests import structured_reads as sr
    rng = np.random.default_rng(seed)
    T = sr._rand(rng, 400)
    extra = sr._rand(rng, INSERT_LEN)
    tr = [T, np.concatenate([T[:EXON[0]], T[EXON[1]:]]), np.concatenate([T[:INSERT_AT], extra, T[INSERT_AT:]])]
    reads, truths = [], []
    for t, n in zip(tr, PLANTED_SIZES):
        rs = sr.reads_from([t], n, rng, q_lo=q[0], q_hi=q[1])
        for i in range(n):
            s = rs.seq[rs.offs[i]:rs.offs[i + 1]]
            reads.append((sr._COMP[s[::-1]] if rs.strand[i] < 0 else s).tobytes())
            truths.append(t.tobytes())
    return T.tobytes(), reads, truths


def project_all(ops, query, rlen):
    """(base, slots, ilen, qpos) of one string through the host projections"""
    return api.ops_project(ops, query, rlen)[0], api.ops_project_ins(ops, query, rlen), api.ops_project_ilen(ops, rlen), api.ops_project_qpos(ops, rlen)


def whole_read(read, ops, corrected):
    """the read with its aligned part replaced: what a record of corrected_reads.fq holds"""
    st = api.ops_stats(ops)
    return read[:st["lead_i"]] + corrected + read[len(read) - st["trail_i"]:]
