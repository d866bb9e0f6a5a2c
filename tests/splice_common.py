"""What the tests of the isoforms' full-length sequence share: py_row and py_splice, a plain restatement of ioc_host_pileup_call row by
row and of ioc_host_isoform_splice on top of it, from the rules in include/isonclust2_hip.h; random tables and plans; the definition
of the device entry group-segment by group-segment from the host functions; and the property cases — the reads of
blocks_common.property_case against representatives A and B of inserts_common through the host aligner, the host projections and
the definitions."""
import numpy as np

from isonclust2_amd import api
from tests import blocks_common as bc
from tests import inserts_common as ic
from tests import iso_polish_common as ipc
from tests import plane_pile_common as pp
from tests import polish_common as pc
from tests import windows_common as wc

LACK, DONE, UNCALLED, OVERLAP = api.SPLICE_LACK, api.SPLICE_DONE, api.SPLICE_UNCALLED, api.SPLICE_OVERLAP
CARRY = api.INS_CARRY
STAT_KEYS = ("n_sub", "n_del", "n_ins", "n_low")


def py_row(cols, ins, frame, p, min_depth):
    """row p of ioc_host_pileup_call: (sequence, qualities, {n_sub, n_del, n_ins, n_low}) of what the row emits and counts"""
    rlen = len(frame)
    seq, qual, st = bytearray(), bytearray(), dict.fromkeys(STAT_KEYS, 0)
    D = pc._depth(cols[p]) if p < rlen else (pc._depth(cols[rlen - 1]) if rlen else 0)
    for s in range(pc.SLOTS):
        slot = [int(v) for v in ins["slot"][p][s]]
        if not (D >= min_depth and 2 * sum(slot) > D):
            break
        seq.append(pc.LETTER[slot.index(max(slot))]), qual.append(33 + min(40, 40 * max(slot) // D))
        st["n_ins"] += 1
    if p == rlen:
        return bytes(seq), bytes(qual), st
    d = pc._depth(cols[p])
    if d < min_depth:
        st["n_low"] += 1
        return bytes(seq) + frame[p:p + 1], bytes(qual) + b"!", st
    cnt = [int(cols[p][f]) for f in pc.COL_FIELDS]
    m, fch = max(cnt), pc.CH.get(frame[p], 4)
    who = fch if cnt[fch] == m else cnt.index(m)
    if who == 5:
        st["n_del"] += 1
        return bytes(seq), bytes(qual), st
    st["n_sub"] += who != fch
    seq.append(frame[p] if who == fch else pc.LETTER[who]), qual.append(33 + min(40, 40 * m // d))
    return bytes(seq), bytes(qual), st


def py_states(key, win):
    """rule 1: the state of every site under a key"""
    out, last_hi = [], 0
    for b, w in enumerate(win):
        if (int(key) >> (2 * b)) & 3 != CARRY:
            out.append(LACK)
        elif int(w["tlen"]) == 0:
            out.append(UNCALLED)
        elif int(w["lo"]) < last_hi:
            out.append(OVERLAP)
        else:
            out.append(DONE)
            last_hi = int(w["hi"])
    return out


def py_splice(cols, ins, frame, key, win, win_seq, min_depth):
    """ioc_host_isoform_splice as api.isoform_splice returns it: (sequence, qualities, stats, sites, sstats)"""
    rlen, states = len(frame), py_states(key, win)
    start = {int(win[b]["lo"]): b for b, s in enumerate(states) if s == DONE}
    gone = {p for b, s in enumerate(states) if s == DONE for p in range(int(win[b]["lo"]), int(win[b]["hi"]))}
    sites = np.zeros(len(win), api.SPLICE_SITE_DTYPE)
    sites["state"], sites["at"] = states, -1
    seq, qual, st = b"", b"", dict.fromkeys(("out_len",) + STAT_KEYS, 0)
    for p in range(rlen + 1):
        if p in start:
            b = start[p]
            sites[b]["at"], sites[b]["len"] = len(seq), len(win_seq[b][0])
            seq, qual = seq + bytes(win_seq[b][0]), qual + bytes(win_seq[b][1])
        if p in gone:
            continue
        s, q, d = py_row(cols, ins, frame, p, min_depth)
        seq, qual = seq + s, qual + q
        for f in STAT_KEYS:
            st[f] += d[f]
    st["out_len"] = len(seq)
    done = [b for b, s in enumerate(states) if s == DONE]
    sstats = dict(n_done=len(done), n_uncalled=states.count(UNCALLED), n_overlap=states.count(OVERLAP),
                  rows_replaced=sum(int(win[b]["hi"]) - int(win[b]["lo"]) for b in done), spliced_bytes=sum(len(win_seq[b][0]) for b in done))
    return seq, qual, st, sites, sstats


def same_splice(got, want):
    """two results of isoform_splice / py_splice, as bytes"""
    assert got[0] == want[0] and got[1] == want[1], (got[0], want[0])
    assert got[2] == want[2] and got[4] == want[4], (got[2], want[2], got[4], want[4])
    assert got[3].tobytes() == want[3].tobytes(), (got[3], want[3])


def windows(spans, tlen=None):
    """INSERT_WINDOW_DTYPE records of [(lo, hi)]; tlen 1 (called) unless given per site"""
    w = np.zeros(len(spans), api.INSERT_WINDOW_DTYPE)
    for b, (lo, hi) in enumerate(spans):
        w[b]["lo"], w[b]["hi"], w[b]["template_pair"], w[b]["tlen"] = lo, hi, 0, 1 if tlen is None else tlen[b]
    return w


def random_string(rng, n):
    return (bytes(b"ACGTN"[x] for x in rng.integers(0, 5, n)), bytes(33 + int(x) for x in rng.integers(0, 41, n)))


def key_of(states):
    return sum(int(s) << (2 * b) for b, s in enumerate(states))


def random_plan(rng, rlen, n_sites, lens=(0, 1, 8, 40)):
    """(key, win, win_seq) of a segment of rlen >= 2 rows: windows in ascending order of lo, some of them overlapping the one before,
    some not called, under a key of every state"""
    los = sorted(int(x) for x in rng.integers(1, rlen, n_sites))
    spans = [(lo, int(min(rlen, lo + 1 + rng.integers(0, max(2, rlen // max(n_sites, 1)))))) for lo in los]
    tlen = [int(x) for x in rng.choice([0, 5], n_sites, p=[.2, .8])]
    win_seq = [random_string(rng, int(rng.choice(lens)) if t else 0) for t in tlen]
    key = key_of(rng.choice([api.INS_LACK, CARRY, CARRY, api.INS_NONE, 2], n_sites))
    return key, windows(spans, tlen), win_seq


def group_keys(n_segs, seg_of_pair, ireads, n_groups):
    """a key per group-segment: that of the lowest-numbered DIRECT read of the group (0 for a group without one)"""
    gseg_off = np.concatenate([[0], np.cumsum(n_groups)]).astype(np.int64)
    keys = np.zeros(int(gseg_off[-1]), np.uint64)
    seen = set()
    for i, g in enumerate(seg_of_pair):
        h = int(ireads[i]["group"])
        if int(ireads[i]["how"]) == api.ISO_DIRECT and 0 <= h < int(n_groups[g]) and (g, h) not in seen:
            seen.add((g, h))
            keys[int(gseg_off[g]) + h] = ireads[i]["key"]
    return keys


def host_isoforms_full(frames, seg_of_pair, group, n_groups, base, slots, iso_key, win, win_seq, win_qual, min_depth):
    """The definition of the device entry from the host functions: api.isoform_splice over the tables api.planes_pile adds up from
    every group's pairs.  Returns a dict like Context.planes_isoforms_full's with tables=True."""
    ns = len(frames)
    gseg_off, gmem_off, gmembers = ipc.py_group_member_lists(ns, seg_of_pair, group, n_groups)
    out = {"gseq": [], "gqual": [], "gpolish": [], "gseg_off": np.array(gseg_off, np.int64), "splice": [], "grow0": []}
    gcols, gins, sst, off, spoff, rows = [], [], [], [0], [0], 0
    for g, frame in enumerate(frames):
        out["gseq"].append([]), out["gqual"].append([])
        pol = np.zeros(int(n_groups[g]), api.POLISH_STATS_DTYPE)
        for h in range(int(n_groups[g])):
            x = gseg_off[g] + h
            cols, ins = np.zeros(len(frame) + 1, api.PILEUP_DTYPE), np.zeros(len(frame) + 1, api.PILEUP_INS_DTYPE)
            for i in gmembers[gmem_off[x]:gmem_off[x + 1]]:
                api.planes_pile(base[i], slots[i], cols=cols, ins=ins)
            s, q, st, sites, ss = api.isoform_splice(cols, ins, frame, int(iso_key[x]), win[g], list(zip(win_seq[g], win_qual[g])), min_depth)
            out["gseq"][g].append(s), out["gqual"][g].append(q), out["splice"].append(sites), out["grow0"].append(rows)
            for f in api.POLISH_STATS_FIELDS:
                pol[h][f] = st[f]
            rec = np.zeros(1, api.SPLICE_STATS_DTYPE)[0]
            for f in api.SPLICE_STATS_FIELDS:
                rec[f] = ss[f]
            sst.append(rec), gcols.append(cols), gins.append(ins), off.append(off[-1] + len(s)), spoff.append(spoff[-1] + len(sites))
            rows += len(frame) + 1
        out["gpolish"].append(pol)
    cat = lambda parts, dt: np.concatenate([np.zeros(0, dt)] + parts)
    out.update(off=np.array(off, np.int64), splice_off=np.array(spoff, np.int64), sstats=np.array(sst, api.SPLICE_STATS_DTYPE).reshape(-1),
               gcols=cat(gcols, api.PILEUP_DTYPE), gins=cat(gins, api.PILEUP_INS_DTYPE), grow0=np.array(out["grow0"], np.int64))
    return out


def same_full(got, want, tables=True):
    """a result of Context.planes_isoforms_full against the definition, as bytes"""
    ipc.same_groups(got, want, tables)
    assert got["off"].tolist() == want["off"].tolist() and got["splice_off"].tolist() == want["splice_off"].tolist()
    assert got["sstats"].tobytes() == want["sstats"].tobytes(), (got["sstats"], want["sstats"])
    assert len(got["splice"]) == len(want["splice"])
    for x, (a, b) in enumerate(zip(got["splice"], want["splice"])):
        assert a.tobytes() == b.tobytes(), (x, a, b)


# ---- the property cases ----
# Representative A lacks both exons (two sites), B the first one only (a block and a site).  Every combined isoform's full-length
# sequence must lie nearer (edit distance) to its own true transcript than to each of the other three, and every isoform that
# carries an exon must be nearer to its transcript than the unspliced call of the same tables by at least half the carried exons'
# total length (windows_common.MARGIN is half of 40 and of 120).  The seed of each case is the first of 0, 1, .. 5 at which the
# conditions of the stages before (inserts_common) and these hold on the host path (find_seeds below).
EXONS = {"A": (bc.CUTS[0][1] - bc.CUTS[0][0], bc.CUTS[1][1] - bc.CUTS[1][0]), "B": (bc.CUTS[0][1] - bc.CUTS[0][0],)}
assert tuple(e // 2 for e in EXONS["A"]) == wc.MARGIN
SEED_A, SEEDS_TRIED_A = 0, 1
SEED_B, SEEDS_TRIED_B = 0, 1
# measured on the host path at the seeds; pinned as equalities in tests/test_iso_splice_host.py: per combined isoform, in the
# library's order, (its true isoform, the distances of its full-length sequence to the four true transcripts, the distance of the
# unspliced call of the same tables to its own transcript)
PINNED_A = ((2, (160, 120, 0, 40), 0), (3, (120, 160, 40, 0), 34), (1, (40, 0, 120, 160), 114), (0, (0, 40, 160, 120), 148))
PINNED_B = ((1, (40, 0, 120, 160), 0), (0, (0, 40, 160, 120), 34), (2, (160, 120, 0, 40), 0), (3, (120, 160, 40, 0), 34))


def carried(which, true_iso):
    """the total length of the exons true isoform x holds and the representative lacks"""
    if which == "A":
        return sum(e for e, s in zip(EXONS["A"], ic.TRUE_A[true_iso]) if s == CARRY)
    return EXONS["B"][0] if ic.TRUE_B[true_iso][1] == CARRY else 0


def host_case(which, seed, min_depth=3):
    """the property case on the host path up to the windows: a dict of T, frame, reads, the planes per read, the insert stage's
    result (combined isoforms) and the windows"""
    T, reads, _ = bc.property_case(seed)
    frame = ic.representative(T, which)
    base, slots, ilen, qpos = [], [], [], []
    for rd in reads:
        ops, _ = api.host_align_ops(rd, frame, gap_open=pc.gap_open(0.1))
        b, s = pp.planes_of(ops, rd, len(frame))
        base.append(np.asarray(b, np.uint8)), slots.append(np.asarray(s, np.uint8))
        ilen.append(api.ops_project_ilen(ops, len(frame))), qpos.append(api.ops_project_qpos(ops, len(frame)))
    ba, la, qa = np.array(base, np.uint8), np.array(ilen, np.uint8), np.array(qpos, np.uint32)
    blocks = None
    if which == "B":
        blocks = api.planes_blocks(ba)
        nb = len(blocks["blocks"])
        mask = np.array([sum(3 << (2 * b) for b in range(nb) if (int(k) >> (2 * b)) & 3 != bc.NOT) for k in blocks["reads"]["key"]], np.uint64)
        ins = api.planes_inserts(ba, la, pre_key=blocks["reads"]["key"], pre_mask=mask, pre_full=(1 << (2 * nb)) - 1)
    else:
        ins = api.planes_inserts(ba, la)
    win = wc.host_windows(reads, ba, qa, ins["sites"], ins["reads"]["key"], min_depth=min_depth)
    return dict(T=T, frame=frame, reads=reads, base=base, slots=slots, ilen=ilen, qpos=qpos, blocks=blocks, ins=ins, win=win)


def host_isoforms(case, max_iso=16, min_depth=3):
    """every combined isoform of a host_case on the host path: [(full sequence, qualities, sites, sstats, unspliced sequence)]"""
    ins, n = case["ins"], len(case["reads"])
    ng = min(int(ins["seg"]["n_groups"]), max_iso)
    keys = group_keys(1, [0] * n, ins["reads"], [ng])
    got = host_isoforms_full([case["frame"]], [0] * n, ins["reads"]["group"].tolist(), [ng], case["base"], case["slots"], keys, [case["win"]["win"]],
                             [case["win"]["seq"]], [case["win"]["qual"]], min_depth)
    out = []
    for h in range(ng):
        r0 = int(got["grow0"][h])
        cols, tins = got["gcols"][r0:r0 + len(case["frame"]) + 1], got["gins"][r0:r0 + len(case["frame"]) + 1]
        out.append((got["gseq"][0][h], got["gqual"][0][h], got["splice"][h], got["sstats"][h], api.pileup_call(cols, tins, case["frame"], min_depth)[0]))
    return out


def true_of_groups(ireads, ng):
    """the true isoform of every combined isoform: that of its complete reads (the first 38 reads of property_case), all the same"""
    truth = ic.true_of_reads()
    out = []
    for h in range(ng):
        mine = {truth[i] for i in range(len(truth)) if int(ireads[i]["group"]) == h and int(ireads[i]["how"]) == api.ISO_DIRECT}
        out.append(mine.pop() if len(mine) == 1 else -1)
    return out


def measure(which, T, ireads, seqs, unspliced):
    """per combined isoform: (its true isoform, the distances of its sequence to the four true transcripts, the distance of the
    unspliced call to its own transcript)"""
    iso = ipc.true_isoforms(T)
    true = true_of_groups(ireads, len(seqs))
    return tuple((x, tuple(ipc.edit_distance(s, t) for t in iso), ipc.edit_distance(u, iso[x]) if x >= 0 else -1) for x, s, u in zip(true, seqs, unspliced))


def property_holds(which, measured):
    """four isoforms, each of another true isoform, each nearer its own transcript than any other, and the carriers nearer than their
    unspliced call by at least half the carried exons' length"""
    if len(measured) != 4 or sorted(x for x, _, _ in measured) != [0, 1, 2, 3]:
        return False
    nearer = all(d[x] < min(d[y] for y in range(4) if y != x) for x, d, _ in measured)
    gained = all(u - d[x] >= carried(which, x) / 2 for x, d, u in measured if carried(which, x) > 0)
    return nearer and gained


def host_measure(which, seed):
    case = host_case(which, seed)
    iso = host_isoforms(case)
    return case, iso, measure(which, case["T"], case["ins"]["reads"], [i[0] for i in iso], [i[4] for i in iso])


def find_seeds(limit=6):
    """the first seed at which each property holds on the host path, how many were tried, and what every seed tried gave"""
    out = {}
    for which in "AB":
        seen = []
        for seed in range(limit):
            seen.append(host_measure(which, seed)[2])
            if property_holds(which, seen[-1]):
                break
        out[which] = (seed if property_holds(which, seen[-1]) else None, len(seen), seen)
    return out
