"""What the tests of the variants of an insertion site share: plain restatements of ioc_host_ops_agreement, ioc_host_key_isoforms and
ioc_host_insert_window_variants from the rules in include/isonclust2_hip.h (the windows, the aligner and a slot's consensus are
windows_common's); planted segments where each rule of the decision bites; and the property case — representative A of
inserts_common with two different exons at its first junction."""
import random

import numpy as np

from isonclust2_amd import api
from tests import blocks_common as bc
from tests import inserts_common as ic
from tests import iso_polish_common as ipc
from tests import polish_common as pc
from tests import windows_common as wc

CARRY, CARRY_B, LACK, NOT = api.INS_CARRY, api.INS_CARRY_B, api.INS_LACK, api.INS_NONE
VOTER, SHORT, LONG = api.WIN_VOTER, api.WIN_SHORT, api.WIN_LONG
NONE, A, B, OTHER = api.WINVAR_NONE, api.WINVAR_A, api.WINVAR_B, api.WINVAR_OTHER
NO = api.NO_AGREEMENT
RULE = {**api.WINDOWS_RULE, **api.VARIANTS_RULE}


def py_agreement(ops):
    return sum({61: 1, 88: -1, 68: -1, 73: -1, 105: 0, 100: 0}[o] for o in bytes(ops))


def py_near(a, qlen, tlen, min_agree):
    return a >= 1 and 100 * a >= min_agree * max(qlen, tlen)


def py_key_isoforms(key, mask, full, min_alt, pre_key=None, pre_mask=None, pre_full=0):
    """(group, how, counts) from the rules: step 9 of ioc_host_planes_inserts"""
    n = len(key)
    pk = [int(x) for x in pre_key] if pre_key is not None else [0] * n
    pm = [int(x) for x in pre_mask] if pre_key is not None else [0] * n
    pre_full = int(pre_full) if pre_key is not None else 0
    key, mask = [int(x) for x in key], [int(x) for x in mask]
    complete = [(pk[i], key[i]) for i in range(n) if mask[i] == full and pm[i] == pre_full]
    supported = sorted(k for k in set(complete) if complete.count(k) >= min_alt)
    group, how = [], []
    for i in range(n):
        mine = (pk[i], key[i])
        if mask[i] == full and pm[i] == pre_full:
            g, h = (supported.index(mine), api.ISO_DIRECT) if mine in supported else (-1, api.ISO_RARE)
        else:
            agree = [x for x, (a, k) in enumerate(supported) if (a ^ pk[i]) & pm[i] == 0 and (k ^ key[i]) & mask[i] == 0] if mask[i] | pm[i] else []
            g, h = (agree[0], api.ISO_ASSIGNED) if len(agree) == 1 else (-1, api.ISO_AMBIGUOUS)
        group.append(g), how.append(h)
    counts = dict(n_groups=len(supported), n_direct=how.count(api.ISO_DIRECT), n_assigned=how.count(api.ISO_ASSIGNED), n_rare=how.count(api.ISO_RARE),
                  n_ambiguous=how.count(api.ISO_AMBIGUOUS))
    return np.array(group, np.int32), np.array(how, np.int32), counts


def py_variants(reads, base, qpos, sites, keys, min_depth=3, **rule):
    """one segment from the rules: a dict as api.insert_window_variants returns it"""
    r = {**RULE, **rule}
    score = (r["match"], r["mismatch"], r["gap"])
    n, S = len(reads), len(sites)
    win, cls, start, ln = wc.py_windows(base, qpos, [len(x) for x in reads], sites, keys, slack=r["slack"], max_win=r["max_win"])
    var = np.zeros(S, api.WINDOW_VARIANT_DTYPE)
    variant, agree = np.zeros((n, S), np.uint8), np.full((n, S, 2), NO, np.int32)
    key2 = [int(k) for k in keys]
    seq, qual, polish = [], [], []
    for k in range(S):
        cut = lambda i: reads[i][int(start[i, k]):int(start[i, k]) + int(ln[i, k])]
        voters = [i for i in range(n) if cls[i, k] == VOTER]
        need = bc.need(len(voters), r["min_alt"], r["min_pct"])

        def round_(who, t, which):
            near = []
            for i in who:
                a = py_agreement(wc.py_global(cut(i), cut(t), *score)[0])
                agree[i, k, which] = a
                if py_near(a, len(cut(i)), len(cut(t)), r["min_agree"]):
                    near.append(i)
            return near

        near_a = round_(voters, int(win[k]["template_pair"]), 0) if voters else []
        far = [i for i in voters if i not in near_a]
        tb, near_b = -1, []
        if len(far) >= need and len(voters) - len(far) >= need:
            tb = sorted((int(ln[i, k]), i) for i in far)[(len(far) - 1) // 2][1]
            near_b = round_(far, tb, 1)
        split = tb >= 0 and len(near_b) >= need
        va = near_a if split else voters
        vb = near_b if split else []
        var[k] = (int(split), tb, int(ln[tb, k]) if tb >= 0 else 0, len(va), len(near_b), len(far) - len(near_b) if tb >= 0 else 0, len(far), 0)
        for i in range(n):
            variant[i, k] = NONE if i not in voters else A if i in va else B if i in vb else OTHER
            st = (key2[i] >> (2 * k)) & 3
            if split and st == CARRY:
                st = NOT if cls[i, k] != VOTER or variant[i, k] == OTHER else CARRY_B if variant[i, k] == B else CARRY
            key2[i] = key2[i] & ~(3 << (2 * k)) | st << (2 * k)
        for who, t in ((va, int(win[k]["template_pair"])), (vb, tb)):
            if who:
                s, q, st, _, _ = wc.host_site([cut(i) for i in who], cut(t), min_depth, *score)
                seq.append(s), qual.append(q), polish.append(st)
            else:
                seq.append(b""), qual.append(b""), polish.append(None)
    mask2 = [sum(3 << (2 * k) for k in range(S) if (x >> (2 * k)) & 3 != NOT) for x in key2]
    return dict(win=win, var=var, variant=variant, agree=agree, key2=np.array(key2, np.uint64), mask2=np.array(mask2, np.uint64), seq=seq, qual=qual, polish=polish)


def same_as_py(got, want):
    """a result of api.insert_window_variants against py_variants', as bytes"""
    for f in ("win", "var", "variant", "agree", "key2", "mask2"):
        assert np.asarray(got[f]).tobytes() == np.asarray(want[f]).tobytes(), (f, got[f], want[f])
    assert got["seq"] == want["seq"] and got["qual"] == want["qual"]
    for x, st in enumerate(want["polish"]):
        if st is None:
            assert got["polish"][x].tobytes() == bytes(32), x
        else:
            assert all(int(got["polish"][x][f]) == st[f] for f in api.POLISH_STATS_FIELDS), (x, got["polish"][x], st)


# ---- planted segments: reads that are the frame with something inserted in front of a site's row ----
MAX_WIN = 80   # (the rule the planted segments are run with: a window of 8 + 60 + 9 bases is the longest voter)
PLANT = dict(max_win=MAX_WIN)


def _rand(rng, n):
    return bytes(b"ACGT"[x] for x in rng.integers(0, 4, n))


def _nudge(rng, s, n=1):
    """s with n substitutions: the same exon read again (the length stays)"""
    s = bytearray(s)
    for at in rng.choice(len(s), n, replace=False):
        s[at] = b"ACGT"[(b"ACGT".index(s[at]) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(s)


def plant(rng, rlen, rows, inserts, short=()):
    """(reads, base, qpos, sites, keys): a segment of rlen rows with a site [row, row + 1) for every row of `rows`; read i is the frame
    with inserts[i][k] in front of rows[k] (b"": it lacks).  short: (read, k) pairs — the read's base plane ends inside the slack
    behind site k, so that it carries and does not cover."""
    frame = _rand(rng, rlen)
    reads, base, qpos, keys = [], [], [], []
    for i, ins in enumerate(inserts):
        ops, rd, at = b"", b"", 0
        for k, row in enumerate(rows):
            ops += b"=" * (row - at) + b"I" * len(ins[k])
            rd += frame[at:row] + ins[k]
            at = row
        ops, rd = ops + b"=" * (rlen - at), rd + frame[at:]
        b = api.ops_project(ops, rd, rlen)[0]
        key = sum((CARRY if ins[k] else LACK) << (2 * k) for k in range(len(rows)))
        for j, k in short:
            if j == i:
                b[rows[k] + 4:] = api.ALLELE_NONE
                key |= sum(NOT << (2 * m) for m in range(k + 1, len(rows)))
        reads.append(rd), base.append(b), qpos.append(api.ops_project_qpos(ops, rlen)), keys.append(key)
    sites = np.zeros(len(rows), api.PILE_INSERT_DTYPE)
    sites["first"], sites["end"] = rows, [r + 1 for r in rows]
    return reads, np.array(base), np.array(qpos), sites, np.array(keys, np.uint64)


def planted_segment(seed=3):
    """One segment of 400 rows and five sites, 15 reads; need(n) is 3 up to 12 voters.  What each site is there for:
      0 (row 50)   splits 6 / 5: reads 0 .. 10 carry exon P (30 bases) and Q (24 bases) in turn, P at the even reads.  Read 11 carries
                   and ends inside the slack (IOC_WIN_SHORT), read 12 holds 70 bases (IOC_WIN_LONG at max_win 80): both are re-keyed
                   to NONE.  The five Q windows have one length: template B is the third of them by index.
      1 (row 120)  9 carriers of one exon and 2 of another: n_far 2 < need, round B does not run.
      2 (row 190)  6 carriers of one exon and 5 that hold five different ones: round B runs, n_b is 1 < need, the site does not
                   split and the far voters vote in the one consensus.
      3 (row 260)  6 carriers of P, 4 of Q and one of a third exon: the site splits and that voter is OTHER.
      4 (row 330)  reads 0 .. 4 carry one exon, nobody else: no far voter at all.
    Reads 13 and 14 lack everything."""
    rng = np.random.default_rng(seed)
    P, Q, R = _rand(rng, 30), _rand(rng, 24), _rand(rng, 27)
    ins = [[b""] * 5 for _ in range(15)]
    for i in range(11):
        ins[i][0] = _nudge(rng, P if i % 2 == 0 else Q)
        ins[i][1] = _nudge(rng, P if i < 9 else Q)
        ins[i][2] = _nudge(rng, R) if i < 6 else _rand(rng, 22 + i)
        ins[i][3] = _nudge(rng, P) if i < 6 else _nudge(rng, Q) if i < 10 else _rand(rng, 26)
    ins[11][0], ins[12][0] = _nudge(rng, P), _rand(rng, 70)
    for i in range(5):
        ins[i][4] = _nudge(rng, R)
    return plant(rng, 400, [50, 120, 190, 260, 330], ins, short=[(11, 0)])


def quiet_segment(seed=5):
    """a segment where no site splits: two sites, 8 carriers of one exon each and 4 reads that lack"""
    rng = np.random.default_rng(seed)
    P, Q = _rand(rng, 30), _rand(rng, 40)
    ins = [[_nudge(rng, P), _nudge(rng, Q)] if i < 8 else [b"", b""] for i in range(12)]
    return plant(rng, 300, [80, 200], ins)


# ---- the property case ----
# Representative A of inserts_common (T without [150, 190) and [400, 520)).  At its first junction 10 reads hold exon EXON_A (60
# bases) and 10 a different exon EXON_B (45 bases), all 20 with [400, 520) behind it; 6 reads lack it and hold [400, 520), 6 lack both
# — three isoforms to the insert stage, four in truth.  All mutated at 8 %, through the
# host aligner and the host projections.  The conditions, nobody left out: the site splits; every voter's variant is its planted
# exon; each consensus lies nearer to its own true window than to the other's by at least half the shorter exon.
# SEED is the first seed from 0 at which the host definition meets them (find_seed below).
SEED, SEEDS_TRIED = 0, 1
SIZES = (10, 10, 6, 6)
EXONS = (60, 45)
# measured on the host path at SEED; pinned as equalities in tests/test_window_variants_host.py: per slot of the first site (distance
# to its own true window, distance to the other's, the consensus' length)
PINNED = ((1, 34, 77), (0, 34, 93))


def property_reads(seed, rate=0.08):
    """(frame, exons, reads, planted): planted[i] is WINVAR_A / WINVAR_B for a carrier of the first junction, WINVAR_NONE else"""
    rng = random.Random(seed)
    T = bytes(rng.choice(b"ACGT") for _ in range(1000))
    frame = ic.representative(T, "A")
    (a0, _), (b0, b1) = bc.CUTS
    ea, eb = (bytes(rng.choice(b"ACGT") for _ in range(n)) for n in EXONS)
    second = T[b0:b1]
    j2 = ic.JUNCTIONS_A[1]
    iso = [frame[:a0] + ea + frame[a0:j2] + second + frame[j2:], frame[:a0] + eb + frame[a0:j2] + second + frame[j2:], frame[:j2] + second + frame[j2:], frame]
    reads, planted = [], []
    for x, n in enumerate(SIZES):
        reads += [pc.mutate(rng, iso[x], rate) for _ in range(n)]
        planted += [(A, B, NONE, NONE)[x]] * n
    return frame, (ea, eb), reads, planted


def host_property(seed=None, **rule):
    """(frame, exons, reads, planted, inserts, variants): the property case on the host path"""
    frame, exons, reads, planted = property_reads(SEED if seed is None else seed)
    base, ilen, qpos = [], [], []
    for rd in reads:
        ops, _ = api.host_align_ops(rd, frame, gap_open=pc.gap_open(0.1))
        base.append(api.ops_project(ops, rd, len(frame))[0]), ilen.append(api.ops_project_ilen(ops, len(frame))), qpos.append(api.ops_project_qpos(ops, len(frame)))
    base, ilen, qpos = np.array(base, np.uint8), np.array(ilen, np.uint8), np.array(qpos, np.uint32)
    ins = api.planes_inserts(base, ilen)
    return frame, exons, reads, planted, (base, qpos, ins), api.insert_window_variants(base, qpos, [len(x) for x in reads], ins["sites"], ins["reads"]["key"], reads, **rule)


def true_windows(frame, exons, lo, hi):
    a0 = bc.CUTS[0][0]
    assert lo < a0 < hi
    return [frame[lo:a0] + e + frame[a0:hi] for e in exons]


def slot_exons(got, planted):
    """which planted exon each slot of the first site stands for (0: EXON_A, 1: EXON_B): variant A is the exon of the site's template,
    whichever that is — the lower median by length falls among the shorter exon's windows when the halves are equal"""
    first = 0 if planted[int(got["win"][0]["template_pair"])] == A else 1
    return first, 1 - first


def distances(frame, exons, got, planted):
    """per slot of the first site: (edit distance of its consensus to its own true window, to the other's, its length)"""
    true = true_windows(frame, exons, int(got["win"][0]["lo"]), int(got["win"][0]["hi"]))
    return tuple((ipc.edit_distance(got["seq"][h], true[e]), ipc.edit_distance(got["seq"][h], true[1 - e]), len(got["seq"][h])) for h, e in enumerate(slot_exons(got, planted)))


def property_holds(got, planted, frame, exons):
    """(the first site splits, every carrier's variant is its planted exon and nobody is left out, both margins hold)"""
    var, variant = got["var"], got["variant"]
    splits = len(var) >= 1 and int(var[0]["split"]) == 1
    slot_of = {(A, B)[e]: (A, B)[h] for h, e in enumerate(slot_exons(got, planted))} if splits else {}
    right = splits and all(int(variant[i, 0]) == slot_of.get(planted[i], NONE) for i in range(len(planted)))
    d = distances(frame, exons, got, planted) if splits else ()
    margin = splits and all(2 * (x[1] - x[0]) >= min(EXONS) for x in d)
    return splits, right, margin


def find_seed(limit=5):
    """the first seed at which the property holds, and how many were tried"""
    for s in range(limit):
        frame, exons, _, planted, _, got = host_property(s)
        if all(property_holds(got, planted, frame, exons)):
            return s, s + 1
    return None, limit
