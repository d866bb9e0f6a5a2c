"""What the tests of the inserted exon's sequence share: plain restatements of ioc_host_ops_project_qpos, ioc_host_align_global_ops
and ioc_host_insert_windows from the rules in include/isonclust2_hip.h; the host path of a site's consensus (the global aligner, both
host projections, api.planes_pile and api.pileup_call); planted planes where the clamps, the classes and the template's order bite;
and the property case — the reads of blocks_common.property_case against representative A of inserts_common."""
import numpy as np

from isonclust2_amd import api
from tests import blocks_common as bc
from tests import inserts_common as ic
from tests import iso_polish_common as ipc

DEL, NONE = api.ALLELE_DEL, api.ALLELE_NONE
CARRY, LACK, NOT = api.INS_CARRY, api.INS_LACK, api.INS_NONE
RULE = dict(api.WINDOWS_RULE)


def py_qpos(ops, rlen):
    """the position plane of one operation string, or None where the definition refuses it"""
    ops = bytes(ops)
    if any(o not in b"=XIDid" for o in ops) or sum(o in b"=XDd" for o in ops) != rlen:
        return None
    out, q = [0], 0
    for o in ops:
        q += o in b"=XIi"
        if o in b"=XDd":
            out.append(q)
    return np.array(out, np.uint32)


def py_global(query, ref, match=2, mismatch=-2, gap=2):
    """(ops, score): the whole matrix in Python integers and the walk back — the diagonal first, then 'D', then 'I'"""
    n, m = len(query), len(ref)
    H = [[-j * gap for j in range(m + 1)]] + [[-i * gap] + [0] * m for i in range(1, n + 1)]
    sub = lambda i, j: match if query[i - 1] == ref[j - 1] else mismatch
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            H[i][j] = max(H[i - 1][j - 1] + sub(i, j), H[i][j - 1] - gap, H[i - 1][j] - gap)
    i, j, back = n, m, []
    while i or j:
        if i and j and H[i][j] == H[i - 1][j - 1] + sub(i, j):
            back.append(b"="[0] if query[i - 1] == ref[j - 1] else b"X"[0])
            i, j = i - 1, j - 1
        elif j and (i == 0 or H[i][j] == H[i][j - 1] - gap):
            back.append(b"D"[0])
            j -= 1
        else:
            back.append(b"I"[0])
            i -= 1
    return bytes(reversed(back)), H[n][m]


def ops_score(ops, match=2, mismatch=-2, gap=2):
    """what a string of "=XID" costs: a plain loop"""
    return sum({61: match, 88: mismatch, 73: -gap, 68: -gap}[o] for o in ops)


def py_windows(base, qpos, qlen, sites, keys, slack=8, max_win=512):
    """(win, cls, start, len) as api.insert_windows returns them, from the rules"""
    base, qpos = np.asarray(base, np.uint8), np.asarray(qpos, np.uint32)
    n, rlen, S = base.shape[0], base.shape[1] - 1, len(sites)
    win = np.zeros(S, api.INSERT_WINDOW_DTYPE)
    cls, start, ln = np.zeros((n, S), np.uint8), np.zeros((n, S), np.uint32), np.zeros((n, S), np.uint32)
    for k in range(S):
        lo, hi = max(int(sites[k]["first"]) - slack, 1), min(int(sites[k]["end"]) + slack, rlen)
        voters = []
        for i in range(n):
            if (int(keys[i]) >> (2 * k)) & 3 != CARRY:
                continue
            a, b = int(qpos[i, lo]), int(qpos[i, hi])
            if base[i, lo - 1] > DEL or base[i, hi - 1] > DEL:
                cls[i, k] = api.WIN_SHORT
            elif b < a or b > int(qlen[i]) or not 1 <= b - a <= max_win:
                cls[i, k] = api.WIN_LONG
            else:
                cls[i, k], start[i, k], ln[i, k] = api.WIN_VOTER, a, b - a
                voters.append((b - a, i))
        voters.sort()
        t = voters[(len(voters) - 1) // 2] if voters else (0, -1)
        win[k] = (lo, hi, t[1], t[0], len(voters), int((cls[:, k] == api.WIN_SHORT).sum()), int((cls[:, k] == api.WIN_LONG).sum()), 0)
    return win, cls, start, ln


def host_site(windows, template, min_depth=3, match=2, mismatch=-2, gap=2):
    """the consensus of one site on the host path: every voter's window (bytes, in pair order) aligned to the template's, projected,
    piled and called — (sequence, qualities, stats, cols, ins)"""
    t = len(template)
    cols, ins = np.zeros(t + 1, api.PILEUP_DTYPE), np.zeros(t + 1, api.PILEUP_INS_DTYPE)
    for w in windows:
        ops, _ = api.align_global_ops(w, template, match, mismatch, gap)
        api.planes_pile(api.ops_project(ops, w, t)[0], api.ops_project_ins(ops, w, t), cols=cols, ins=ins)
    return api.pileup_call(cols, ins, template, min_depth) + (cols, ins)


def host_windows(reads, base, qpos, sites, keys, min_depth=3, **rule):
    """one segment on the host path: api.insert_windows and host_site per called site — a dict as Context.planes_insert_windows
    returns it (template_pair: the read), with `cols` / `ins` a list per site (None where the site is not called)"""
    r = {**RULE, **rule}
    w = api.insert_windows(base, qpos, [len(x) for x in reads], sites, keys, slack=r["slack"], max_win=r["max_win"])
    out = {"win": w["win"], "seq": [], "qual": [], "polish": [], "cols": [], "ins": []}
    for k, rec in enumerate(w["win"]):
        if rec["tlen"] == 0:
            out["seq"].append(b""), out["qual"].append(b""), out["polish"].append(None), out["cols"].append(None), out["ins"].append(None)
            continue
        cut = lambda i: reads[i][int(w["start"][i, k]):int(w["start"][i, k]) + int(w["len"][i, k])]
        voters = [cut(i) for i in range(len(reads)) if w["cls"][i, k] == api.WIN_VOTER]
        s, q, st, cols, ins = host_site(voters, cut(int(rec["template_pair"])), min_depth, r["match"], r["mismatch"], r["gap"])
        out["seq"].append(s), out["qual"].append(q), out["polish"].append(st), out["cols"].append(cols), out["ins"].append(ins)
    return out


def same_site(got, x, want, k):
    """site x of a device result against site k of a host_windows result, as bytes (the template's index is compared by the caller)"""
    for f in ("lo", "hi", "tlen", "n_voters", "n_short", "n_long", "reserved"):
        assert int(got["win"][x][f]) == int(want["win"][k][f]), (x, f, got["win"][x], want["win"][k])
    assert (got["seq"][x], got["qual"][x]) == (want["seq"][k], want["qual"][k]), (x, got["seq"][x], want["seq"][k])
    if want["polish"][k] is not None:
        assert all(int(got["polish"][x][f]) == want["polish"][k][f] for f in api.POLISH_STATS_FIELDS), (x, got["polish"][x], want["polish"][k])
    else:
        assert got["polish"][x].tobytes() == bytes(32)
    if "cols" in got and want["cols"][k] is not None:
        r0, r1 = int(got["row0"][x]), int(got["row0"][x + 1])
        assert got["cols"][r0:r1].tobytes() == want["cols"][k].tobytes() and got["ins"][r0:r1].tobytes() == want["ins"][k].tobytes(), x


# ---- planted planes: one segment of 200 rows, reads that are their own planes ----
def planted_segment(max_win=40, slack=8):
    """(reads, base, qpos, sites, keys, what): a segment of 200 rows and three sites — [1, 3) at junction 1, where lo clamps at 1;
    [100, 101); [198, 200), which ends at rlen - 1 and hi clamps at rlen.  Every read covers all rows with one base a row, and inserts
    what `what` says in front of row 100: reads 0 .. 3 windows of 25, 25, 30 and 21 (equal lengths are decided by the index), read 4
    a window of max_win — five voters, an odd number —, read 5 one of max_win + 1 (n_long), read 6 ends inside the slack (n_short),
    read 7 lacks.  At the first site reads 0 .. 3 carry, 15 bases each (an even number of voters); at the last nobody does."""
    rng = np.random.default_rng(11)
    rand = lambda n: bytes(b"ACGT"[x] for x in rng.integers(0, 4, n))
    rlen, rows_in_win = 200, 1 + 2 * slack
    extra = [25, 25, 30, 21, max_win, max_win + 1, 25, 0]
    ins100 = [e - rows_in_win if e else 0 for e in extra]   # the window of site 1 has 17 rows at slack 8: its bases plus the insertion
    reads, base, qpos, keys = [], [], [], []
    for i, n_ins in enumerate(ins100):
        first = 5 if i < 4 else 0                            # what reads 0 .. 3 insert in front of row 2: the first site
        body = rand(rlen)
        ops = b"=" * 2 + b"I" * first + b"=" * 98 + b"I" * n_ins + b"=" * 100
        rd = body[:2] + rand(first) + body[2:100] + rand(n_ins) + body[100:]
        b = api.ops_project(ops, rd, rlen)[0]
        if i == 6:
            b[105:] = NONE                                   # ends inside the slack of site 1: covers row lo - 1, not row hi - 1
        reads.append(rd), base.append(b), qpos.append(api.ops_project_qpos(ops, rlen))
        keys.append((CARRY if first else LACK) | (CARRY if n_ins else LACK) << 2 | (NOT if i == 6 else LACK) << 4)
    sites = np.zeros(3, api.PILE_INSERT_DTYPE)
    sites["first"], sites["end"] = [1, 100, 198], [3, 101, 200]
    return reads, np.array(base), np.array(qpos), sites, np.array(keys, np.uint64), extra


# ---- the property case ----
# The reads of blocks_common.property_case(SEED) against representative A of inserts_common, which lacks both exons: the consensus
# of a site must lie nearer to the true window WITH the exon than to the representative's own rows [lo, hi) by at least half the
# exon's length.  SEED is the seed at which property A of the insert stage holds (inserts_common.SEED_A: the first seed tried).
SEED, SEEDS_TRIED = ic.SEED_A, ic.SEEDS_TRIED_A
MARGIN = (20, 60)
# measured on the host path (host aligner, host projections, the definitions) at SEED; pinned as equalities in
# tests/test_insert_windows_host.py: per site (distance to the true window, distance to the representative's rows, the window's length)
PINNED = ((0, 40, 73), (0, 120, 153))


def true_window(T, lo, hi, site):
    """the stretch of T between the anchors of a site of representative A, exon included"""
    (a0, a1), (b0, b1) = bc.CUTS
    if site == 0:
        assert lo < a0 < hi <= b0 - (a1 - a0)
        return T[lo:hi + (a1 - a0)]
    assert a0 <= lo < b0 - (a1 - a0) < hi
    return T[lo + (a1 - a0):hi + (a1 - a0) + (b1 - b0)]


def host_property(seed=None, **rule):
    """(T, frame, reads, base, qpos, inserts, windows): the property case on the host path"""
    T, reads, _ = bc.property_case(SEED if seed is None else seed)
    frame = ic.representative(T, "A")
    base, ilen, qpos = [], [], []
    for rd in reads:
        ops, _ = api.host_align_ops(rd, frame, gap_open=ic.pc.gap_open(0.1))
        base.append(api.ops_project(ops, rd, len(frame))[0]), ilen.append(api.ops_project_ilen(ops, len(frame))), qpos.append(api.ops_project_qpos(ops, len(frame)))
    base, ilen, qpos = np.array(base, np.uint8), np.array(ilen, np.uint8), np.array(qpos, np.uint32)
    ins = api.planes_inserts(base, ilen)
    return T, frame, reads, base, qpos, ins, host_windows(reads, base, qpos, ins["sites"], ins["reads"]["key"], **rule)


def distances(T, frame, win, seq):
    """per site: (edit distance of the consensus to the true window, to the representative's rows, the consensus' length)"""
    out = []
    for k in range(len(win)):
        lo, hi = int(win[k]["lo"]), int(win[k]["hi"])
        out.append((ipc.edit_distance(seq[k], true_window(T, lo, hi, k)), ipc.edit_distance(seq[k], frame[lo:hi]), len(seq[k])))
    return tuple(out)
