"""What the tests of the variable sites share (test_pile_sites_host.py, test_gpu_pile_sites.py, test_gpu_align_alleles.py,
test_cli_sites.py): plain-Python restatements of the three definitions — ioc_host_ops_project byte by byte, ioc_host_pileup_sites
row by row, ioc_host_site_alleles site by site, in Python's unbounded integers — which are the independent witness for the host
functions and, through them, for the kernels; tables spelled out by hand with the sites they must give; and the builder of the
two-haplotype case, whose answer is known in closed form."""
import random

import numpy as np

from isonclust2_amd import api
from tests import polish_common as pc

NONE, DEL = 7, 5
BASE, INS = 0, 1
M32 = 2**32 - 1
COUNTERS = ("a", "c", "g", "t", "other", "del")
SITE_FIELDS = ("row", "kind", "major", "minor", "depth", "n_major", "n_minor")


def py_project(ops, query, rlen):
    """The walk of ioc_host_ops_project, byte by byte: (base, insf), two lists of rlen + 1 values."""
    base, insf = [NONE] * (rlen + 1), [0] * (rlen + 1)
    r = q = 0
    prev = None
    for op in bytes(ops):
        op = chr(op)
        if op == "d":
            r += 1
        elif op == "i":
            q += 1
        elif op == "D":
            base[r] = DEL
            r += 1
        elif op == "I":
            if prev != "I":
                insf[r] = 1
            q += 1
        else:
            assert op in "=X"
            base[r] = pc.CH.get(query[q], 4)
            r, q = r + 1, q + 1
        prev = op
    assert (q, r) == (len(query), rlen)
    return base, insf


def _need(D, min_alt, min_pct):
    return max(min_alt, (min_pct * D + 99) // 100)


def py_sites(cols, min_depth, min_alt, min_pct, max_sites):
    """ioc_host_pileup_sites, row by row: ([the first max_sites sites as tuples of SITE_FIELDS], n_found)."""
    rlen = len(cols) - 1
    depth = [sum(int(cols[f][p]) for f in COUNTERS) for p in range(rlen + 1)]
    sat = lambda v: min(v, M32)
    found = []
    for p in range(rlen + 1):
        D = depth[p] if p < rlen else (depth[rlen - 1] if rlen else 0)
        w = int(cols["ins_runs"][p])
        wo = D - w if D > w else 0
        if D >= min_depth and w >= _need(D, min_alt, min_pct) and wo >= _need(D, min_alt, min_pct):
            found.append((p, INS, 1, 0, sat(D), sat(w), sat(wo)) if w > wo else (p, INS, 0, 1, sat(D), sat(wo), sat(w)))
        if p == rlen or depth[p] < min_depth:
            continue
        cnt = [int(cols[f][p]) for f in COUNTERS]
        major = cnt.index(max(cnt))
        rest = [(v, ch) for ch, v in enumerate(cnt) if ch != major]
        minor = next(ch for v, ch in rest if v == max(v for v, _ in rest))
        if cnt[minor] >= _need(depth[p], min_alt, min_pct):
            found.append((p, BASE, major, minor, sat(depth[p]), cnt[major], cnt[minor]))
    return found[:max_sites], len(found)


def py_alleles(base, insf, sites):
    """ioc_host_site_alleles, site by site (sites: tuples of SITE_FIELDS, or records)."""
    rlen = len(base) - 1
    out = []
    for s in sites:
        row, kind = int(s[0]), int(s[1])
        if kind == BASE:
            out.append(int(base[row]))
        else:
            spans = base[row] != NONE if row < rlen else (rlen > 0 and base[rlen - 1] != NONE)
            out.append(int(insf[row]) if spans else NONE)
    return out


def as_tuples(sites):
    """An array of PILE_SITE_DTYPE as tuples of SITE_FIELDS (`reserved` must be 0)."""
    assert not np.any(sites["reserved"])
    return [tuple(int(s[f]) for f in SITE_FIELDS) for s in sites]


def table(rows):
    """cols from rows of (a, c, g, t, other, del, ins_runs); ins_bases is not read by the site search."""
    t = np.zeros(len(rows), api.PILEUP_DTYPE)
    for p, r in enumerate(rows):
        for f, v in zip(COUNTERS + ("ins_runs",), r):
            t[f][p] = v
    return t


Z = (0, 0, 0, 0, 0, 0, 0)
# (name, rows of cols (rlen + 1 of them), (min_depth, min_alt, min_pct, max_sites), the sites written, n_found), every expected
# value worked out by hand from the rules in include/isonclust2_hip.h; need(D) = max(min_alt, ceil(min_pct * D / 100))
HAND_SITES = [
    # depth 10 at 25 %: need = max(3, ceil(2.5)) = 3
    ("min_alt_at_equality", [(7, 3, 0, 0, 0, 0, 0), Z], (3, 3, 25, 10), [(0, BASE, 0, 1, 10, 7, 3)], 1),
    ("min_alt_one_below", [(8, 2, 0, 0, 0, 0, 0), Z], (3, 3, 25, 10), [], 0),
    # depth 20 at 25 %: need 5; depth 21: ceil(5.25) = 6
    ("min_pct_at_equality", [(15, 5, 0, 0, 0, 0, 0), Z], (3, 3, 25, 10), [(0, BASE, 0, 1, 20, 15, 5)], 1),
    ("min_pct_one_below", [(16, 4, 0, 0, 0, 0, 0), Z], (3, 3, 25, 10), [], 0),
    ("min_pct_rounds_up", [(16, 5, 0, 0, 0, 0, 0), Z], (3, 3, 25, 10), [], 0),
    # depth 5: need = max(1, ceil(1.25)) = 2
    ("min_depth_at_equality", [(3, 2, 0, 0, 0, 0, 0), Z], (5, 1, 25, 10), [(0, BASE, 0, 1, 5, 3, 2)], 1),
    ("min_depth_one_below", [(3, 2, 0, 0, 0, 0, 0), Z], (6, 1, 25, 10), [], 0),
    # the tie orders: the first maximal counter is the major, the first maximal of the rest the minor
    ("major_tie_first_in_order", [(0, 4, 0, 4, 0, 0, 0), Z], (1, 1, 25, 10), [(0, BASE, 1, 3, 8, 4, 4)], 1),
    ("minor_tie_first_in_order", [(0, 0, 2, 5, 0, 2, 0), Z], (1, 1, 20, 10), [(0, BASE, 3, 2, 9, 5, 2)], 1),
    ("minor_tie_other_before_del", [(6, 0, 0, 0, 3, 3, 0), Z], (1, 1, 25, 10), [(0, BASE, 0, 4, 12, 6, 3)], 1),
    ("all_six_equal", [(2, 2, 2, 2, 2, 2, 0), Z], (1, 1, 10, 10), [(0, BASE, 0, 1, 12, 2, 2)], 1),
    # insertion sites, D = 10, need 3: both sides must reach it; the larger side is the major, a tie goes to "absent"
    ("ins_absent_major", [(10, 0, 0, 0, 0, 0, 4), Z], (3, 3, 25, 10), [(0, INS, 0, 1, 10, 6, 4)], 1),
    ("ins_tie_goes_to_absent", [(10, 0, 0, 0, 0, 0, 5), Z], (3, 3, 25, 10), [(0, INS, 0, 1, 10, 5, 5)], 1),
    ("ins_present_major_without_at_equality", [(10, 0, 0, 0, 0, 0, 7), Z], (3, 3, 25, 10), [(0, INS, 1, 0, 10, 7, 3)], 1),
    ("ins_without_one_below", [(10, 0, 0, 0, 0, 0, 8), Z], (3, 3, 25, 10), [], 0),
    ("ins_with_at_equality", [(10, 0, 0, 0, 0, 0, 3), Z], (3, 3, 25, 10), [(0, INS, 0, 1, 10, 7, 3)], 1),
    ("ins_with_one_below", [(10, 0, 0, 0, 0, 0, 2), Z], (3, 3, 25, 10), [], 0),
    ("ins_depth_one_below", [(10, 0, 0, 0, 0, 0, 5), Z], (11, 3, 25, 10), [], 0),
    # a row with both: the insertion site first
    ("ins_before_base_of_one_row", [(6, 4, 0, 0, 0, 0, 5), Z], (3, 3, 25, 10), [(0, INS, 0, 1, 10, 5, 5), (0, BASE, 0, 1, 10, 6, 4)], 2),
    # row rlen is held against depth(rlen - 1); with > D leaves nothing without
    ("row_rlen_uses_depth_before", [(8, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 3)], (3, 3, 25, 10), [(1, INS, 0, 1, 8, 5, 3)], 1),
    ("with_above_d_at_row_rlen", [(4, 0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 6)], (3, 1, 25, 10), [], 0),
    ("rlen_0", [(0, 0, 0, 0, 0, 0, 9)], (1, 1, 1, 10), [], 0),
    ("rlen_1_nothing", [(1, 0, 0, 0, 0, 0, 0), Z], (1, 1, 1, 10), [], 0),
    # counters of 2^32 - 1 = M: depth 3 M, need at 25 % = (75 M + 99) / 100 = 3221225472 <= M; without = 2 M; the record saturates
    ("counts_2_32", [(M32, M32, 0, 0, 0, M32, M32), Z], (3, 3, 25, 10), [(0, INS, 0, 1, M32, M32, M32), (0, BASE, 0, 1, M32, M32, M32)], 2),
    # ... and at 50 %: need = ceil(1.5 M) > M: nothing (in 32 bits 150 M would have wrapped)
    ("counts_2_32_at_50", [(M32, M32, 0, 0, 0, M32, M32), Z], (3, 3, 50, 10), [], 0),
    ("counts_2_32_every_channel", [(M32,) * 6 + (0,), Z], (1, 1, 50, 10), [], 0),
    ("min_pct_1", [(99, 1, 0, 0, 0, 0, 0), Z], (1, 1, 1, 10), [(0, BASE, 0, 1, 100, 99, 1)], 1),
    ("min_pct_1_needs_2_of_101", [(100, 1, 0, 0, 0, 0, 0), Z], (1, 1, 1, 10), [], 0),
    ("min_pct_50_at_equality", [(5, 5, 0, 0, 0, 0, 0), Z], (1, 1, 50, 10), [(0, BASE, 0, 1, 10, 5, 5)], 1),
    ("min_pct_50_one_below", [(6, 4, 0, 0, 0, 0, 0), Z], (1, 1, 50, 10), [], 0),
    # three sites, the first is kept: n_found says that the list was cut
    ("max_sites_1", [(6, 4, 0, 0, 0, 0, 5), (5, 5, 0, 0, 0, 0, 0), Z], (3, 3, 25, 1), [(0, INS, 0, 1, 10, 5, 5)], 3),
    ("max_sites_2", [(6, 4, 0, 0, 0, 0, 5), (5, 5, 0, 0, 0, 0, 0), Z], (3, 3, 25, 2), [(0, INS, 0, 1, 10, 5, 5), (0, BASE, 0, 1, 10, 6, 4)], 3),
]

# one string by hand: (ops, query, rlen, base, insf); and sites with the alleles that projection has at them
HAND_PROJECTION = (b"d=XIID=i", b"ACGTGA", 5, [NONE, 0, 1, DEL, 2, NONE], [0, 0, 0, 1, 0, 0])
HAND_ALLELES = [((3, BASE), DEL), ((3, INS), 1), ((0, INS), NONE), ((0, BASE), NONE), ((5, INS), 0), ((1, INS), 0), ((4, BASE), 2)]


def other_base(*avoid):
    return next(b for b in b"ACGT" if b not in avoid)


def haplotypes():
    """The two-haplotype case: T is polish_common.anchor()'s T; B differs from it by one substitution (at 40), a deletion of 3
    bases (T[120:123]) and an insertion of 2 bases in front of T[200], chosen so that no equally good alignment moves a gap.
    Returns (T, B, reads): 6 reads equal to T, then 5 equal to B."""
    T = pc.anchor()[0]
    B = bytearray(T[:120] + T[123:200] + bytes([other_base(T[200]), other_base(T[199])]) + T[200:])
    B[40] = other_base(T[40])
    B = bytes(B)
    return T, B, [T] * 6 + [B] * 5


SITES_ON_T = [(40, BASE), (120, BASE), (121, BASE), (122, BASE), (200, INS)]
SITES_ON_B = [(40, BASE), (120, INS), (197, BASE), (198, BASE)]
RULE = dict(min_depth=3, min_alt=3, min_pct=25)


def noisy_haplotypes(seed, rate=0.08):
    """(T, reads): 20 reads of T and then 15 of B, each mutated independently at `rate`."""
    T, B, _ = haplotypes()
    rng = random.Random(seed)
    return T, [pc.mutate(rng, T, rate) for _ in range(20)] + [pc.mutate(rng, B, rate) for _ in range(15)]


def host_sites_and_alleles(frame, reads, e=0.1, max_sites=4096, **rule):
    """Through the host aligner and the host definitions: (cols, sites, n_found, [alleles per read])."""
    rule = {**RULE, **rule}
    cols = np.zeros(len(frame) + 1, api.PILEUP_DTYPE)
    proj = []
    for rd in reads:
        ops, _ = api.host_align_ops(rd, frame, gap_open=pc.gap_open(e))
        api.ops_pileup(ops, rd, len(frame), cols=cols)
        proj.append(api.ops_project(ops, rd, len(frame)))
    sites, found = api.pileup_sites(cols, max_sites=max_sites, **rule)
    return cols, sites, found, [api.site_alleles(b, i, sites) for b, i in proj]


def random_ops(rng, n):
    """(ops, query, rlen): n operation bytes in any order — the definitions walk whatever they are given — and a query to fit."""
    ops = bytes(rng.choice(b"====XXIIDDid") for _ in range(n))
    qlen = sum(ops.count(c) for c in b"=XIi")
    rlen = sum(ops.count(c) for c in b"=XDd")
    return ops, bytes(rng.choice(b"ACGTACGTN") for _ in range(qlen)), rlen
