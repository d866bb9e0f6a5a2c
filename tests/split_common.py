"""What the tests of the split by linked sites share (test_site_split_host.py, test_gpu_site_split.py, test_gpu_align_split.py,
test_cli_split.py): a plain-Python restatement of ioc_host_alleles_split in Python's unbounded integers — the independent witness
for the host function and, through it, for the kernels —; cases spelled out by hand with the values they must give; the tiled
case, which needs the refinement rounds; and generators of random and planted matrices."""
import random

import numpy as np

from isonclust2_amd import api

NONE_GROUP = 255
SEG_FIELDS = ("seed", "n_linked", "n_reads", "n_group0", "n_group1", "n_none", "seed_link")


def sign_at(d, least):
    return 1 if d >= least else -1 if d <= -least else 0


def py_split(minor, major, alleles, min_link, min_margin, rounds):
    """ioc_host_alleles_split, rule by rule.  minor / major: one int per site; alleles: one list of bytes per read.  Returns
    (link, phase, group, vote, seg) as plain lists and a tuple of SEG_FIELDS."""
    ns, nr = len(minor), len(alleles)
    m = [[1 if a[s] == minor[s] else -1 if a[s] == major[s] else 0 for s in range(ns)] for a in alleles]
    d = lambda s, t: sum(r[s] * r[t] for r in m)
    link = [sum(abs(d(s, t)) for t in range(ns) if t != s and abs(d(s, t)) >= min_link) for s in range(ns)]
    if ns == 0 or max(link) == 0:
        return link, [0] * ns, [NONE_GROUP] * nr, [0] * nr, (-1, 0, nr, 0, 0, nr, 0)
    seed = link.index(max(link))
    phase = [1 if t == seed else sign_at(d(seed, t), min_link) for t in range(ns)]

    def votes():
        v = [sum(phase[t] * r[t] for t in range(ns)) for r in m]
        return v, [1 if x >= min_margin else 0 if x <= -min_margin else NONE_GROUP for x in v]

    vote, group = votes()
    for _ in range(rounds):
        g = [1 if x == 1 else -1 if x == 0 else 0 for x in group]
        phase = [sign_at(sum(g[i] * m[i][t] for i in range(nr)), min_link) for t in range(ns)]
        vote, group = votes()
    seg = (seed, sum(p != 0 for p in phase), nr, group.count(0), group.count(1), group.count(NONE_GROUP), link[seed])
    return link, phase, group, vote, seg


def sites_of(minor, major, kind=0):
    """PILE_SITE_DTYPE records with the given alleles (the split reads nothing else of a site)."""
    s = np.zeros(len(minor), api.PILE_SITE_DTYPE)
    s["minor"], s["major"], s["kind"] = minor, major, kind
    s["row"] = np.arange(len(minor))
    return s


def as_lists(out):
    """What api.alleles_split returns, in py_split's form."""
    return (out["link"].tolist(), out["phase"].tolist(), out["group"].tolist(), out["vote"].tolist(), tuple(int(out["seg"][f]) for f in SEG_FIELDS))


def from_marks(rows, n_sites, minor=1, major=0, nothing=7):
    """A matrix from one string per read: '+' the minor, '-' the major, '0' a byte that is neither."""
    assert all(len(r) == n_sites for r in rows)
    return [[{"+": minor, "-": major, "0": nothing}[ch] for ch in r] for r in rows]


N = NONE_GROUP
_CHAIN = ["+00+", "+00+", "-00-", "0+0+", "0+0+", "0-0-", "0++0", "0--0", "0--0"]
# (name, minor per site, major per site, alleles per read, (min_link, min_margin, rounds), link, phase, group, vote, seg), every
# expected value worked out by hand from the rules in include/isonclust2_hip.h.  Alleles: C (1) the minor, A (0) the major
# unless the case says otherwise.
HAND_SPLITS = [
    # d(0, 1) = 3 of three reads that agree
    ("min_link_at_equality", [1, 1], [0, 0], from_marks(["++", "++", "--"], 2), (3, 1, 0), [3, 3], [1, 1], [1, 1, 0], [2, 2, -2], (0, 2, 3, 1, 2, 0, 3)),
    ("min_link_one_below", [1, 1], [0, 0], from_marks(["++", "++", "--"], 2), (4, 1, 0), [0, 0], [0, 0], [N, N, N], [0, 0, 0], (-1, 0, 3, 0, 0, 3, 0)),
    # two reads say + -, one says - +: d = -3, the second site is in opposite phase
    ("negative_d", [1, 1], [0, 0], from_marks(["+-", "+-", "-+"], 2), (3, 1, 0), [3, 3], [1, -1], [1, 1, 0], [2, 2, -2], (0, 2, 3, 1, 2, 0, 3)),
    # votes 2, 2, -2, 1 under a margin of 2: 2 is in, 1 is not
    ("min_margin_at_equality_and_below", [1, 1], [0, 0], from_marks(["++", "++", "--", "+0"], 2), (3, 2, 0), [3, 3], [1, 1], [1, 1, 0, N], [2, 2, -2, 1],
     (0, 2, 4, 1, 2, 1, 3)),
    # d = 5 - 1 = 4; the read that says + - votes 0
    ("vote_0_is_none", [1, 1], [0, 0], from_marks(["++", "++", "++", "--", "--", "+-"], 2), (3, 1, 0), [4, 4], [1, 1], [1, 1, 1, 0, 0, N],
     [2, 2, 2, -2, -2, 0], (0, 2, 6, 2, 3, 1, 4)),
    # a third allele (2), IOC_ALLELE_NONE (7) and a byte outside every table (9) count for nothing: d = 3 from the first three reads
    ("third_allele_and_none", [1, 1], [0, 0], [[1, 1], [1, 1], [0, 0], [2, 1], [7, 0], [1, 9]], (3, 1, 0), [3, 3], [1, 1], [1, 1, 0, 1, 0, 1],
     [2, 2, -2, 1, -1, 1], (0, 2, 6, 2, 4, 0, 3)),
    ("one_site_only", [1], [0], from_marks(["+", "-", "+"], 1), (1, 1, 2), [0], [0], [N, N, N], [0, 0, 0], (-1, 0, 3, 0, 0, 3, 0)),
    ("no_reads", [1, 1], [0, 0], [], (1, 1, 2), [0, 0], [0, 0], [], [], (-1, 0, 0, 0, 0, 0, 0)),
    ("no_sites", [], [], [[], []], (1, 1, 2), [], [], [N, N], [0, 0], (-1, 0, 2, 0, 0, 2, 0)),
    # insertion sites: "present" the minor at the first, "absent" the minor at the second; three reads + +, two - -, one uncovered
    ("insertion_sites", [1, 0], [0, 1], [[1, 0], [1, 0], [1, 0], [0, 1], [0, 1], [7, 7]], (3, 1, 1), [5, 5], [1, 1], [1, 1, 1, 0, 0, N],
     [2, 2, 2, -2, -2, 0], (0, 2, 6, 2, 3, 1, 5)),
    # four sites, no read covers both 0 and 1: d03 = d12 = d13 = 3, the others 0.  link = 3 6 3 6: the tie between 1 and 3 goes to
    # 1.  phase(0) = 0 because d(1, 0) = 0, phase(2) = phase(3) = +1 at equality.  Votes 1 1 -1 2 2 -2 2 -2 -2.
    ("link_tie_and_d_0", [1] * 4, [0] * 4, from_marks(_CHAIN, 4), (3, 1, 0), [3, 6, 3, 6], [0, 1, 1, 1], [1, 1, 0, 1, 1, 0, 1, 0, 0],
     [1, 1, -1, 2, 2, -2, 2, -2, -2], (1, 3, 9, 4, 5, 0, 6)),
    # ... one round: dg(0) = 3 from the first three reads, which site 3 has placed: at equality, site 0 comes in
    ("rephase_at_equality", [1] * 4, [0] * 4, from_marks(_CHAIN, 4), (3, 1, 1), [3, 6, 3, 6], [1, 1, 1, 1], [1, 1, 0, 1, 1, 0, 1, 0, 0],
     [2, 2, -2, 2, 2, -2, 2, -2, -2], (1, 4, 9, 4, 5, 0, 6)),
    # ... the third read does not cover site 0: d03 = 2 (link 0 6 3 3), and dg(0) = 2 is one below: site 0 stays out
    ("rephase_one_below", [1] * 4, [0] * 4, from_marks(_CHAIN[:2] + ["000-"] + _CHAIN[3:], 4), (3, 1, 1), [0, 6, 3, 3], [0, 1, 1, 1],
     [1, 1, 0, 1, 1, 0, 1, 0, 0], [1, 1, -1, 2, 2, -2, 2, -2, -2], (1, 3, 9, 4, 5, 0, 6)),
    # ... and under min_link 4 nothing is linked at all
    ("seed_links_one_below", [1] * 4, [0] * 4, from_marks(_CHAIN, 4), (4, 1, 3), [0] * 4, [0] * 4, [N] * 9, [0] * 9, (-1, 0, 9, 0, 0, 9, 0)),
]

TILED_RULE = dict(min_link=3, min_margin=1)
TILED_NONE = {0: 28, 1: 12, 2: 0, 3: 0}   # reads left unassigned after that many rounds


def tiled():
    """40 base sites on a reference that no read spans: a read covers 10 consecutive sites, reads start every 2 sites, 4 reads
    per start in alternating groups, group 1 carries the minor (C), group 0 the major (A).  Returns (minor, major, alleles,
    truth): 64 reads."""
    ns = 40
    alleles, truth = [], []
    for start in range(0, ns - 10 + 1, 2):
        for j in range(4):
            alleles.append([(j % 2) if start <= s < start + 10 else 7 for s in range(ns)])
            truth.append(j % 2)
    return [1] * ns, [0] * ns, alleles, truth


BYTES = (0, 1, 2, 3, 4, 5, 7, 9)


def random_case(rng, n_reads, n_sites):
    """Any bytes from BYTES, any two different alleles per site."""
    minor, major = [], []
    for _ in range(n_sites):
        a, b = rng.sample(range(6), 2)
        minor.append(a), major.append(b)
    return minor, major, [[rng.choice(BYTES) for _ in range(n_sites)] for _ in range(n_reads)]


def planted_case(rng, n_reads, n_sites, noise=0.1, cover=0.8):
    """Two groups: a read of group 1 carries the minor, one of group 0 the major, at the sites it covers; a byte is replaced by a
    random one at `noise`."""
    minor, major, _ = random_case(rng, 0, n_sites)
    alleles = []
    for i in range(n_reads):
        row = []
        for s in range(n_sites):
            b = (minor[s] if i % 2 else major[s]) if rng.random() < cover else 7
            row.append(rng.choice(BYTES) if rng.random() < noise else b)
        alleles.append(row)
    return minor, major, alleles


def host(minor, major, alleles, min_link, min_margin, rounds):
    """The host function on a case in py_split's form."""
    a = np.array(alleles, np.uint8).reshape(len(alleles), len(minor))
    return as_lists(api.alleles_split(sites_of(minor, major), a, min_link, min_margin, rounds))
