"""What the tests of the alternative ends share: py_ends, a plain restatement of ioc_host_reads_ends from the rules in
include/isonclust2_hip.h; the planted extents of the GPU test, with what each of them is there for; random extents; and the two
property cases — a representative with a class of reads that stops early, one that starts late and a few that start anywhere —
through the host aligner, ioc_host_ops_extent and the host projections."""
import functools
import random

import numpy as np

from isonclust2_amd import api
from tests import blocks_common as bc
from tests import polish_common as pc

DEFAULT = dict(api.ENDS_RULE)
# the rule of the planted case: 35 sites of three reads each among 105 reads are sites only where need(105) is 3
PLANTED = dict(min_pct=2)
E = api.READ_EXTENT_DTYPE
TOP = 2**31 - 1


def need(N, min_alt, min_pct):
    return max(min_alt, (min_pct * N + 99) // 100)


def distance(first, end, x):
    return first - x if x < first else x - end + 1 if x >= end else 0


def py_ends(extents, rlen, pre_group=None, slack=10, min_over=20, min_depth=3, min_alt=3, min_pct=10, max_sites=32, max_variants=64):
    """{rows, starts, stops, variants, reads, seg} of a segment's extents, as arrays of the library's records."""
    ext = np.asarray(extents, E)
    n = len(ext)
    pre = [int(x) for x in pre_group] if pre_group is not None else [0] * n
    part = [int(e["end_row"]) > int(e["first_row"]) for e in ext]
    N = sum(part)
    rows = np.zeros(rlen + 1, api.END_ROW_DTYPE)
    for i in range(n):
        if part[i]:
            rows[int(ext[i]["first_row"])]["starts"] += 1
            rows[int(ext[i]["end_row"])]["stops"] += 1
    for p in range(rlen + 1):
        lo, hi = max(p - slack, 0), min(p + slack, rlen)
        rows[p]["w_starts"], rows[p]["w_stops"] = rows["starts"][lo:hi + 1].sum(), rows["stops"][lo:hi + 1].sum()
    is_row = lambda w: int(N >= min_depth and int(w) >= need(N, min_alt, min_pct))
    out, found, site_of = {}, {}, {}
    for kind, (h, w, at, beyond) in enumerate((("starts", "w_starts", "first_row", "head"), ("stops", "w_stops", "end_row", "tail"))):
        runs = bc._runs([is_row(x) for x in rows[w]], 1)
        kept = runs[:max_sites]
        sites = np.zeros(len(kept), api.END_SITE_DTYPE)
        for b, (a, e) in enumerate(kept):
            counts = rows[h][a:e].astype(np.int64)
            sites[b]["first"], sites[b]["end"], sites[b]["kind"] = a, e, kind
            sites[b]["peak_row"], sites[b]["peak_reads"] = a + int(np.argmax(counts)), int(counts.max())   # (argmax: the lowest on a tie)
        mine = [-1] * n
        for i in range(n):
            if not part[i]:
                continue
            d = [(distance(a, e, int(ext[i][at])), b) for b, (a, e) in enumerate(kept)]
            d = [x for x in d if x[0] <= slack]
            if d:
                mine[i] = min(d)[1]
                sites[mine[i]]["n_reads"] += 1
                sites[mine[i]]["n_over"] += int(ext[i][beyond]) >= min_over
        out[h], found[kind], site_of[kind] = sites, len(runs), mine
    triples = [(pre[i], site_of[0][i], site_of[1][i]) for i in range(n)]
    placed = [t for t in triples if min(t) >= 0]
    supported = sorted(t for t in set(placed) if placed.count(t) >= min_alt)
    kept = supported[:max_variants]
    variants = np.zeros(len(kept), api.END_VARIANT_DTYPE)
    for x, t in enumerate(kept):
        variants[x] = (*t, placed.count(t))
    reads = np.zeros(n, api.READ_ENDS_DTYPE)
    for i in range(n):
        reads[i] = (site_of[0][i], site_of[1][i], kept.index(triples[i]) if min(triples[i]) >= 0 and triples[i] in kept else -1, 0)
    seg = np.zeros(1, api.ENDS_SEG_DTYPE)[0]
    seg["n_reads"], seg["n_starts"], seg["n_starts_found"], seg["n_stops"], seg["n_stops_found"] = N, len(out["starts"]), found[0], len(out["stops"]), found[1]
    seg["n_variants"], seg["n_variants_found"], seg["n_placed"] = len(kept), len(supported), len(placed)
    return dict(rows=rows, starts=out["starts"], stops=out["stops"], variants=variants, reads=reads, seg=seg)


FIELDS = ("seg", "starts", "stops", "variants", "reads", "rows")


def same(got, want, what=""):
    """two results of one segment, as bytes"""
    for f in FIELDS:
        if f in got and f in want:
            assert got[f].tobytes() == want[f].tobytes(), (what, f, got[f], want[f])


def extents(rows):
    """READ_EXTENT_DTYPE records of (first_row, end_row[, head[, tail]]) tuples"""
    return np.array([tuple(r) + (0,) * (4 - len(r)) for r in rows], E) if len(rows) else np.zeros(0, E)


# ---- the planted extents of the GPU test (tests/test_gpu_reads_ends.py; tests/test_reads_ends_host.py measures them) ----
ORDER = (0, 1, 2, 63, 64, 65, 127, 128, 129, 600, 4200, 2000)


def planted_case(seed=9):
    """[(rlen, extents, pre_group)] in segment order: the lengths around the 64 rows of a word and the 64 words of a batch, the
    read counts around the 64 lanes of a member chunk and the four waves of a workgroup.  The rule is PLANTED over the defaults:
    need(N) is 3 for every segment here; the same extents are run at slack 0, 1 and 32, at max_sites 1, at max_variants 2 and at
    min_pct 100."""
    rng = np.random.default_rng(seed)
    X, P = {}, {}
    X[0] = [(0, 0, 5, 5)]                                     # a segment without rows: its one read can take no part
    X[1] = [(0, 1)] * 3                                       # a start site that holds row 0, a stop site that holds row rlen
    X[2] = [(0, 2), (0, 2), (1, 1), (0, 0), (2, 2), (1, 1)]   # N = 2 below min_depth: no sites, and reads that take no part
    # 63: at slack 1 the reads at rows 20, 20 and 22 make row 21 the only start row there, and all three land in [21, 22);
    # reads that take no part; head / tail at min_over - 1 and at min_over
    X[63] = [(0, 63)] * 30 + [(20, 63), (20, 63), (22, 63)] + [(5, 5)] * 10 + [(0, 63, 19, 20)] * 11 + [(0, 63, 20, 19)] * 11
    # 64: start sites [0, 16) and [35, 56) at slack 10 and a read at row 25, ten rows from either: the lower wins; the stop site
    # [20, 41) with a read that stops at row 10, exactly slack below it, and one at row 9, slack + 1: the other stop site is [54, 65)
    X[64] = [(5, 30)] * 5 + [(45, 64)] * 5 + [(25, 64)] + [(0, 10), (0, 9)] + [(5, 30)] * 51
    X[65] = []                                                # a segment without pairs
    # 127: two reads each at rows 63 and 64: at slack 1 the start site [63, 65) lies across two words, at slack 0 there is none;
    # pre_group -1 (never placed) and 2^31 - 1 (the key's high word)
    X[127] = [(63, 127), (63, 127), (64, 127), (64, 127)] + [(0, 127)] * 60
    P[127] = [0] * 4 + [0] * 20 + [TOP] * 20 + [-1] * 17 + [TOP - 1] * 3
    # 128: a stop site at row rlen, the first row of the segment's third word; n_over 10 of the start site, 7 of the stop site
    X[128] = [(0, 128, 19, 0)] * 10 + [(0, 128, 20, 0)] * 10 + [(0, 128, 0, 19)] * 5 + [(0, 128, 0, 20)] * 7 + [(0, 128)] * 33
    # 129: (pre_group 0, start site 1) sorts before (pre_group 1, start site 0): pre_group is the major word; two reads of
    # pre_group 2 are placed and unsupported; max_variants 2 cuts four variants
    X[129] = [(0, 129)] * 40 + [(0, 129)] * 30 + [(60, 129)] * 30 + [(60, 129)] * 28 + [(0, 129)] * 2
    P[129] = [0] * 40 + [1] * 30 + [0] * 30 + [1] * 28 + [2] * 2
    # 600: three classes with ragged ends, and ten reads that start and stop anywhere
    jit = lambda c, n: np.clip(c + rng.integers(-3, 4, n), 0, 600)
    X[600] = ([(a, z, h) for a, z, h in zip(jit(0, 50), jit(600, 50), rng.choice([0, 19, 20, 60], 50))] + [(a, z, 0, t) for a, z, t in zip(jit(0, 40), jit(450, 40), rng.choice([0, 25], 40))]
              + list(zip(jit(200, 30), jit(600, 30))) + [tuple(sorted(rng.integers(0, 601, 2))) for _ in range(10)])
    P[600] = rng.integers(0, 2, 130).tolist()
    # 4200: a start site across rows 4095 | 4096 at slack 1, the 64 words of a batch, and stops scattered around it
    X[4200] = [(4095, 4200), (4095, 4200), (4096, 4200), (4096, 4200)] + [(0, int(z)) for z in rng.integers(4088, 4104, 20)] + [(0, 4200)] * 40
    # 2000: 35 start sites of three reads each, 32 kept: the reads of the last three have no start site
    X[2000] = [(50 * k + 25, 2000) for k in range(35) for _ in range(3)] + [(7, 7)] * 25
    P[2000] = [k % 3 for k in range(35) for _ in range(3)] + [0] * 25
    case = [(r, extents(X[r]), np.array(P[r], np.int32) if r in P else np.zeros(len(X[r]), np.int32)) for r in ORDER]
    assert [len(e) for _, e, _ in case] == [1, 3, 6, 65, 64, 0, 64, 65, 130, 130, 64, 130]
    return case


def interleaved(case):
    """(rlen, seg_of_pair, extents per pair, pre_group per pair, [the pairs of each segment]) with the segments' pairs dealt out in turn"""
    rlen, sop, ext, mine = bc.interleaved([(r, list(e)) for r, e, _ in case])
    pre = np.zeros(len(sop), np.int32)
    for g, (_, _, p) in enumerate(case):
        pre[mine[g]] = p
    return rlen, sop, np.array(ext, E) if ext else np.zeros(0, E), pre, mine


def host_segments(case, with_pre=True, **rule):
    """the host definition of every segment of a case"""
    return [api.host_reads_ends(e, r, pre_group=p if with_pre else None, **{**DEFAULT, **rule}) for r, e, p in case]


def same_as_host(got, want, mine):
    """the device's result of a whole call against the host definition segment by segment, as bytes"""
    for g, w in enumerate(want):
        one = {f: got[f][g] for f in ("seg", "starts", "stops", "variants")}
        one["reads"] = got["reads"][mine[g]]
        if "rows" in got:
            one["rows"] = got["rows"][g]
        same(one, w, g)
    assert int(got["site_off"][-1]) == sum(len(w["starts"]) + len(w["stops"]) for w in want)
    assert int(got["var_off"][-1]) == sum(len(w["variants"]) for w in want)


def random_extents(rng, n, rlen):
    """extents no aligner would produce: a few centres with jitter for either end, reads that take no part, heads and tails around
    min_over, and pre_group of every kind"""
    starts, stops = rng.integers(0, rlen + 1, 3), rng.integers(0, rlen + 1, 3)
    rows = []
    for _ in range(n):
        a = int(np.clip(rng.choice(starts) + rng.integers(-12, 13), 0, rlen)) if rng.random() < 0.8 else int(rng.integers(0, rlen + 1))
        z = int(np.clip(rng.choice(stops) + rng.integers(-12, 13), 0, rlen)) if rng.random() < 0.8 else int(rng.integers(0, rlen + 1))
        a, z = min(a, z), max(a, z)
        rows.append((a, z, int(rng.choice([0, 19, 20, 300])), int(rng.choice([0, 19, 20, 300]))))
    return extents(rows), rng.choice(np.array([-1, 0, 1, 2, TOP], np.int32), n, p=[.1, .4, .3, .1, .1]).astype(np.int32)


# ---- the property cases ----
# A: a representative R of 1500 random bases; 40 reads of R, 40 of R[0:1200] (an early polyadenylation site), 40 of R[250:1500] (a
# late start) and 12 of R[s:1500], s uniform in 0 .. 1000, all mutated independently at 8 % as blocks_common.property_case mutates
# its reads.  B: the same reads against R[100:1500]: the representative itself is the truncated one.
RLEN, CLASS = 1500, 40
STARTS_A, STOPS_A = (0, 250), (1200, 1500)
WHOLE = ((0, 1500), (0, 1200), (250, 1500))   # the three whole classes, 40 reads each, in this order


@functools.lru_cache(maxsize=None)
def property_reads(seed=0, rate=0.08):
    rng = random.Random(seed)
    R = bytes(rng.choice(b"ACGT") for _ in range(RLEN))
    reads = [pc.mutate(rng, R[a:z], rate) for a, z in WHOLE for _ in range(CLASS)]
    reads += [pc.mutate(rng, R[rng.randrange(0, 1001):], rate) for _ in range(12)]
    return R, reads


@functools.lru_cache(maxsize=None)
def property_case(which, seed=0):
    """(frame, reads, [operation strings], extents) of case A or B through the host aligner and ioc_host_ops_extent"""
    R, reads = property_reads(seed)
    frame = R if which == "A" else R[100:]
    ops = [api.host_align_ops(rd, frame, gap_open=pc.gap_open(0.1))[0] for rd in reads]
    return frame, reads, ops, np.array([api.host_ops_extent(o, len(frame)) for o in ops], E)
