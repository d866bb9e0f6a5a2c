"""What the tests of the isoforms' consensus share (test_iso_polish_host.py, test_gpu_planes_polish_groups.py,
test_gpu_align_blocks_polish.py, test_cli_isoforms_polish.py): plain-Python restatements of the grouped member lists and of the
definition of the feature — group-segment (g, h) is pileup_call of frame g on the tables planes_pile adds up from the pairs of
segment g whose group is h —, the property case with its seed, and the edit distance the property is stated in."""
import numpy as np

from isonclust2_amd import api
from tests import blocks_common as bc
from tests import plane_pile_common as pp

# The seed of the property case: the first of 0, 1, 2, .. that meets the four conditions of blocks_common.SEED and the strict
# conditions of the consensus — every isoform's consensus strictly closer (edit distance) to its own true isoform than to any
# other of the four, and closer to it than the representative-frame consensus of the whole cluster is — chosen on the host
# aligner, the host projections and the definition alone (find_seed below).
SEED = bc.SEED
SEEDS_TRIED = bc.SEEDS_TRIED   # blocks_common.SEED is the first that meets the block conditions, and it meets the strict ones


def py_group_member_lists(n_segs, seg_of_pair, group, n_groups):
    """group_member_lists (ioc_sink_plan.h): (gseg_off, gmem_off, gmembers) — the group-segments in segment order, each group's
    pairs in ascending order; a pair in -1, or in a group its segment does not have, is in no list."""
    gseg_off = [0]
    for g in range(n_segs):
        gseg_off.append(gseg_off[-1] + int(n_groups[g]))
    lists = [[] for _ in range(gseg_off[-1])]
    for i, (g, h) in enumerate(zip(seg_of_pair, group)):
        if 0 <= int(h) < int(n_groups[g]):
            lists[gseg_off[g] + int(h)].append(i)
    gmem_off = [0]
    for lst in lists:
        gmem_off.append(gmem_off[-1] + len(lst))
    return gseg_off, gmem_off, [i for lst in lists for i in lst]


def host_groups_polish(frames, seg_of_pair, group, n_groups, base, slots, min_depth):
    """The definition from the host functions, walked through the grouped member lists.  Returns a dict like
    Context.planes_polish_groups' with tables=True."""
    ns = len(frames)
    gseg_off, gmem_off, gmembers = py_group_member_lists(ns, seg_of_pair, group, n_groups)
    gseq, gqual, gpol, gcols, gins, grow0 = [], [], [], [], [], []
    rows = 0
    for g, frame in enumerate(frames):
        gseq.append([]), gqual.append([])
        pol = np.zeros(int(n_groups[g]), api.POLISH_STATS_DTYPE)
        for h in range(int(n_groups[g])):
            x = gseg_off[g] + h
            cols, ins = np.zeros(len(frame) + 1, api.PILEUP_DTYPE), np.zeros(len(frame) + 1, api.PILEUP_INS_DTYPE)
            for i in gmembers[gmem_off[x]:gmem_off[x + 1]]:
                api.planes_pile(base[i], slots[i], cols=cols, ins=ins)
            s, q, st = api.pileup_call(cols, ins, frame, min_depth)
            gseq[g].append(s), gqual[g].append(q)
            for f in api.POLISH_STATS_FIELDS:
                pol[h][f] = st[f]
            gcols.append(cols), gins.append(ins), grow0.append(rows)
            rows += len(frame) + 1
        gpol.append(pol)
    cat = lambda parts, dt: np.concatenate([np.zeros(0, dt)] + parts)
    return {"gseq": gseq, "gqual": gqual, "gpolish": gpol, "gseg_off": np.array(gseg_off, np.int64), "gcols": cat(gcols, api.PILEUP_DTYPE),
            "gins": cat(gins, api.PILEUP_INS_DTYPE), "grow0": np.array(grow0, np.int64)}


def same_groups(got, want, tables=True):
    """a result of Context.planes_polish_groups (or the isoform part of align_pairs_blocks_polish) against the definition, as bytes"""
    assert got["gseq"] == want["gseq"] and got["gqual"] == want["gqual"]
    assert got["gseg_off"].tolist() == want["gseg_off"].tolist()
    assert len(got["gpolish"]) == len(want["gpolish"])
    for a, b in zip(got["gpolish"], want["gpolish"]):
        assert a.tobytes() == b.tobytes()
    if tables:
        assert got["gcols"].tobytes() == want["gcols"].tobytes() and got["gins"].tobytes() == want["gins"].tobytes()
        assert got["grow0"].tolist() == want["grow0"].tolist()


def edit_distance(a, b):
    """the unit-cost edit distance of two byte strings (rows of the table as numpy arrays: the insertions by a running minimum)"""
    a, b = np.frombuffer(bytes(a), np.uint8), np.frombuffer(bytes(b), np.uint8)
    prev = np.arange(len(b) + 1, dtype=np.int64)
    idx = np.arange(len(b) + 1, dtype=np.int64)
    for i in range(len(a)):
        cur = np.empty_like(prev)
        cur[0] = i + 1
        cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (b != a[i]))
        cur = np.minimum.accumulate(cur - idx) + idx   # cur[j] = min over j' <= j of cur[j'] + (j - j')
        prev = cur
    return int(prev[-1])


def true_isoforms(T):
    (a0, a1), (b0, b1) = bc.CUTS
    return [T, T[:a0] + T[a1:], T[:a0] + T[a1:b0] + T[b1:], T[:b0] + T[b1:]]


def host_planes(frame, reads, e=0.1):
    """every read's (base plane, slot planes) through the host aligner and both host projections"""
    base, slots = [], []
    for rd in reads:
        ops, _ = api.host_align_ops(rd, frame, gap_open=bc.pc.gap_open(e))
        b, s = pp.planes_of(ops, rd, len(frame))
        base.append(b), slots.append(s)
    return base, slots


def property_distances(seed, min_depth=3):
    """The property case through the host pipeline: host aligner, host planes, api.planes_blocks, the definition.  Returns
    (blocks result, consensus per isoform, dist) with dist[h][x] the edit distance of isoform h's consensus to true isoform x, and
    whole[x] the distance of the representative-frame consensus of the whole cluster to true isoform x."""
    T, reads, true = bc.property_case(seed)
    base, slots = host_planes(T, reads)
    got = api.planes_blocks(np.array(base, np.uint8))
    ng = int(got["seg"]["n_groups"])
    want = host_groups_polish([T], [0] * len(reads), got["reads"]["group"].tolist(), [ng], base, slots, min_depth)
    iso = true_isoforms(T)
    cons = want["gseq"][0]
    dist = [[edit_distance(c, t) for t in iso] for c in cons]
    one = host_groups_polish([T], [0] * len(reads), [0] * len(reads), [1], base, slots, min_depth)["gseq"][0][0]
    whole = [edit_distance(one, t) for t in iso]
    return got, true, cons, dist, whole


# The isoforms are numbered by ascending key (state at block 0 + 4 * state at block 1): keep/keep 0, skip/keep 1, keep/skip 4,
# skip/skip 5 — so isoform h of the library is true isoform TRUE_OF[h] of property_case, whose list has skip/skip third.
TRUE_OF = (0, 1, 3, 2)


# What the host path gives on the property case at SEED (measured on the host aligner, the host projections, api.planes_blocks and
# the definition; test_iso_polish_host.py pins them as equalities): DIST[h][x] is the edit distance of isoform h's consensus to true
# isoform x, OWN[h] = DIST[h][TRUE_OF[h]] that to its own; WHOLE[x] that of the representative-frame consensus of the whole cluster.
DIST = ((0, 40, 160, 120), (40, 0, 120, 160), (119, 159, 41, 1), (161, 121, 1, 41))
OWN = (0, 0, 1, 1)
WHOLE = (14, 30, 146, 130)


def strict_holds(dist, whole):
    """every isoform's consensus strictly closer to its own true isoform than to any other, and closer than the whole cluster's is"""
    if len(dist) != 4:
        return False
    own = [dist[h][TRUE_OF[h]] for h in range(4)]
    return all(own[h] < min(dist[h][x] for x in range(4) if x != TRUE_OF[h]) and own[h] < whole[TRUE_OF[h]] for h in range(4))


def find_seed(limit=50):
    """the first seed at which the four block conditions and the strict conditions hold, and how many were tried"""
    for seed in range(limit):
        got, true, _, dist, whole = property_distances(seed)
        if all(bc.property_holds(got, true)) and strict_holds(dist, whole):
            return seed, seed + 1
    raise AssertionError("no seed")
