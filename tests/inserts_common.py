"""What the tests of the insertion sites share: py_inserts, a plain restatement of ioc_host_planes_inserts from the rules in
include/isonclust2_hip.h; the planted planes of the GPU test, with what each of them is there for; and the two property cases —
the reads of blocks_common.property_case against a representative that lacks both exons (A) or the first one only (B) — through the
host aligner and the host projections."""
import numpy as np

from isonclust2_amd import api
from tests import blocks_common as bc
from tests import polish_common as pc

DEL, NONE = api.ALLELE_DEL, api.ALLELE_NONE
LACK, CARRY, NOT = api.INS_LACK, api.INS_CARRY, api.INS_NONE
DEFAULT = dict(api.INSERTS_RULE)
M64 = 2**64 - 1


def py_inserts(base, ilen, pre_key=None, pre_mask=None, pre_full=0, min_ins=20, slack=8, min_depth=3, min_alt=3, min_pct=25, max_sites=32):
    """(rows, sites, reads, seg) of n_reads x (rlen + 1) bytes of each kind of plane, as arrays of the library's records."""
    base, ilen = np.asarray(base, np.uint8), np.asarray(ilen, np.uint8)
    n, rlen = base.shape[0], base.shape[1] - 1
    pk = [int(x) for x in pre_key] if pre_key is not None else [0] * n
    pm = [int(x) for x in pre_mask] if pre_key is not None else [0] * n
    pre_full = int(pre_full) if pre_key is not None else 0
    covers = base[:, :rlen] <= DEL
    junctions = range(1, rlen)   # 1 .. rlen - 1
    spans = np.zeros((n, rlen + 1), bool)
    W = np.zeros((n, rlen + 1), np.int64)
    for p in junctions:
        spans[:, p] = covers[:, p - 1] & covers[:, p]
    for p in range(rlen + 1):
        W[:, p] = ilen[:, max(p - slack, 0):min(p + slack, rlen) + 1].astype(np.int64).sum(axis=1)
    near = spans & (W >= min_ins)
    rows = np.zeros(rlen + 1, api.INSERT_ROW_DTYPE)
    rows["span"], rows["in_ins"] = spans.sum(axis=0), near.sum(axis=0)
    variable = [int(s >= min_depth and g >= bc.need(s, min_alt, min_pct) and s - g >= bc.need(s, min_alt, min_pct))
                for s, g in zip(rows["span"].tolist(), rows["in_ins"].tolist())]
    found = bc._runs(variable, 1)
    kept = found[:max_sites]
    sites = np.zeros(len(kept), api.PILE_INSERT_DTYPE)
    reads = np.zeros(n, api.READ_INSERTS_DTYPE)
    keys, masks = [0] * n, [0] * n
    for b, (a, e) in enumerate(kept):
        sites[b]["first"], sites[b]["end"] = a, e
        longest = []
        for i in range(n):
            st = NOT if not spans[i, a:e].all() else CARRY if near[i, a:e].any() else LACK
            keys[i] |= st << (2 * b)
            masks[i] |= 0 if st == NOT else 3 << (2 * b)
            sites[b][{CARRY: "n_carry", LACK: "n_lack", NOT: "n_none"}[st]] += 1
            if st == CARRY:
                longest.append(int(W[i, a:e].max()))
        sites[b]["len_min"], sites[b]["len_max"] = (min(longest), max(longest)) if longest else (0, 0)
    full = (1 << (2 * len(kept))) - 1
    complete = [(pk[i], keys[i]) for i in range(n) if masks[i] == full and pm[i] == pre_full]
    supported = sorted(k for k in set(complete) if complete.count(k) >= min_alt)   # (tuples of Python integers: unsigned, pre word major)
    seg = np.zeros(1, api.INSERTS_SEG_DTYPE)[0]
    seg["n_sites"], seg["n_found"], seg["n_groups"], seg["n_reads"] = len(kept), len(found), len(supported), n
    for i in range(n):
        reads[i]["key"] = keys[i]
        reads[i]["n_near"] = int(near[i].sum())
        reads[i]["ins_bases"] = int(ilen[i][spans[i]].astype(np.int64).sum())
        mine = (pk[i], keys[i])
        if masks[i] == full and pm[i] == pre_full:
            group, how = (supported.index(mine), api.ISO_DIRECT) if mine in supported else (-1, api.ISO_RARE)
        else:
            agree = [g for g, (a, k) in enumerate(supported) if (a ^ pk[i]) & pm[i] == 0 and (k ^ keys[i]) & masks[i] == 0] if masks[i] | pm[i] else []
            group, how = (agree[0], api.ISO_ASSIGNED) if len(agree) == 1 else (-1, api.ISO_AMBIGUOUS)
        reads[i]["group"], reads[i]["how"] = group, how
        seg[("n_direct", "n_assigned", "n_rare", "n_ambiguous")[how]] += 1
    return rows, sites, reads, seg


def same_as_py(got, base, ilen, pre=None, **rule):
    """a result of api.planes_inserts (or one segment of the device's) against py_inserts, as bytes; returns py_inserts' tuple"""
    pk, pm, pf = pre if pre is not None else (None, None, 0)
    rows, sites, reads, seg = py_inserts(base, ilen, pk, pm, pf, **{**DEFAULT, **rule})
    assert got["seg"].tobytes() == seg.tobytes(), (got["seg"], seg)
    assert got["sites"].tobytes() == sites.tobytes(), (got["sites"], sites)
    assert got["reads"].tobytes() == reads.tobytes()
    if "rows" in got:
        assert got["rows"].tobytes() == rows.tobytes()
    return rows, sites, reads, seg


def states(reads, n_sites):
    """every read's states at the kept sites, from its key"""
    return [[(int(k) >> (2 * b)) & 3 for b in range(n_sites)] for k in reads["key"]]


# ---- the planted planes of the GPU test (tests/test_gpu_planes_inserts.py; tests/test_planes_inserts_host.py measures them) ----
PRE_X, PRE_Y, PRE_Z = 2**63 + 1, 1, 0   # block words of the segment of 600 rows: X has bit 63, so it sorts behind Y only unsigned


def _covered(rng, n, rlen):
    p = rng.integers(0, 5, (n, rlen + 1)).astype(np.uint8)
    p[:, rlen] = NONE
    return p


def planted_case(seed=7):
    """[(rlen, base planes, length planes, (pre_key, pre_mask, pre_full))] in segment order: the lengths around the 64 junctions of a
    word and the 64 words of a batch, the pair counts around the 64 lanes of a member chunk and the four waves of a workgroup.  The
    default rule: 20 bases within 8 junctions; with 64 or 65 reads need(S) is 16 or 17, with 130 it is 33.  The same planes are run
    at slack 0 and at slack 32."""
    rng = np.random.default_rng(seed)
    B, L, pre = {}, {}, {}
    for rlen, n in ((0, 1), (1, 3), (2, 6), (63, 65), (64, 64), (65, 0), (127, 64), (128, 65), (129, 130), (600, 130), (4200, 64), (2000, 64)):
        B[rlen], L[rlen] = _covered(rng, n, rlen), np.zeros((n, rlen + 1), np.uint8)
        pre[rlen] = (np.zeros(n, np.uint64), np.zeros(n, np.uint64), 0)
    L[0][0, 0] = 200                                        # a segment without rows: one length byte, no junction
    L[1][:, 0], L[1][:, 1] = 30, 30                         # rows 0 and rlen of a segment without junctions
    L[2][:3, 1] = 25                                        # one junction, 3 of 6 reads carry: a site at junction 1 that ends at rlen - 1
    L[63][:20, 0] = 25                                      # a byte at row 0: junctions 1 .. 8 see it at slack 8, none at slack 0
    L[63][20:40, 63] = 25                                   # a byte at row rlen: junctions 55 .. 62, a site that ends at rlen - 1
    L[64][:20, :] = 255                                     # 255 throughout every window: 65 x 255 at slack 32; a site [1, 64)
    b, l = B[127], L[127]
    l[:20, 60], l[:20, 66] = 12, 12                         # 12 + 12 six rows apart: near at 58 .. 68 (slack 8), across 63 | 64
    b[30, 80:90], l[30, 85] = NONE, 40                      # a length byte at junctions the read does not span
    b[31, 70], b[32, 71] = 6, 0xEE                          # bytes no projection writes cover nothing
    l[40:43, 100] = 20                                      # min_alt carriers of min_ins bases: need(64) is 16, no site
    L[128][:20, 64], L[128][20:23, 64] = 20, 19             # exactly min_ins at a word's first junction, and one fewer
    L[129][:40, 128], L[129][40:80, 129] = 30, 30           # junction rlen - 1, and row rlen seen from 121 .. 128: a site [120, 129)
    b, l, n = B[600], L[600], 130                           # sites A around junction 100 and B around 300
    l[40:100, 100], l[70:112, 300] = 40, 40                 # 40 lack both, 30 carry A, 30 both, 12 carry B
    pk, pm = np.full(n, PRE_Y, np.uint64), np.full(n, M64, np.uint64)
    pk[20:40] = PRE_X                                       # the same insert word under another block word: bit 63
    pk[112:115] = PRE_Z                                     # exactly min_alt carriers of (Z, lack lack)
    pk[115:117] = 2                                         # min_alt - 1 carriers of (2, lack lack): rare
    b[117, :120], l[117, 300] = NONE, 40                    # no state at A, carries B under Y: (Y, both) and (Y, B) agree
    b[118, :120], l[118, 300], pk[118] = NONE, 40, PRE_X    # ... under X: nothing agrees
    b[119, :120], pk[119] = NONE, PRE_X                     # no state at A, lacks B under X: (X, lack lack) alone
    l[120, 100], pm[120] = 40, 0                            # carries A, no block word: (Y, A) alone
    pm[121] = 0                                             # lacks both, no block word: three pairs agree
    b[122, :], pm[122] = NONE, 0                            # no state anywhere
    b[123, :], pk[123] = NONE, PRE_X                        # covers nothing, a complete block word X: (X, lack lack) alone
    pre[600] = (pk, pm, M64)
    l = L[4200]
    l[:20, 4090], l[:20, 4100] = 12, 12                     # near at 4092 .. 4098: across 4095 | 4096, the 64 words of a batch
    l[:20, 2000] = 255
    b, l = B[2000], L[2000]                                 # 35 sites, 32 kept; reads 0 .. 19 carry all, 20 .. 39 all but site 31
    for k in range(35):
        l[:20, 50 * k + 25] = 30
        if k != 31:
            l[20:40, 50 * k + 25] = 30
    b[63, 1560:1600] = NONE                                 # no state at site 31: bit 63 of the key
    return [(rlen, B[rlen], L[rlen], pre[rlen]) for rlen in (0, 1, 2, 63, 64, 65, 127, 128, 129, 600, 4200, 2000)]


def interleaved(case):
    """(rlen, seg_of_pair, [base plane per pair], [length plane per pair], pre_key, pre_mask, pre_full, [the pairs of each segment])
    with the segments' pairs dealt out in turn"""
    rlen, sop, planes, mine = bc.interleaved([(r, b) for r, b, _, _ in case])
    _, _, lens, _ = bc.interleaved([(r, l) for r, _, l, _ in case])
    pk, pm = np.zeros(len(sop), np.uint64), np.zeros(len(sop), np.uint64)
    for g, (_, _, _, (k, m, _)) in enumerate(case):
        pk[mine[g]], pm[mine[g]] = k, m
    return rlen, sop, planes, lens, pk, pm, np.array([c[3][2] for c in case], np.uint64), mine


def host_segments(case, with_pre=True, **rule):
    """the host definition of every segment of a case"""
    out = []
    for r, b, l, (pk, pm, pf) in case:
        kw = dict(pre_key=pk, pre_mask=pm, pre_full=pf) if with_pre else {}
        out.append(api.planes_inserts(b.reshape(-1, r + 1), l.reshape(-1, r + 1), **kw, **{**DEFAULT, **rule}))
    return out


def same_as_host(got, want, mine):
    """the device's result of a whole call against the host definition segment by segment, as bytes"""
    for g, w in enumerate(want):
        assert got["seg"][g].tobytes() == w["seg"].tobytes(), (g, got["seg"][g], w["seg"])
        assert got["sites"][g].tobytes() == w["sites"].tobytes(), (g, got["sites"][g], w["sites"])
        assert got["reads"][mine[g]].tobytes() == w["reads"].tobytes(), g
        if "rows" in got:
            assert got["rows"][g].tobytes() == w["rows"].tobytes(), g
    assert int(got["site_off"][-1]) == sum(len(w["sites"]) for w in want)


def random_planes(rng, n, rlen):
    """planes no aligner would produce: every base byte that matters, and length bytes of every size at random"""
    b = bc.random_planes(rng, n, rlen, p_gap=0.2)
    l = rng.choice(np.array([0, 1, 3, 9, 19, 20, 40, 254, 255], np.uint8), (n, rlen + 1), p=[.9, .03, .02, .015, .01, .01, .005, .005, .005])
    return b, l


def random_pre(rng, n):
    """block words and masks at random: a few values, so that pairs repeat; most masks complete"""
    full = (0xF, M64, 0)[int(rng.integers(0, 3))]
    pk = np.array([(0, 1, 4, 5, 2**63 + 1)[int(x)] & full for x in rng.integers(0, 5, n)], np.uint64)
    pm = np.array([full if x < 0.8 else full & 3 for x in rng.random(n)], np.uint64)
    return pk, pm, full


# ---- the property cases ----
# The reads are those of blocks_common.property_case(seed).  A: the representative is the isoform that lacks [150, 190) and [400,
# 520), so both exons are insertions, at junctions 150 and 360.  B: it lacks [150, 190) only; [400, 520) is a block at [360, 480)
# and the first exon an insertion at junction 150.
JUNCTIONS_A = (150, 360)
TRUE_A = ((CARRY, CARRY), (LACK, CARRY), (LACK, LACK), (CARRY, LACK))           # per isoform of property_case, at the two sites
TRUE_B = ((bc.KEEP, CARRY), (bc.KEEP, LACK), (bc.SKIP, LACK), (bc.SKIP, CARRY))  # ... (state at the block, state at the site)
# The first seed from 0 at which each property holds on the host aligner and the host projections (find_seeds below).
SEED_A, SEEDS_TRIED_A = 0, 1
SEED_B, SEEDS_TRIED_B = 0, 1


def representative(T, which):
    (a0, a1), (b0, b1) = bc.CUTS
    return T[:a0] + T[a1:b0] + T[b1:] if which == "A" else T[:a0] + T[a1:]


def host_planes(frame, reads, e=0.1):
    """every read's base plane and length plane through the host aligner, ioc_host_ops_project and ioc_host_ops_project_ilen"""
    base, ilen = [], []
    for rd in reads:
        ops, _ = api.host_align_ops(rd, frame, gap_open=pc.gap_open(e))
        base.append(api.ops_project(ops, rd, len(frame))[0])
        ilen.append(api.ops_project_ilen(ops, len(frame)))
    return np.array(base, np.uint8), np.array(ilen, np.uint8)


def true_of_reads():
    return [x for x, n in enumerate(bc.SIZES) for _ in range(n)]   # the isoform of each of the 38 complete reads


def property_a_holds(got):
    """(exactly two sites, each holds its junction, all 38 complete reads in their true state, four isoforms) of a result on A"""
    sites, seg = got["sites"], got["seg"]
    two = int(seg["n_found"]) == 2 and len(sites) == 2
    holds = two and all(int(sites[b]["first"]) <= JUNCTIONS_A[b] < int(sites[b]["end"]) for b in range(2))
    st = states(got["reads"], 2) if two else []
    right = two and all(tuple(st[i]) == TRUE_A[x] for i, x in enumerate(true_of_reads()))
    return two, holds, right, int(seg["n_groups"]) == 4


def property_b_holds(blocks, got):
    """(the block stage alone reports 2 isoforms, blocks and sites together 4, every complete read in its true one) on B"""
    alone = int(blocks["seg"]["n_groups"]) == 2
    four = int(got["seg"]["n_groups"]) == 4
    want = sorted(range(4), key=lambda x: TRUE_B[x])   # the isoforms in ascending order of (block word, insert word)
    right = int(blocks["seg"]["n_blocks"]) == 1 and int(got["seg"]["n_sites"]) == 1 and all(
        int(got["reads"][i]["how"]) == api.ISO_DIRECT and int(got["reads"][i]["group"]) == want.index(x) for i, x in enumerate(true_of_reads()))
    return alone, four, right


def run_a(seed, py=False, **rule):
    T, reads, _ = bc.property_case(seed)
    base, ilen = host_planes(representative(T, "A"), reads)
    if py:
        rows, sites, rd, seg = py_inserts(base, ilen, **{**DEFAULT, **rule})
        return base, ilen, dict(rows=rows, sites=sites, reads=rd, seg=seg)
    return base, ilen, api.planes_inserts(base, ilen, **rule)


def run_b(seed):
    T, reads, _ = bc.property_case(seed)
    base, ilen = host_planes(representative(T, "B"), reads)
    blocks = api.planes_blocks(base)
    mask = np.array([sum(3 << (2 * b) for b in range(len(blocks["blocks"])) if (int(k) >> (2 * b)) & 3 != bc.NOT) for k in blocks["reads"]["key"]], np.uint64)
    full = (1 << (2 * len(blocks["blocks"]))) - 1
    return base, ilen, blocks, (blocks["reads"]["key"].copy(), mask, full), api.planes_inserts(base, ilen, pre_key=blocks["reads"]["key"], pre_mask=mask, pre_full=full)


def find_seeds(limit=6):
    """the first seed at which each property holds, and how many were tried"""
    a = next(s for s in range(limit) if all(property_a_holds(run_a(s)[2])))
    b = next(s for s in range(limit) if all(property_b_holds(*(lambda r: (r[2], r[4]))(run_b(s)))))
    return (a, a + 1), (b, b + 1)
