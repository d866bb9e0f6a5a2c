"""The kernels of ioc_window_variants.hip against the host definition, as bytes, through ioc_planes_insert_window_variants: the
agreement at the chunk edges of a lane per template row, both rounds; sites of 1, 64, 65 and 130 voters, the member chunks of the
ballots and of the rank loop; the planted segment between segments of 0, 1 and 32 sites; a round B whose direction words cross the
per-launch limit; the property case; the refusals against canaries and the empty call."""
import ctypes as C

import numpy as np
import pytest

from isonclust2_amd import api
from tests import variants_common as vc
from tests import windows_common as wc

pytestmark = pytest.mark.gpu

CARRY = api.INS_CARRY


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _rand(rng, n):
    return bytes(b"ACGT"[x] for x in rng.integers(0, 4, n))


def _mutate(rng, s, rate):
    out = bytearray()
    for c in s:
        u = rng.random()
        if u < rate / 3:
            continue
        out.append(b"ACGT"[int(rng.integers(0, 4))] if u < 2 * rate / 3 else c)
        if u > 1 - rate / 3:
            out.append(b"ACGT"[int(rng.integers(0, 4))])
    return bytes(out) or b"A"


def _site_of_windows(windows):
    """a segment of 8 rows with ONE site whose carriers hold exactly `windows` between the anchors at slack 0 (test_gpu_insert_windows
    has the same): (rlen, reads, base, qpos, sites, keys)"""
    rlen = 8
    reads, base, qpos = [], [], []
    for w in windows:
        rd = b"CCCC" + w + b"GGG"
        ops = b"====" + b"I" * (len(w) - 1) + b"=" + b"==="
        reads.append(rd), base.append(api.ops_project(ops, rd, rlen)[0]), qpos.append(api.ops_project_qpos(ops, rlen))
    sites = np.zeros(1, api.PILE_INSERT_DTYPE)
    sites[0]["first"], sites[0]["end"] = 4, 5
    return rlen, reads, base, qpos, sites, np.full(len(windows), CARRY, np.uint64)


def _run(ctx, segments, min_depth=1, pre=None, **rule):
    """segments: (rlen, reads, base, qpos, sites, keys) each; their pairs interleaved in one call, against the host definition segment
    by segment and the host recount over its key2 / mask2.  pre: (pre_key, pre_mask, pre_full) per segment, or None."""
    seqs, sop, query, base, qpos, keys, mine = [], [], [], [], [], [], [[] for _ in segments]
    left = [list(range(len(s[1]))) for s in segments]
    while any(left):
        for g, s in enumerate(segments):
            if left[g]:
                i = left[g].pop(0)
                mine[g].append(len(sop))
                sop.append(g), query.append(len(seqs)), seqs.append(s[1][i]), base.append(s[2][i]), qpos.append(s[3][i]), keys.append(int(s[5][i]))
    n = len(sop)
    kw = {}
    if pre is not None:
        pk, pm = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        for g, (k, m, _) in enumerate(pre):
            pk[mine[g]], pm[mine[g]] = k, m
        kw = dict(pre_key=pk, pre_mask=pm, pre_full=np.array([p[2] for p in pre], np.uint64))
    ctx.align_set_pool(seqs + [b"ACGT"])
    got = ctx.planes_insert_window_variants([s[0] for s in segments], sop, query, base, qpos, [s[4] for s in segments], keys, min_depth=min_depth, **kw, **rule)
    r = {**vc.RULE, **rule}
    x = 0
    for g, s in enumerate(segments):
        m, S, nr = np.array(mine[g], np.int64), len(s[4]), len(s[1])
        want = api.insert_window_variants(np.array(s[2]).reshape(nr, s[0] + 1), np.array(s[3]).reshape(nr, s[0] + 1), [len(rd) for rd in s[1]], s[4], s[5], s[1],
                                          min_depth=min_depth, **rule)
        for k in range(S):
            for f in ("lo", "hi", "tlen", "n_voters", "n_short", "n_long", "reserved"):
                assert int(got["win"][x][f]) == int(want["win"][k][f]), (g, k, f)
            for f in ("split", "tlen_b", "n_a", "n_b", "n_other", "n_far", "reserved"):
                assert int(got["var"][x][f]) == int(want["var"][k][f]), (g, k, f, got["var"][x], want["var"][k])
            for rec, f in (("win", "template_pair"), ("var", "template_pair_b")):
                t = int(want[rec][k][f])
                assert int(got[rec][x][f]) == (mine[g][t] if t >= 0 else -1), (g, k, f)
            for h in range(2):
                assert (got["seq"][2 * x + h], got["qual"][2 * x + h]) == (want["seq"][2 * k + h], want["qual"][2 * k + h]), (g, k, h)
                assert got["polish"][2 * x + h].tobytes() == want["polish"][2 * k + h].tobytes(), (g, k, h)
            x += 1
        assert got["variant"][m][:, :S].tobytes() == want["variant"].tobytes() and (got["variant"][m][:, S:] == 0).all(), g
        assert got["agree"][m][:, :S].tobytes() == want["agree"].tobytes() and (got["agree"][m][:, S:] == vc.NO).all(), g
        assert got["reads"]["key2"][m].tobytes() == want["key2"].tobytes(), g
        p = dict(pre_key=pre[g][0], pre_mask=pre[g][1], pre_full=pre[g][2]) if pre is not None else {}
        grp, how, c = api.key_isoforms(want["key2"], want["mask2"], (1 << (2 * S)) - 1, r["min_alt"], **p)
        assert got["reads"]["group"][m].tolist() == grp.tolist() and got["reads"]["how"][m].tolist() == how.tolist(), g
        rec = got["seg"][g]
        assert [int(rec[f]) for f in ("n_sites", "n_split", "n_groups", "n_reads", "n_direct", "n_assigned", "n_rare", "n_ambiguous")] == [
            S, int(want["var"]["split"].sum()), c["n_groups"], nr, c["n_direct"], c["n_assigned"], c["n_rare"], c["n_ambiguous"]], (g, rec)
    assert x == len(got["win"]) and int(got["off"][-1]) == sum(len(s) for s in got["seq"])
    return got


LENGTHS = (1, 63, 64, 65, 128, 129, 512)


def test_the_agreement_at_the_chunk_edges_in_both_rounds(ctx):
    """every template length x every voter length of LENGTHS: a segment per combination with three carriers, the template twice and a
    voter mutated at 8 % or unrelated.  At min_alt 1 and min_pct 1 need is 1, so an unrelated voter is far, round B runs with that
    voter as template B — the same lengths in round B — and the site splits 2 / 1.  The host's agreements are ioc_host_ops_agreement of
    the host alignments."""
    rng = np.random.default_rng(29)
    segments = []
    for t in LENGTHS:
        core = _rand(rng, t)
        for n in LENGTHS:
            near = _mutate(rng, (core * (n // t + 1))[:n], 0.08)[:n].ljust(n, b"G")
            for other in (near, _rand(rng, n)):
                segments.append(_site_of_windows([core, core, other] if n >= t else [other, core, core]))
    got = _run(ctx, segments, max_win=512, slack=0, min_alt=1, min_pct=1)
    assert int(got["var"]["split"].sum()) >= len(LENGTHS) ** 2 - 10   # (two unrelated strings of one base may be equal)
    assert (got["agree"][:, 0, 0] != vc.NO).all() and int((got["agree"][:, 0, 1] != vc.NO).sum()) >= len(LENGTHS) ** 2 - 10


def test_sites_of_one_to_a_hundred_and_thirty_voters(ctx):
    """1, 64, 65 and 130 voters of two exons in turn, and 130 of which every fifth holds an exon of its own: the ballots and the rank
    loop of k_win_template_far and k_win_decide take the members 64 at a time"""
    rng = np.random.default_rng(37)
    P, Q = _rand(rng, 40), _rand(rng, 34)
    segments = [_site_of_windows([_mutate(rng, P if i % 2 == 0 else Q, 0.05) for i in range(n)]) for n in (1, 64, 65, 130)]
    segments.append(_site_of_windows([_mutate(rng, P if i % 2 else Q, 0.05) if i % 5 else _rand(rng, 30 + i % 7) for i in range(130)]))
    got = _run(ctx, segments, min_depth=3, max_win=64, slack=0)
    assert got["var"]["split"].tolist() == [0, 1, 1, 1, 1] and int(got["var"][4]["n_other"]) >= 20
    assert [int(x) for x in got["var"]["n_far"][:4]] == [0, 32, 32, 65]


def _many_sites(rng, n_sites=32):
    """a segment of 2000 rows and 32 sites, a site every 50 rows, ten carriers each: two exons in turn at the even sites"""
    P, Q = _rand(rng, 30), _rand(rng, 24)
    ins = [[vc._nudge(rng, P if (i % 2 == 0 or k % 2) else Q) for k in range(n_sites)] for i in range(10)] + [[b""] * n_sites for _ in range(4)]
    reads, base, qpos, sites, keys = vc.plant(rng, 2000, [50 * k + 25 for k in range(n_sites)], ins)
    return 2000, reads, list(base), list(qpos), sites, keys


def test_the_planted_segment_between_segments_of_no_one_and_thirty_two_sites(ctx):
    rng = np.random.default_rng(43)
    reads, base, qpos, sites, keys = vc.planted_segment()
    planted = (400, reads, list(base), list(qpos), sites, keys)
    qr, qb, qq, qs, qk = vc.quiet_segment()
    none = (300, qr, list(qb), list(qq), qs[:0], np.zeros(len(qr), np.uint64))   # reads and no site: key2 is the key, one isoform
    one = _site_of_windows([_mutate(rng, _rand(rng, 40), 0.05) for _ in range(5)])
    many = _many_sites(rng)
    segments = [planted, none, one, many, planted, (300, qr, list(qb), list(qq), qs, qk)]
    got = _run(ctx, segments, min_depth=3, **vc.PLANT)
    assert len(got["win"]) == 5 + 0 + 1 + 32 + 5 + 2 and [int(x) for x in got["seg"]["n_split"]] == [2, 0, 0, 16, 2, 0]
    # the block stage's words as the major ones: the planted segment under three of them, one without a complete mask
    pre = []
    for s in segments:
        n = len(s[1])
        pk = np.array([(1, 2**63 + 1, 0)[i % 3] for i in range(n)], np.uint64)
        pm = np.full(n, 2**64 - 1, np.uint64)
        pm[n // 2] = 3
        pre.append((pk, pm, 2**64 - 1))
    _run(ctx, segments, min_depth=3, pre=pre, **vc.PLANT)


def test_a_round_b_across_the_launch_limit(ctx):
    """The direction words of round B cross the per-launch limit of k_win_align once, with real alignments of 512 x 512 — 16384 words
    each, 2048 of them a launch — and not with many small ones: 2060 carriers of a 20-base exon, whose median is template A and keeps
    round A cheap, and 2052 of a 512-base window, all far, that make up round B."""
    rng = np.random.default_rng(47)
    short, long = _rand(rng, 20), _rand(rng, 512)
    swap = lambda s, at: s[:at] + bytes([b"ACGT"[(b"ACGT".index(s[at]) + 1) % 4]]) + s[at + 1:]   # one substitution: the same exon read again
    windows = [swap(short, i % 20) if i % 2 == 0 or i >= 4104 else swap(swap(long, i % 512), (7 * i) % 512) for i in range(4112)]
    got = _run(ctx, [_site_of_windows(windows)], min_depth=3, max_win=512, slack=0)
    assert [int(got["var"][0][f]) for f in ("split", "n_a", "n_b", "n_other", "n_far", "tlen_b")] == [1, 2060, 2052, 0, 2052, 512]


def test_the_property_case_on_the_device(ctx):
    frame, exons, reads, planted, (base, qpos, ins), want = vc.host_property()
    got = _run(ctx, [(len(frame), reads, list(base), list(qpos), ins["sites"], ins["reads"]["key"])], min_depth=3)
    host_like = dict(win=got["win"], var=got["var"], variant=got["variant"], seq=got["seq"])
    assert all(vc.property_holds(host_like, planted, frame, exons))
    dist = vc.distances(frame, exons, host_like, planted)
    print("variants", got["var"], "(to its own true window, to the other's, length)", dist)
    assert dist == vc.PINNED   # the device's bytes are the host path's
    assert int(got["seg"][0]["n_groups"]) == 4 and int(got["seg"][0]["n_split"]) == 1
    # the window call returns what it returned: its records, and its bytes at the site that does not split
    ctx.align_set_pool(reads)
    old = ctx.planes_insert_windows([len(frame)], [0] * len(reads), list(range(len(reads))), list(base), list(qpos), [ins["sites"]], ins["reads"]["key"])
    assert old["win"].tobytes() == got["win"].tobytes() and old["seq"][1] == got["seq"][2] and old["seq"][0] == wc.host_windows(
        reads, base, qpos, ins["sites"], ins["reads"]["key"])["seq"][0]


def test_refusals_against_canaries_and_the_empty_call(ctx):
    rlen, reads, base, qpos, sites, keys = _site_of_windows([b"ACGTACGT"] * 3)
    ctx.align_set_pool(reads)
    L, S, n = ctx.L, 1, 3
    fb, fq = np.concatenate(base), np.concatenate(qpos)
    rl, sop, qy, soff = np.array([rlen], np.int32), np.zeros(3, np.int32), np.arange(3, dtype=np.int32), np.array([0, 1], np.int64)
    bound = 2 * (7 * 64 + 6)
    pre = np.zeros(3, np.uint64)

    def call(**kw):
        a = dict(rl=rl, sop=sop, qy=qy, sites=sites, soff=soff, slack=0, max_win=64, match=2, mismatch=-2, gap=2, depth=1, min_agree=45, min_alt=3, min_pct=25, cap=bound,
                 pk=None, pm=None, pf=None)
        a.update(kw)
        outs = [np.full(m, 0xA5, np.uint8) for m in (S * 32, S * 32, bound, bound, (2 * S + 1) * 8, 2 * S * 32, n * 32, n * 32 * 8, n * 16, 32)]
        p = lambda x, t: x.ctypes.data_as(C.POINTER(t)) if x is not None else None
        d = lambda x: x.ctypes.data if x is not None else None
        rc = L.ioc_planes_insert_window_variants(ctx.h, 1, p(a["rl"], C.c_int32), 3, p(a["sop"], C.c_int32), p(a["qy"], C.c_int32), fb.ctypes.data, fq.ctypes.data,
                                                 a["sites"].ctypes.data, p(a["soff"], C.c_int64), keys.ctypes.data, a["slack"], a["max_win"], a["match"], a["mismatch"],
                                                 a["gap"], a["depth"], a["min_agree"], a["min_alt"], a["min_pct"], d(a["pk"]), d(a["pm"]), d(a["pf"]),
                                                 *(o.ctypes.data for o in outs[:4]), a["cap"], p(outs[4], C.c_int64), *(o.ctypes.data for o in outs[5:]))
        return rc, all((o == 0xA5).all() for o in outs)

    assert call() == (0, False)
    assert call(pk=pre, pm=pre, pf=pre[:1]) == (0, False)
    outside = sites.copy()
    outside[0]["end"] = rlen + 1
    for bad in (dict(min_agree=0), dict(min_agree=101), dict(min_alt=0), dict(min_pct=0), dict(min_pct=51), dict(slack=-1), dict(slack=33), dict(max_win=0),
                dict(max_win=513), dict(gap=-1), dict(match=(1 << 20) + 1), dict(depth=0), dict(sites=outside), dict(soff=np.array([1, 1], np.int64)),
                dict(soff=np.array([0, 33], np.int64)), dict(qy=np.array([0, 1, 3], np.int32)), dict(sop=np.array([0, 1, 0], np.int32)), dict(cap=-1),
                dict(pk=pre), dict(pk=pre, pm=pre), dict(pf=pre[:1])):
        assert call(**bad) == (-1, True), bad
    assert call(cap=bound - 1) == (-4, True)
    empty = ctx.planes_insert_window_variants([], [], [], [], [], [], [])
    assert len(empty["win"]) == 0 and empty["off"].tolist() == [0] and len(empty["reads"]) == 0
    # pairs and no site anywhere: every read keeps its key, one isoform a segment
    qr, qb, qq, qs, _ = vc.quiet_segment()
    got = _run(ctx, [(300, qr, list(qb), list(qq), qs[:0], np.zeros(len(qr), np.uint64))], min_depth=3)
    assert len(got["win"]) == 0 and int(got["seg"][0]["n_groups"]) == 1


def test_the_fused_call_against_the_host_path_on_the_property_case(ctx):
    """ioc_align_pairs_blocks_inserts_variants on the property case beside a segment where nothing splits (the reads of
    blocks_common.property_case on representative A): everything ioc_align_pairs_blocks_inserts_seq returns is what that call returns
    alone, and the variants are the host definition's over the host pipeline's planes, the block stage's words as pre_*."""
    from tests import blocks_common as bc
    from tests import inserts_common as ic
    frame, exons, reads, planted = vc.property_reads(vc.SEED)
    T, reads2, _ = bc.property_case(wc.SEED)
    frames, groups = [frame, ic.representative(T, "A")], [reads, reads2]
    seqs, pairs = list(frames), []
    for g, rds in enumerate(groups):
        for rd in rds:
            pairs.append((len(seqs), g, 0, 0.1))
            seqs.append(rd)
    order = sorted(range(len(pairs)), key=lambda x: (sum(1 for y in range(x) if pairs[y][1] == pairs[x][1]), pairs[x][1]))
    pairs = [pairs[x] for x in order]
    sop = [p[1] for p in pairs]
    segs = [(g, 0) for g in range(2)]
    ctx.align_set_pool(seqs)
    plain = ctx.align_pairs_blocks_inserts_seq(pairs, 11, segs, sop, tables=True, stats=True)
    got = ctx.align_pairs_blocks_inserts_variants(pairs, 11, segs, sop, tables=True, stats=True)
    for f in ("score", "windows", "ratio", "block_off", "reads", "seg", "stats", "cols", "row0"):
        assert got[f].tobytes() == plain[f].tobytes(), f
    for f in ("blocks", "rows"):
        assert [x.tobytes() for x in got[f]] == [x.tobytes() for x in plain[f]], f
    for f in ("site_off", "reads", "seg"):
        assert got["inserts"][f].tobytes() == plain["inserts"][f].tobytes(), f
    for f in ("sites", "rows"):
        assert [x.tobytes() for x in got["inserts"][f]] == [x.tobytes() for x in plain["inserts"][f]], f
    for f in ("win", "off", "polish"):
        assert got["insert_windows"][f].tobytes() == plain["insert_windows"][f].tobytes(), f
    assert got["insert_windows"]["seq"] == plain["insert_windows"]["seq"] and got["insert_windows"]["qual"] == plain["insert_windows"]["qual"]
    v, x = got["insert_variants"], 0
    for g, (f, rds) in enumerate(zip(frames, groups)):
        mine = [i for i, s in enumerate(sop) if s == g]
        base, ilen, qpos = [], [], []
        for rd in rds:
            ops, _ = api.host_align_ops(rd, f, gap_open=ic.pc.gap_open(0.1))
            base.append(api.ops_project(ops, rd, len(f))[0]), ilen.append(api.ops_project_ilen(ops, len(f))), qpos.append(api.ops_project_qpos(ops, len(f)))
        ins = api.planes_inserts(np.array(base), np.array(ilen))
        assert ins["sites"][["first", "end"]].tobytes() == got["inserts"]["sites"][g][["first", "end"]].tobytes()
        want = api.insert_window_variants(np.array(base), np.array(qpos), [len(rd) for rd in rds], ins["sites"], ins["reads"]["key"], rds)
        S = len(ins["sites"])
        for k in range(S):
            for fld in ("split", "tlen_b", "n_a", "n_b", "n_other", "n_far"):
                assert int(v["var"][x][fld]) == int(want["var"][k][fld]), (g, k, fld)
            tb = int(want["var"][k]["template_pair_b"])
            assert int(v["var"][x]["template_pair_b"]) == (mine[tb] if tb >= 0 else -1)
            for h in range(2):
                assert (v["seq"][2 * x + h], v["qual"][2 * x + h]) == (want["seq"][2 * k + h], want["qual"][2 * k + h]), (g, k, h)
            x += 1
        assert v["variant"][mine][:, :S].tobytes() == want["variant"].tobytes() and v["agree"][mine][:, :S].tobytes() == want["agree"].tobytes(), g
        assert v["reads"]["key2"][mine].tobytes() == want["key2"].tobytes(), g
        blocks = got["reads"][mine]   # the block stage's records of the segment's pairs: its key, and the mask of the states it has
        nb = int(got["seg"][g]["n_blocks"])
        pm = np.array([sum(3 << (2 * b) for b in range(nb) if (int(key) >> (2 * b)) & 3 != api.BLOCK_NONE) for key in blocks["key"]], np.uint64)
        grp, how, c = api.key_isoforms(want["key2"], want["mask2"], (1 << (2 * S)) - 1, api.BLOCKS_RULE["min_alt"], pre_key=blocks["key"], pre_mask=pm,
                                       pre_full=(1 << (2 * nb)) - 1)
        assert v["reads"]["group"][mine].tolist() == grp.tolist() and v["reads"]["how"][mine].tolist() == how.tolist(), g
        assert int(v["seg"][g]["n_groups"]) == c["n_groups"] and int(v["seg"][g]["n_split"]) == (1, 0)[g]
    assert x == len(v["var"]) == 4
    own = [i for i, s in enumerate(sop) if s == 0]
    host_like = dict(win=v["win"][:2].copy(), var=v["var"][:2], variant=v["variant"][own], seq=v["seq"][:4])
    host_like["win"]["template_pair"] = [own.index(int(t)) for t in host_like["win"]["template_pair"]]
    assert all(vc.property_holds(host_like, planted, frame, exons)) and vc.distances(frame, exons, host_like, planted) == vc.PINNED
    empty = ctx.align_pairs_blocks_inserts_variants([], 11, [], [])
    assert len(empty["insert_variants"]["var"]) == 0 and empty["insert_variants"]["off"].tolist() == [0]
    with pytest.raises(api.IocError) as e:
        ctx.align_pairs_blocks_inserts_variants(pairs, 11, segs, sop, min_agree=0)
    assert e.value.code == -1
    with pytest.raises(api.IocError) as e:
        ctx.align_pairs_blocks_inserts_variants(pairs, 11, segs, sop, var_cap=api.insert_window_variants_bound(64) - 1)
    assert e.value.code == -4


def test_the_fused_call_where_no_site_is_kept(ctx):
    """reads that are their representative at 5 % errors: no block, no site — key2 is the key, the isoforms counted again are the insert
    stage's, every variant byte is 0 and no slot is called; everything else is what ioc_align_pairs_blocks_inserts_seq returns"""
    rng = np.random.default_rng(61)
    frames = [_rand(rng, 400), _rand(rng, 300)]
    seqs, pairs = list(frames), []
    for i in range(14):
        pairs.append((len(seqs), i % 2, 0, 0.1))
        seqs.append(_mutate(rng, frames[i % 2], 0.05))
    sop, segs = [p[1] for p in pairs], [(0, 0), (1, 0)]
    ctx.align_set_pool(seqs)
    plain = ctx.align_pairs_blocks_inserts_seq(pairs, 11, segs, sop)
    got = ctx.align_pairs_blocks_inserts_variants(pairs, 11, segs, sop)
    assert int(got["inserts"]["site_off"][-1]) == 0 and got["inserts"]["reads"].tobytes() == plain["inserts"]["reads"].tobytes()
    assert got["reads"].tobytes() == plain["reads"].tobytes() and got["score"].tobytes() == plain["score"].tobytes()
    v, ins = got["insert_variants"], got["inserts"]
    assert len(v["var"]) == 0 and v["off"].tolist() == [0] and not v["variant"].any() and (v["agree"] == vc.NO).all()
    for f, g in (("key2", "key"), ("group", "group"), ("how", "how")):
        assert v["reads"][f].tolist() == ins["reads"][g].tolist(), f
    for f in ("n_groups", "n_reads", "n_direct", "n_assigned", "n_rare", "n_ambiguous"):
        assert v["seg"][f].tolist() == ins["seg"][f].tolist(), f
    assert v["seg"]["n_sites"].tolist() == [0, 0] and v["seg"]["n_split"].tolist() == [0, 0] and v["seg"]["n_groups"].tolist() == [1, 1]
