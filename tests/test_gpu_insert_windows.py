"""The kernels of ioc_insert_windows.hip against the host definitions, as bytes: k_win_bounds, k_win_template and k_win_align
through ioc_planes_insert_windows (windows of every length at which the fill takes another path, the chosen strings of the host
test, a few hundred random pairs, interleaved segments, 32 kept sites, the refusals against canaries); the position plane and the
fused call through ioc_align_pairs_blocks_inserts_seq against ioc_align_pairs_blocks_inserts and the host pipeline; the property."""
import ctypes as C

import numpy as np
import pytest

from isonclust2_amd import api
from tests import blocks_common as bc
from tests import inserts_common as ic
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
    """A segment of 8 rows with ONE site, the junction in front of row 4, whose carriers hold exactly `windows` between the anchors at
    slack 0 (lo = 4, hi = 5): read i is CCCC, its window, GGG, and its planes say that the window's last base stands on row 4 and
    the rest is an insertion in front of it.  Returns (rlen, reads, base, qpos, sites, keys)."""
    rlen = 8
    reads, base, qpos = [], [], []
    for w in windows:
        rd = b"CCCC" + w + b"GGG"
        ops = b"====" + b"I" * (len(w) - 1) + b"=" + b"==="
        reads.append(rd), base.append(api.ops_project(ops, rd, rlen)[0]), qpos.append(api.ops_project_qpos(ops, rlen))
    sites = np.zeros(1, api.PILE_INSERT_DTYPE)
    sites[0]["first"], sites[0]["end"] = 4, 5
    return rlen, reads, base, qpos, sites, np.full(len(windows), CARRY, np.uint64)


def _run_sites(ctx, segments, min_depth=1, tables=True, **rule):
    """segments: a list of _site_of_windows results; their pairs interleaved in one call, against the host path segment by segment"""
    seqs, sop, query, base, qpos, keys, mine = [], [], [], [], [], [], [[] for _ in segments]
    left = [list(range(len(s[1]))) for s in segments]
    while any(left):
        for g, s in enumerate(segments):
            if left[g]:
                i = left[g].pop(0)
                mine[g].append(len(sop))
                sop.append(g), query.append(len(seqs)), seqs.append(s[1][i]), base.append(s[2][i]), qpos.append(s[3][i]), keys.append(int(s[5][i]))
    ctx.align_set_pool(seqs + [b"ACGT"])
    got = ctx.planes_insert_windows([s[0] for s in segments], sop, query, base, qpos, [s[4] for s in segments], keys, min_depth=min_depth, tables=tables, **rule)
    x = 0
    for g, s in enumerate(segments):
        want = wc.host_windows(s[1], np.array(s[2]).reshape(len(s[1]), s[0] + 1), np.array(s[3]).reshape(len(s[1]), s[0] + 1), s[4], s[5], min_depth=min_depth, **rule)
        for k in range(len(s[4])):
            wc.same_site(got, x, want, k)
            t = int(want["win"][k]["template_pair"])
            assert int(got["win"][x]["template_pair"]) == (mine[g][t] if t >= 0 else -1), (g, k)
            x += 1
    assert x == len(got["win"]) and int(got["off"][-1]) == sum(len(s) for s in got["seq"])
    return got


LENGTHS = (1, 15, 16, 17, 63, 64, 65, 128, 129, 512)


def test_windows_of_every_length_against_the_host(ctx):
    """every template length x every voter length of LENGTHS in one call: a segment per combination with three carriers, the template
    twice and the voter — the template's length is the middle of the three, and of two equal windows the index decides"""
    rng = np.random.default_rng(23)
    segments, want_t = [], []
    for t in LENGTHS:
        core = _rand(rng, t)
        for n in LENGTHS:
            other = _mutate(rng, (core * (n // t + 1))[:n], 0.08)[:n].ljust(n, b"G")
            segments.append(_site_of_windows([core, core, other] if n >= t else [other, core, core]))
            want_t.append(t)
    got = _run_sites(ctx, segments, max_win=512, slack=0)
    assert [int(w["tlen"]) for w in got["win"]] == want_t and all(int(w["n_voters"]) == 3 for w in got["win"])


def test_chosen_strings_and_scoring_sets_against_the_host(ctx):
    rng = np.random.default_rng(5)
    long = _rand(rng, 200)
    pairs = [(b"G", long), (long, b"G"), (long, long), (b"AAAA", b"AAA"), (b"AAA", b"AAAA"), (b"ACGT", b"TGCA"), (b"A", b"C")]
    for match, mismatch, gap in ((2, -2, 2), (1, -1, 1), (5, -4, 2), (-7, -8, 1), (2, -9, 1)):
        # the template is the middle of (voter, template, template) or (template, template, voter) by length
        segments = [_site_of_windows([t, t, q] if len(q) >= len(t) else [q, t, t]) for q, t in pairs]
        got = _run_sites(ctx, segments, max_win=512, slack=0, match=match, mismatch=mismatch, gap=gap)
        assert [int(w["tlen"]) for w in got["win"]] == [len(t) for _, t in pairs]


def test_random_pairs_against_the_host(ctx):
    """a few hundred alignments in one call: 12 sites of 25 carriers each, 8 % errors, at depths where the call calls"""
    rng = np.random.default_rng(31)
    segments = []
    for _ in range(12):
        core = _rand(rng, int(rng.integers(20, 300)))
        segments.append(_site_of_windows([_mutate(rng, core, 0.08) for _ in range(25)]))
    got = _run_sites(ctx, segments, min_depth=3, max_win=512, slack=0)
    assert all(int(w["n_voters"]) == 25 for w in got["win"])


def test_planted_classes_interleaved_segments_and_thirty_two_sites(ctx):
    reads, base, qpos, sites, keys, _ = wc.planted_segment(max_win=40)
    seg = (200, reads, list(base), list(qpos), sites, keys)
    # 35 sites found, 32 kept: a segment of 2000 rows, sites every 50 rows, eight carriers of a 20-base insertion at each
    rng = np.random.default_rng(41)
    rlen, n_sites = 2000, 32
    many = np.zeros(n_sites, api.PILE_INSERT_DTYPE)
    many["first"], many["end"] = 50 * np.arange(n_sites) + 25, 50 * np.arange(n_sites) + 26
    body = _rand(rng, rlen)
    rds, bs, qs = [], [], []
    for i in range(8):
        ops, rd = b"", b""
        for k in range(35):
            ins = _rand(rng, 20) if k < 32 or i < 4 else b""
            ops += b"=" * 25 + b"I" * len(ins) + b"=" * 25
            rd += body[50 * k:50 * k + 25] + ins + body[50 * k + 25:50 * k + 50]
        ops, rd = ops + b"=" * (rlen - 1750), rd + body[1750:]
        rds.append(rd), bs.append(api.ops_project(ops, rd, rlen)[0]), qs.append(api.ops_project_qpos(ops, rlen))
    full = np.full(8, sum(CARRY << (2 * k) for k in range(32)), np.uint64)
    got = _run_sites(ctx, [seg, (rlen, rds, bs, qs, many, full), seg], min_depth=3, max_win=40, slack=8)
    assert len(got["win"]) == 3 + 32 + 3 and int(got["win"][1]["n_short"]) == 1 and int(got["win"][1]["n_long"]) == 1
    assert got["seq"][2] == b"" and int(got["win"][2]["template_pair"]) == -1   # a site with no voter is not called
    assert all(int(w["n_voters"]) == 8 and int(w["tlen"]) == 37 for w in got["win"][3:35])


def test_refusals_against_canaries(ctx):
    rlen, reads, base, qpos, sites, keys = _site_of_windows([b"ACGTACGT"] * 3)
    ctx.align_set_pool(reads)
    L, S = ctx.L, 1
    fb, fq = np.concatenate(base), np.concatenate(qpos)
    rl, sop, qy, soff = np.array([rlen], np.int32), np.zeros(3, np.int32), np.arange(3, dtype=np.int32), np.array([0, 1], np.int64)

    def call(**kw):
        a = dict(rl=rl, sop=sop, qy=qy, fb=fb, fq=fq, sites=sites, soff=soff, keys=keys, slack=0, max_win=64, match=2, mismatch=-2, gap=2, depth=1, cap=7 * 64 + 6)
        a.update(kw)
        win, off = np.full(S * 32, 0xA5, np.uint8), np.full((S + 1) * 8, 0xA5, np.uint8)
        seq, qual, pol = np.full(7 * 64 + 6, 0xA5, np.uint8), np.full(7 * 64 + 6, 0xA5, np.uint8), np.full(S * 32, 0xA5, np.uint8)
        p = lambda x, t: x.ctypes.data_as(C.POINTER(t)) if x is not None else None
        rc = L.ioc_planes_insert_windows(ctx.h, 1, p(a["rl"], C.c_int32), 3, p(a["sop"], C.c_int32), p(a["qy"], C.c_int32), a["fb"].ctypes.data, a["fq"].ctypes.data,
                                         a["sites"].ctypes.data, p(a["soff"], C.c_int64), a["keys"].ctypes.data, a["slack"], a["max_win"], a["match"], a["mismatch"],
                                         a["gap"], a["depth"], win.ctypes.data, seq.ctypes.data, qual.ctypes.data, a["cap"], p(off, C.c_int64), pol.ctypes.data, None, None)
        return rc, all((x == 0xA5).all() for x in (win, off, seq, qual, pol))

    assert call() == (0, False)
    outside = sites.copy()
    outside[0]["end"] = rlen + 1
    for bad in (dict(slack=-1), dict(slack=33), dict(max_win=0), dict(max_win=513), dict(gap=-1), dict(match=(1 << 20) + 1), dict(depth=0), dict(sites=outside),
                dict(soff=np.array([1, 1], np.int64)), dict(soff=np.array([0, -1], np.int64)), dict(soff=np.array([0, 33], np.int64)),
                dict(qy=np.array([0, 1, 3], np.int32)), dict(qy=np.array([0, -1, 2], np.int32)), dict(sop=np.array([0, 1, 0], np.int32)), dict(cap=-1)):
        assert call(**bad) == (-1, True), bad
    assert call(cap=7 * 64 + 5) == (-4, True)


def _fused(ctx, frames, groups, irule={}, **kw):
    seqs, pairs = list(frames), []
    for g, reads in enumerate(groups):
        for rd in reads:
            pairs.append((len(seqs), g, 0, 0.1))
            seqs.append(rd)
    order = sorted(range(len(pairs)), key=lambda x: (sum(1 for y in range(x) if pairs[y][1] == pairs[x][1]), pairs[x][1]))
    pairs = [pairs[x] for x in order]
    sop = [p[1] for p in pairs]
    segs = [(g, 0) for g in range(len(frames))]
    ctx.align_set_pool(seqs)
    plain = ctx.align_pairs_blocks_inserts(pairs, 11, segs, sop, tables=True, stats=True, **irule)
    got = ctx.align_pairs_blocks_inserts_seq(pairs, 11, segs, sop, tables=True, stats=True, **irule, **kw)
    for f in ("score", "windows", "ratio", "block_off", "reads", "seg", "stats", "cols", "row0"):
        assert got[f].tobytes() == plain[f].tobytes(), f
    for f in ("blocks", "rows"):
        assert [x.tobytes() for x in got[f]] == [x.tobytes() for x in plain[f]], f
    for f in ("site_off", "reads", "seg"):
        assert got["inserts"][f].tobytes() == plain["inserts"][f].tobytes(), f
    for f in ("sites", "rows"):
        assert [x.tobytes() for x in got["inserts"][f]] == [x.tobytes() for x in plain["inserts"][f]], f
    mine = [[x for x, s in enumerate(sop) if s == g] for g in range(len(frames))]
    return seqs, pairs, mine, got


def _host_segment(frame, reads):
    """the host pipeline of one segment: the host aligner, the three host projections, the site search, the windows"""
    base, ilen, qpos = [], [], []
    for rd in reads:
        ops, _ = api.host_align_ops(rd, frame, gap_open=ic.pc.gap_open(0.1))
        base.append(api.ops_project(ops, rd, len(frame))[0]), ilen.append(api.ops_project_ilen(ops, len(frame))), qpos.append(api.ops_project_qpos(ops, len(frame)))
    return base, ilen, qpos


def test_the_fused_call_and_the_property_on_the_device(ctx):
    T, reads, _ = bc.property_case(wc.SEED)
    frame = ic.representative(T, "A")
    Tb, reads_b, _ = bc.property_case(ic.SEED_B)
    seqs, pairs, mine, got = _fused(ctx, [frame, ic.representative(Tb, "B")], [reads, reads_b])
    w, x = got["insert_windows"], 0
    for g, (f, rds) in enumerate(((frame, reads), (ic.representative(Tb, "B"), reads_b))):
        base, ilen, qpos = _host_segment(f, rds)
        ins = api.planes_inserts(np.array(base), np.array(ilen))   # (the sites and the states do not depend on the block words)
        assert ins["sites"][["first", "end"]].tobytes() == got["inserts"]["sites"][g][["first", "end"]].tobytes()
        want = wc.host_windows(rds, np.array(base), np.array(qpos), ins["sites"], ins["reads"]["key"])
        for k in range(len(ins["sites"])):
            wc.same_site(w, x, want, k)
            assert int(w["win"][x]["template_pair"]) == mine[g][int(want["win"][k]["template_pair"])]
            x += 1
    assert x == len(w["win"]) == 3
    dist = wc.distances(T, frame, w["win"][:2], w["seq"][:2])
    print("windows", w["win"], "(to the true window, to the representative's rows, length)", dist)
    for k in range(2):
        assert dist[k][1] - dist[k][0] >= wc.MARGIN[k], (k, dist[k])
    assert dist == wc.PINNED   # the device's bytes are the host path's


def test_the_position_plane_across_the_256_byte_step(ctx):
    """pairs whose operation bytes cross the 256-byte step of the walk with a run of 'I' open: a 900-base frame, reads that hold
    an insertion of 10 .. 70 bases at 230 .. 260.  The position plane is not returned: a read's window IS its position plane at the
    anchors, so the windows of the fused call are held against those of the host projections."""
    rng = np.random.default_rng(53)
    frame = _rand(rng, 900)
    reads = [frame] * 6
    for at in (225, 232, 240, 247, 250, 253, 255, 256, 258):
        for n in (10, 40, 70):
            reads.append(frame[:at] + _rand(rng, n) + frame[at:])
    seqs, pairs, mine, got = _fused(ctx, [frame], [reads], irule=dict(min_ins=10))
    base, ilen, qpos = _host_segment(frame, reads)
    crossing = 0
    for rd in reads:
        ops, _ = api.host_align_ops(rd, frame, gap_open=ic.pc.gap_open(0.1))
        crossing += any(ops[a] == 73 and ops[a - 1] == 73 for a in range(256, len(ops), 256))
    assert crossing >= 5   # the case is what it says it is
    ins = api.planes_inserts(np.array(base), np.array(ilen), min_ins=10)
    assert len(ins["sites"]) >= 1 and ins["sites"][["first", "end"]].tobytes() == got["inserts"]["sites"][0][["first", "end"]].tobytes()
    want = wc.host_windows(reads, np.array(base), np.array(qpos), ins["sites"], ins["reads"]["key"])
    for k in range(len(ins["sites"])):
        wc.same_site(got["insert_windows"], k, want, k)
        assert int(got["insert_windows"]["win"][k]["n_voters"]) >= 5


def test_the_fused_call_refuses_and_the_empty_call(ctx):
    ctx.align_set_pool([b"ACGTACGTAC", b"ACGTTCGTAC"])
    empty = ctx.align_pairs_blocks_inserts_seq([], 11, [], [])
    assert len(empty["insert_windows"]["win"]) == 0 and empty["insert_windows"]["off"].tolist() == [0]
    pairs = [(1, 0, 0, 0.1)]
    for bad in (dict(max_win=0), dict(max_win=513), dict(win_gap=-1), dict(polish_min_depth=0), dict(slack=33)):
        with pytest.raises(api.IocError) as e:
            ctx.align_pairs_blocks_inserts_seq(pairs, 11, [(0, 0)], [0], **bad)
        assert e.value.code == -1, bad
    with pytest.raises(api.IocError) as e:
        ctx.align_pairs_blocks_inserts_seq(pairs, 11, [(0, 0)], [0], win_cap=api.insert_windows_bound(9) - 1)   # 9 junctions: min(32, rlen - 1) sites
    assert e.value.code == -4
    got = ctx.align_pairs_blocks_inserts_seq(pairs, 11, [(0, 0)], [0], min_depth=1, min_alt=1)
    assert len(got["insert_windows"]["win"]) == 0 and int(got["inserts"]["seg"][0]["n_groups"]) == 1
