"""ioc_align_pairs_blocks_ends: ioc_align_pairs_blocks with the ends kernels behind the block kernels.  Everything
align_pairs_blocks returns must equal that call's own result, byte for byte; the extents must equal ioc_host_ops_extent of what
align_pairs_ops returns pair for pair, pairs without an alignment included; the ends must equal the host definition on those extents
and the block stage's groups, as bytes — with and without the statistics, in slices and under a re-run of every pair.  Property
case A must hold on the device, and every variant's consensus from ioc_planes_polish_groups must be the representative."""
import random

import numpy as np
import pytest

from isonclust2_amd import api
from tests import blocks_common as bc
from tests import ends_common as ec
from tests import iso_polish_common as ipc
from tests import polish_common as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _pool(frames, groups):
    """frames[g] with the reads groups[g], their pairs interleaved: (sequences, pairs, segments, seg_of_pair, the pairs of each segment)"""
    seqs, pairs = list(frames), []
    for g, reads in enumerate(groups):
        for rd in reads:
            pairs.append((len(seqs), g, 0, 0.1))
            seqs.append(rd)
    order = sorted(range(len(pairs)), key=lambda x: (sum(1 for y in range(x) if pairs[y][1] == pairs[x][1]), pairs[x][1]))
    pairs = [pairs[x] for x in order]
    sop = [p[1] for p in pairs]
    return seqs, pairs, [(g, 0) for g in range(len(frames))], sop, [[x for x, s in enumerate(sop) if s == g] for g in range(len(frames))]


def _same_as_plain(got, plain, stats):
    for f in ("score", "windows", "ratio", "block_off", "reads", "seg", "cols", "row0") + (("stats",) if stats else ()):
        assert got[f].tobytes() == plain[f].tobytes(), f
    for f in ("blocks", "rows"):
        assert [x.tobytes() for x in got[f]] == [x.tobytes() for x in plain[f]], f


def _check(ctx, frames, groups, rule={}, erule={}, stats=True):
    """the fused call against align_pairs_blocks, align_pairs_ops and the host definition; returns (result, pairs of each segment, strings)"""
    seqs, pairs, segs, sop, mine = _pool(frames, groups)
    ctx.align_set_pool(seqs)
    plain = ctx.align_pairs_blocks(pairs, 11, segs, sop, tables=True, stats=stats, **rule)
    got = ctx.align_pairs_blocks_ends(pairs, 11, segs, sop, tables=True, stats=stats, **rule, **erule)
    assert ("stats" in got) == stats
    _same_as_plain(got, plain, stats)
    ops = ctx.align_pairs_ops(pairs, 11)[3]
    want = np.array([tuple(api.host_ops_extent(o, len(frames[sop[i]]))) if len(o) else (0, 0, 0, 0) for i, o in enumerate(ops)], ec.E)
    assert got["extents"].tobytes() == want.tobytes()
    full = {**bc.DEFAULT, **rule}
    er = {k[5:] if k == "ends_min_pct" else k: v for k, v in erule.items()}
    host = [api.host_reads_ends(want[mine[g]], len(f), pre_group=got["reads"]["group"][mine[g]], **{**ec.DEFAULT, "min_depth": full["min_depth"], "min_alt": full["min_alt"], **er})
            for g, f in enumerate(frames)]
    ec.same_as_host(got["ends"], host, mine)
    lean = ctx.align_pairs_blocks_ends(pairs, 11, segs, sop, rows=False, stats=not stats, **rule, **erule)
    assert "cols" not in lean and "rows" not in lean and "rows" not in lean["ends"]
    assert lean["extents"].tobytes() == got["extents"].tobytes() and lean["reads"].tobytes() == got["reads"].tobytes()
    ec.same_as_host(lean["ends"], host, mine)
    return got, mine, ops, (seqs, pairs, segs, sop)


def _short_case():
    """three short segments, 65 to 200 rows and 3 to 70 reads: whole reads, reads that stop early or start late, reads that go on
    beyond either end of the representative, and an empty query"""
    rng = random.Random(5)
    T = bytes(rng.choice(b"ACGT") for _ in range(260))
    cut = lambda a, z, n: [pc.mutate(rng, T[a:z], 0.06) for _ in range(n)]
    return [T[30:230], T[:65], T[100:229]], [cut(30, 230, 30) + cut(0, 260, 20) + cut(30, 150, 12) + cut(110, 230, 8), cut(0, 65, 2) + [b""], cut(100, 229, 6) + cut(60, 260, 6) + [b""] + cut(130, 229, 5)]


@pytest.mark.parametrize("stats", [True, False], ids=["stats", "no_stats"])
def test_three_short_segments(ctx, stats):
    frames, groups = _short_case()
    assert [len(f) for f in frames] == [200, 65, 129] and [len(g) for g in groups] == [70, 3, 18]
    got, mine, ops, _ = _check(ctx, frames, groups, stats=stats)
    nothing = np.flatnonzero(got["extents"]["end_row"] == 0)   # the two empty queries: no alignment, an extent of zeros, no site
    assert len(nothing) == 2 and not got["extents"][nothing].tobytes().strip(b"\0") and set(got["ends"]["reads"][nothing]["start_site"].tolist()) == {-1}
    assert int(got["ends"]["seg"][0]["n_variants"]) >= 2
    over = got["ends"]["starts"][0][0]
    assert int(over["first"]) == 0 and int(over["n_over"]) >= 15   # the 20 reads of T[0:260] carry 30 bases in front of row 0
    _check(ctx, frames, groups, rule=dict(min_depth=2, min_alt=2), erule=dict(slack=3, min_over=5, ends_min_pct=100, max_sites=2, max_variants=1), stats=stats)


@pytest.mark.parametrize("stats", [True, False], ids=["stats", "no_stats"])
def test_property_case_a_on_the_device(ctx, stats):
    frame, reads, _, _ = ec.property_case("A")
    got, mine, ops, _ = _check(ctx, [frame], [reads], stats=stats)
    ends = got["ends"]
    holding = lambda sites, row: [b for b, s in enumerate(sites) if int(s["first"]) <= row < int(s["end"])]
    assert len(ends["starts"][0]) == 2 and [holding(ends["starts"][0], r) for r in ec.STARTS_A] == [[0], [1]]
    assert len(ends["stops"][0]) == 2 and [holding(ends["stops"][0], r) for r in ec.STOPS_A] == [[0], [1]]
    assert [tuple(v)[:3] for v in ends["variants"][0].tolist()] == [(0, 0, 0), (0, 0, 1), (0, 1, 1)]
    true = [(0, 1)] * ec.CLASS + [(0, 0)] * ec.CLASS + [(1, 1)] * ec.CLASS
    whole = [(int(r["start_site"]), int(r["stop_site"])) for r in ends["reads"][:3 * ec.CLASS]]   # (one segment: pair i is read i)
    assert sum(m != t and -1 not in m for m, t in zip(whole, true)) == 0
    if stats:
        return
    # every variant's consensus with the call that exists: the reads' variant as group of ioc_planes_polish_groups
    base = [api.ops_project(o, rd, len(frame))[0] for o, rd in zip(ops, reads)]
    slots = [api.ops_project_ins(o, rd, len(frame)) for o, rd in zip(ops, reads)]
    called = ctx.planes_polish_groups([frame], [0] * len(reads), ends["reads"]["variant"], [3], base, slots, min_depth=3)
    assert [ipc.edit_distance(s, frame) for s in called["gseq"][0]] == [0, 0, 0]


def test_slices_and_a_rerun_of_every_pair(ctx, monkeypatch):
    frame, reads, _, _ = ec.property_case("A")
    ref, mine, _, (seqs, pairs, segs, sop) = _check(ctx, [frame], [reads], stats=False)
    fields = lambda r: [r["extents"].tobytes(), r["reads"].tobytes(), r["ends"]["reads"].tobytes(), r["ends"]["seg"].tobytes(), r["ends"]["starts"][0].tobytes(),
                        r["ends"]["stops"][0].tobytes(), r["ends"]["variants"][0].tobytes(), r["ends"]["rows"][0].tobytes()]
    monkeypatch.setenv("IOC_ALIGN_CK_BUDGET_MB", "1")
    for stats in (False, True):
        got = ctx.align_pairs_blocks_ends(pairs, 11, segs, sop, stats=stats)
        assert ctx.timings()["align_slices"] > 1 and fields(got) == fields(ref), stats
    monkeypatch.delenv("IOC_ALIGN_CK_BUDGET_MB")
    monkeypatch.setenv("IOC_ALIGN_V2_FAKE_TIMEOUT", "1")
    t0 = ctx.timings()["n_align_refused"]
    got = ctx.align_pairs_blocks_ends(pairs, 11, segs, sop)
    assert ctx.timings()["n_align_refused"] - t0 == len(pairs) and fields(got) == fields(ref)


def test_refusals_and_the_empty_call(ctx):
    ctx.align_set_pool([b"ACGTACGTAC", b"ACGTTCGTAC"])
    empty = ctx.align_pairs_blocks_ends([], 11, [], [], tables=True)
    assert empty["blocks"] == [] and empty["ends"]["starts"] == [] and empty["ends"]["reads"].shape == (0,) and empty["extents"].shape == (0,)
    none = ctx.align_pairs_blocks_ends([], 11, [(0, 0)], [])
    assert none["ends"]["site_off"].tolist() == [0, 0, 0] and none["ends"]["var_off"].tolist() == [0, 0] and int(none["ends"]["seg"][0]["n_reads"]) == 0
    pairs = [(1, 0, 0, 0.1)]
    for bad in (dict(min_gap=0), dict(min_depth=0), dict(min_pct=51), dict(max_blocks=33), dict(slack=-1), dict(slack=33), dict(min_over=0), dict(ends_min_pct=0),
                dict(ends_min_pct=101), dict(max_sites=0), dict(max_sites=33), dict(max_variants=0)):
        with pytest.raises(api.IocError) as e:
            ctx.align_pairs_blocks_ends(pairs, 11, [(0, 0)], [0], **bad)
        assert e.value.code == -1, bad
    for short in (dict(cap=9), dict(sites_cap=21), dict(variants_cap=0)):
        with pytest.raises(api.IocError) as e:
            ctx.align_pairs_blocks_ends(pairs, 11, [(0, 0)], [0], **short)
        assert e.value.code == -4, short
    with pytest.raises(api.IocError):
        ctx.align_pairs_blocks_ends(pairs, 11, [(0, 0)], [1])    # names no segment
    with pytest.raises(api.IocError):
        ctx.align_pairs_blocks_ends(pairs, 11, [(2, 0)], [0])    # a segment outside the pool
    got = ctx.align_pairs_blocks_ends(pairs, 11, [(0, 0)], [0], min_depth=1, min_alt=1)   # (one read: a start site, a stop site, a variant)
    assert tuple(got["extents"][0]) == (0, 10, 0, 0) and tuple(got["ends"]["reads"][0]) == (0, 0, 0, 0)
    assert got["ends"]["variants"][0].tolist() == [(0, 0, 0, 1)] and got["ends"]["rows"][0]["w_stops"].tolist() == [1] * 11
