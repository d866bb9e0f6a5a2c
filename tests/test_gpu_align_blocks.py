"""ioc_align_pairs_blocks: ioc_align_pairs_alleles' alignment, table of counts and projection, and the block kernels over the base
planes where they lie.  Scores, windows and ratio must equal align_pairs' on the same pairs; blocks, records and the row table must
equal the host pipeline's, as bytes — the host aligner, ioc_host_ops_project and ioc_host_planes_blocks —; `depth` must be the depth
of the returned table of counts.  On the property case of test_planes_blocks_host.py and on correct_common.isoform_case."""
import numpy as np
import pytest

from isonclust2_amd import api
from tests import blocks_common as bc
from tests import correct_common as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _check(ctx, frames, groups, **rule):
    """frames[g] with the reads groups[g], their pairs interleaved: the fused call against align_pairs and the host pipeline"""
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
    plain = ctx.align_pairs(pairs, 11)
    got = ctx.align_pairs_blocks(pairs, 11, segs, sop, tables=True, stats=True, **rule)
    for f, w in zip(("score", "windows", "ratio"), plain):
        assert np.array_equal(got[f], w), f
    mine = [[x for x, s in enumerate(sop) if s == g] for g in range(len(frames))]
    want = []
    for g, frame in enumerate(frames):
        planes = bc.host_base_planes(frame, [seqs[pairs[x][0]] for x in mine[g]]) if mine[g] else np.zeros((0, len(frame) + 1), np.uint8)
        want.append(api.planes_blocks(planes, **{**bc.DEFAULT, **rule}))
    bc.same_as_host(got, want, mine)
    for g in range(len(frames)):
        cols = got["cols"][int(got["row0"][g]):int(got["row0"][g]) + len(frames[g]) + 1]
        depth = sum(cols[f].astype(np.int64) for f in ("a", "c", "g", "t", "other", "del"))
        assert np.array_equal(got["rows"][g]["depth"], depth)
    lean = ctx.align_pairs_blocks(pairs, 11, segs, sop, rows=False, **rule)
    assert "cols" not in lean and "rows" not in lean and lean["reads"].tobytes() == got["reads"].tobytes()
    return got, mine


def test_four_isoforms_and_a_cluster_of_haplotypes(ctx):
    T, reads, true = bc.property_case(bc.SEED)
    T2, reads2, _ = cc.isoform_case(cc.SEED)
    got, mine = _check(ctx, [T, T2], [reads, reads2])
    first = {"blocks": got["blocks"][0], "reads": got["reads"][mine[0]], "seg": got["seg"][0]}
    assert all(bc.property_holds(first, true))
    direct = first["reads"][first["reads"]["how"] == api.ISO_DIRECT]
    assert sorted(np.bincount(direct["group"], minlength=4).tolist()) == sorted(bc.SIZES)
    print("second segment:", got["seg"][1], got["blocks"][1])
    assert int(got["seg"][1]["n_reads"]) == 37
    _check(ctx, [T, T2], [reads, reads2], min_gap=30, min_alt=2, min_block=20, max_blocks=1)


def test_refusals_and_the_empty_call(ctx):
    ctx.align_set_pool([b"ACGTACGTAC", b"ACGTTCGTAC"])
    empty = ctx.align_pairs_blocks([], 11, [], [], tables=True)
    assert empty["blocks"] == [] and empty["reads"].shape == (0,) and empty["cols"].shape == (0,) and len(empty["score"]) == 0
    none = ctx.align_pairs_blocks([], 11, [(0, 0)], [])
    assert none["block_off"].tolist() == [0, 0] and int(none["seg"][0]["n_reads"]) == 0
    pairs = [(1, 0, 0, 0.1)]
    for bad in (dict(min_gap=0), dict(min_depth=0), dict(min_alt=0), dict(min_pct=51), dict(min_block=0), dict(max_blocks=33), dict(max_blocks=0)):
        with pytest.raises(api.IocError) as e:
            ctx.align_pairs_blocks(pairs, 11, [(0, 0)], [0], **bad)
        assert e.value.code == -1
    with pytest.raises(api.IocError) as e:
        ctx.align_pairs_blocks(pairs, 11, [(0, 0)], [0], cap=9)
    assert e.value.code == -4
    with pytest.raises(api.IocError):
        ctx.align_pairs_blocks(pairs, 11, [(0, 0)], [1])    # names no segment
    with pytest.raises(api.IocError):
        ctx.align_pairs_blocks(pairs, 11, [(2, 0)], [0])    # a segment outside the pool
    got = ctx.align_pairs_blocks(pairs, 11, [(0, 0)], [0])
    assert tuple(got["reads"][0][["first_row", "end_row", "group", "how"]]) == (0, 10, -1, api.ISO_RARE) and len(got["blocks"][0]) == 0
    got = ctx.align_pairs_blocks(pairs, 11, [(0, 0)], [0], min_depth=1, min_alt=1)   # (one read carries the key 0: an isoform)
    assert tuple(got["reads"][0][["first_row", "end_row", "group", "how"]]) == (0, 10, 0, api.ISO_DIRECT) and int(got["seg"][0]["n_groups"]) == 1
    assert got["rows"][0]["depth"].tolist() == [1] * 10 + [0]
