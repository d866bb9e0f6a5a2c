"""ioc_align_pairs_blocks_inserts: ioc_align_pairs_blocks with the length plane projected beside the base plane and the insert
kernels behind the block kernels.  Everything align_pairs_blocks returns must equal that call's own result, byte for byte; sites,
records and the row table must equal the host pipeline's, as bytes — the host aligner, ioc_host_ops_project,
ioc_host_ops_project_ilen, ioc_host_planes_blocks and ioc_host_planes_inserts with the block stage's keys and masks —; and both
property cases of test_planes_inserts_host.py must hold on the device.  Also a batch with empty queries, and the refusals."""
import numpy as np
import pytest

from isonclust2_amd import api
from tests import blocks_common as bc
from tests import inserts_common as ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _host(frame, reads, rule, irule):
    """the host pipeline of one segment: (blocks, inserts)"""
    if reads:
        base, ilen = ic.host_planes(frame, reads)
    else:
        base = ilen = np.zeros((0, len(frame) + 1), np.uint8)
    blocks = api.planes_blocks(base, **{**bc.DEFAULT, **rule})
    nb = len(blocks["blocks"])
    mask = np.array([sum(3 << (2 * b) for b in range(nb) if (int(k) >> (2 * b)) & 3 != bc.NOT) for k in blocks["reads"]["key"]], np.uint64)
    shared = {k: {**bc.DEFAULT, **rule}[k] for k in ("min_depth", "min_alt", "min_pct")}
    return blocks, api.planes_inserts(base, ilen, pre_key=blocks["reads"]["key"], pre_mask=mask, pre_full=(1 << (2 * nb)) - 1, **{**ic.DEFAULT, **shared, **irule})


def _check(ctx, frames, groups, rule={}, irule={}):
    """frames[g] with the reads groups[g], their pairs interleaved: the fused call against align_pairs_blocks and the host pipeline"""
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
    plain = ctx.align_pairs_blocks(pairs, 11, segs, sop, tables=True, stats=True, **rule)
    got = ctx.align_pairs_blocks_inserts(pairs, 11, segs, sop, tables=True, stats=True, **rule, **irule)
    for f in ("score", "windows", "ratio", "block_off", "reads", "seg", "stats", "cols", "row0"):
        assert got[f].tobytes() == plain[f].tobytes(), f
    for f in ("blocks", "rows"):
        assert [x.tobytes() for x in got[f]] == [x.tobytes() for x in plain[f]], f
    mine = [[x for x, s in enumerate(sop) if s == g] for g in range(len(frames))]
    host = [_host(frame, [seqs[pairs[x][0]] for x in mine[g]], rule, irule) for g, frame in enumerate(frames)]
    bc.same_as_host(got, [h[0] for h in host], mine)
    ic.same_as_host(got["inserts"], [h[1] for h in host], mine)
    lean = ctx.align_pairs_blocks_inserts(pairs, 11, segs, sop, rows=False, **rule, **irule)
    assert "cols" not in lean and "rows" not in lean and "rows" not in lean["inserts"]
    assert lean["inserts"]["reads"].tobytes() == got["inserts"]["reads"].tobytes() and lean["reads"].tobytes() == got["reads"].tobytes()
    return got, mine


def test_both_properties_on_the_device(ctx):
    Ta, reads_a, _ = bc.property_case(ic.SEED_A)
    Tb, reads_b, _ = bc.property_case(ic.SEED_B)
    got, mine = _check(ctx, [ic.representative(Ta, "A"), ic.representative(Tb, "B")], [reads_a, reads_b])
    ins = got["inserts"]
    first = {"sites": ins["sites"][0], "reads": ins["reads"][mine[0]], "seg": ins["seg"][0]}
    print("A:", first["sites"], first["seg"])
    assert all(ic.property_a_holds(first)) and int(got["seg"][0]["n_groups"]) == 1   # (the block stage alone sees one isoform of four)
    second = {"sites": ins["sites"][1], "reads": ins["reads"][mine[1]], "seg": ins["seg"][1]}
    print("B:", got["blocks"][1], second["sites"], second["seg"])
    assert all(ic.property_b_holds({"seg": got["seg"][1]}, second))
    _check(ctx, [ic.representative(Ta, "A"), ic.representative(Tb, "B")], [reads_a, reads_b], rule=dict(min_alt=2, max_blocks=1), irule=dict(min_ins=30, slack=3, max_sites=1))


def test_a_batch_with_empty_queries(ctx):
    T, reads, _ = bc.property_case(ic.SEED_A)
    frame = ic.representative(T, "A")
    some = reads[:8] + [b""] + reads[12:18] + [b""] + reads[22:26]
    got, mine = _check(ctx, [frame, frame[:300]], [some, [b"", reads[38][:250]]], rule=dict(min_depth=2, min_alt=2), irule={})
    empty = [x for x in mine[0] if int(got["reads"][x]["end_row"]) == 0]
    assert len(empty) == 2 and all(int(got["inserts"]["reads"][x]["n_near"]) == 0 and int(got["inserts"]["reads"][x]["ins_bases"]) == 0 for x in empty)
    ns = len(got["inserts"]["sites"][0])
    assert ns >= 2 and all(row == [ic.NOT] * ns for row in ic.states(got["inserts"]["reads"][empty], ns))


def test_refusals_and_the_empty_call(ctx):
    ctx.align_set_pool([b"ACGTACGTAC", b"ACGTTCGTAC"])
    empty = ctx.align_pairs_blocks_inserts([], 11, [], [], tables=True)
    assert empty["blocks"] == [] and empty["inserts"]["sites"] == [] and empty["inserts"]["reads"].shape == (0,) and len(empty["score"]) == 0
    none = ctx.align_pairs_blocks_inserts([], 11, [(0, 0)], [])
    assert none["inserts"]["site_off"].tolist() == [0, 0] and int(none["inserts"]["seg"][0]["n_reads"]) == 0
    pairs = [(1, 0, 0, 0.1)]
    for bad in (dict(min_gap=0), dict(min_depth=0), dict(min_pct=51), dict(max_blocks=33), dict(min_ins=0), dict(min_ins=256), dict(slack=-1), dict(slack=33),
                dict(max_sites=0), dict(max_sites=33)):
        with pytest.raises(api.IocError) as e:
            ctx.align_pairs_blocks_inserts(pairs, 11, [(0, 0)], [0], **bad)
        assert e.value.code == -1, bad
    for short in (dict(cap=9), dict(sites_cap=8)):
        with pytest.raises(api.IocError) as e:
            ctx.align_pairs_blocks_inserts(pairs, 11, [(0, 0)], [0], **short)
        assert e.value.code == -4, short
    with pytest.raises(api.IocError):
        ctx.align_pairs_blocks_inserts(pairs, 11, [(0, 0)], [1])    # names no segment
    with pytest.raises(api.IocError):
        ctx.align_pairs_blocks_inserts(pairs, 11, [(2, 0)], [0])    # a segment outside the pool
    got = ctx.align_pairs_blocks_inserts(pairs, 11, [(0, 0)], [0], min_depth=1, min_alt=1)   # (one read carries the pair (0, 0): an isoform)
    assert tuple(got["inserts"]["reads"][0][["group", "how", "n_near", "ins_bases"]]) == (0, api.ISO_DIRECT, 0, 0) and int(got["inserts"]["seg"][0]["n_groups"]) == 1
    assert got["inserts"]["rows"][0]["span"].tolist() == [0] + [1] * 9 + [0]
