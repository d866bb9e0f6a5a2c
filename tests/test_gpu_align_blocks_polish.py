"""ioc_align_pairs_blocks_polish: ioc_align_pairs_blocks with the slot planes projected beside the two, and k_group_pile and the
call kernels over the planes behind the block kernels.  Everything align_pairs_blocks returns must equal that call's own result on
the same pairs, as bytes; the isoforms' sequences, qualities, records and iso_off must equal the host pipeline's, as bytes — the host
aligner, both host projections, api.planes_blocks and the definition (iso_polish_common.host_groups_polish).  On the property case
of test_iso_polish_host.py plus correct_common.isoform_case as a second segment, the pairs interleaved."""
import numpy as np
import pytest

from isonclust2_amd import api
from tests import blocks_common as bc
from tests import correct_common as cc
from tests import iso_polish_common as ic

pytestmark = pytest.mark.gpu

RULES = (dict(), dict(min_gap=30, min_alt=2, min_block=20, max_blocks=1))


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


@pytest.fixture(scope="module")
def case():
    """(frames, pool, pairs, seg_of_pair, segs, mine, host): the two segments with their pairs interleaved, and the host pipeline —
    planes once, and per rule the blocks of every segment."""
    T, reads, true = bc.property_case(ic.SEED)
    T2, reads2, _ = cc.isoform_case(cc.SEED)
    frames, groups = [T, T2], [reads, reads2]
    seqs, pairs = list(frames), []
    for g, rds in enumerate(groups):
        for rd in rds:
            pairs.append((len(seqs), g, 0, 0.1))
            seqs.append(rd)
    order = sorted(range(len(pairs)), key=lambda x: (sum(1 for y in range(x) if pairs[y][1] == pairs[x][1]), pairs[x][1]))
    pairs = [pairs[x] for x in order]
    sop = [p[1] for p in pairs]
    mine = [[x for x, s in enumerate(sop) if s == g] for g in range(2)]
    planes = [ic.host_planes(frames[sop[x]], [seqs[pairs[x][0]]]) for x in range(len(pairs))]
    base, slots = [p[0][0] for p in planes], [p[1][0] for p in planes]
    blocks = [[api.planes_blocks(np.array([base[x] for x in mine[g]], np.uint8), **{**bc.DEFAULT, **rule}) for g in range(2)] for rule in RULES]
    return dict(frames=frames, seqs=seqs, pairs=pairs, sop=sop, segs=[(0, 0), (1, 0)], mine=mine, base=base, slots=slots, blocks=blocks, true=true)


def _host(case, which, max_iso, min_depth):
    """the definition on the host pipeline's planes and isoforms: (what planes_polish_groups' dict holds, every pair's group)"""
    group = [-1] * len(case["pairs"])
    for g in range(2):
        for x, h in zip(case["mine"][g], case["blocks"][which][g]["reads"]["group"].tolist()):
            group[x] = h
    ng = [min(int(case["blocks"][which][g]["seg"]["n_groups"]), max_iso) for g in range(2)]
    return ic.host_groups_polish(case["frames"], case["sop"], group, ng, case["base"], case["slots"], min_depth), group, ng


BLOCK_KEYS = ("score", "windows", "ratio", "block_off", "reads", "seg", "stats", "cols", "row0")


def _same_blocks(got, plain):
    for f in BLOCK_KEYS:
        assert np.asarray(got[f]).tobytes() == np.asarray(plain[f]).tobytes(), f
    for f in ("blocks", "rows"):
        assert len(got[f]) == len(plain[f]) and all(a.tobytes() == b.tobytes() for a, b in zip(got[f], plain[f])), f


@pytest.mark.parametrize("which", [0, 1])
def test_against_the_blocks_call_and_the_host_pipeline(ctx, case, which):
    rule = RULES[which]
    ctx.align_set_pool(case["seqs"])
    plain = ctx.align_pairs_blocks(case["pairs"], 11, case["segs"], case["sop"], tables=True, stats=True, **rule)
    got = ctx.align_pairs_blocks_polish(case["pairs"], 11, case["segs"], case["sop"], tables=True, stats=True, **rule)
    _same_blocks(got, plain)
    bc.same_as_host(got, case["blocks"][which], case["mine"])
    want, _, ng = _host(case, which, 16, 3)
    ic.same_groups(got, want, tables=False)
    assert got["gseg_off"].tolist() == [0, ng[0], ng[0] + ng[1]] and ng[0] >= 1
    if which == 0:
        assert ng[0] == 4 and all(bc.property_holds({"blocks": got["blocks"][0], "reads": got["reads"][case["mine"][0]], "seg": got["seg"][0]}, case["true"]))
        # the distances pinned on the host path hold for the device's sequences
        iso = ic.true_isoforms(case["frames"][0])
        assert tuple(ic.edit_distance(got["gseq"][0][h], iso[ic.TRUE_OF[h]]) for h in range(4)) == ic.OWN
    lean = ctx.align_pairs_blocks_polish(case["pairs"], 11, case["segs"], case["sop"], rows=False, polish_min_depth=1, **rule)
    assert "cols" not in lean and "rows" not in lean and lean["reads"].tobytes() == got["reads"].tobytes()
    ic.same_groups(lean, _host(case, which, 16, 1)[0], tables=False)


@pytest.mark.parametrize("max_iso", [1, 2])
def test_max_iso_cuts_the_lists(ctx, case, max_iso):
    ctx.align_set_pool(case["seqs"])
    got = ctx.align_pairs_blocks_polish(case["pairs"], 11, case["segs"], case["sop"], max_iso=max_iso)
    want, group, ng = _host(case, 0, max_iso, 3)
    assert ng[0] == max_iso and len(got["gseq"][0]) == max_iso
    ic.same_groups(got, want, tables=False)
    assert got["reads"].tobytes() == ctx.align_pairs_blocks(case["pairs"], 11, case["segs"], case["sop"])["reads"].tobytes()
    # the reads of the uncalled isoforms are in no table: the called ones are those of the full call, read for read
    full = ctx.align_pairs_blocks_polish(case["pairs"], 11, case["segs"], case["sop"])
    assert got["gseq"][0] == full["gseq"][0][:max_iso] and got["gqual"][0] == full["gqual"][0][:max_iso]
    assert got["gpolish"][0].tobytes() == full["gpolish"][0][:max_iso].tobytes()
    cut = [h for h in group if h >= max_iso]
    assert len(cut) >= sum(sorted(bc.SIZES)[:4 - max_iso])   # (so there were reads to leave out)


def test_refusals_and_the_empty_call(ctx):
    ctx.align_set_pool([b"ACGTACGTAC", b"ACGTTCGTAC", b"ACGTTCGTACG"])
    empty = ctx.align_pairs_blocks_polish([], 11, [], [], tables=True)
    assert empty["blocks"] == [] and empty["reads"].shape == (0,) and empty["cols"].shape == (0,) and len(empty["score"]) == 0
    assert empty["gseq"] == [] and empty["gseg_off"].tolist() == [0]
    none = ctx.align_pairs_blocks_polish([], 11, [(0, 0)], [])
    assert none["block_off"].tolist() == [0, 0] and int(none["seg"][0]["n_reads"]) == 0 and none["gseq"] == [[]] and none["gseg_off"].tolist() == [0, 0]
    pairs, segs, sop = [(1, 0, 0, 0.1), (2, 0, 0, 0.1)], [(0, 0)], [0, 0]
    call = lambda **kw: ctx.align_pairs_blocks_polish(pairs, 11, segs, sop, **kw)
    for bad in (dict(max_iso=0), dict(max_iso=-1), dict(polish_min_depth=0), dict(iso_cap=-1), dict(polish_cap=-1), dict(min_gap=0), dict(min_depth=0),
                dict(min_alt=0), dict(min_pct=51), dict(min_block=0), dict(max_blocks=33), dict(max_blocks=0)):
        with pytest.raises(api.IocError) as e:
            call(**bad)
        assert e.value.code == -1, bad
    # the bounds: two reads, so at most min(max_iso, 2) isoforms of pileup_call_bound(10) bytes each
    assert api.blocks_polish_bound(10, 2, 16) == (2, 2 * api.pileup_call_bound(10)) and api.blocks_polish_bound(10, 2, 1) == (1, api.pileup_call_bound(10))
    for bad in (dict(iso_cap=1), dict(polish_cap=2 * api.pileup_call_bound(10) - 1), dict(cap=9), dict(max_iso=1, iso_cap=0),
                dict(max_iso=1, polish_cap=api.pileup_call_bound(10) - 1)):
        with pytest.raises(api.IocError) as e:
            call(**bad)
        assert e.value.code == -4, bad
    with pytest.raises(api.IocError):
        ctx.align_pairs_blocks_polish(pairs, 11, segs, [0, 1])       # names no segment
    with pytest.raises(api.IocError):
        ctx.align_pairs_blocks_polish(pairs, 11, [(3, 0)], sop)      # a segment outside the pool
    got = call(iso_cap=2, polish_cap=2 * api.pileup_call_bound(10))  # both reads are rare: no isoform, nothing called
    assert got["gseq"] == [[]] and int(got["seg"][0]["n_groups"]) == 0
    got = call(min_depth=1, min_alt=1, polish_min_depth=1, max_iso=1, iso_cap=1, polish_cap=api.pileup_call_bound(10))
    assert int(got["seg"][0]["n_groups"]) == 1 and got["reads"]["group"].tolist() == [0, 0] and got["gseg_off"].tolist() == [0, 1]
    assert len(got["gseq"][0]) == 1 and got["gseq"][0][0][:4] == b"ACGT" and len(got["gseq"][0][0]) in (10, 11)
