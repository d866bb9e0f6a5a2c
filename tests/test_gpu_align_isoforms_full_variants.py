"""The fused call ioc_align_pairs_isoforms_full_variants on the property case of variants_common (two exons at the first junction)
beside a segment where nothing splits: everything ioc_align_pairs_blocks_inserts_variants returns comes back byte for byte; the
isoforms' outputs are ioc_planes_isoforms_full_variants over the planes of the same alignments (the device's operation strings through
the host projections) with the groups, the key2 and the slots the run returned, and the host definition over the same; the property
and its pinned numbers hold on the device's bytes; and where nothing splits the isoforms are ioc_align_pairs_isoforms_full's."""
import numpy as np
import pytest

from isonclust2_amd import api
from tests import plane_pile_common as pp
from tests import splice_common as sc
from tests import splice_variants_common as svc
from tests import variants_common as vc

pytestmark = pytest.mark.gpu

# what the device path measures on the property case: the device's alignments give the host path's numbers (the test prints them)
PINNED_DEVICE = svc.PINNED


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _quiet():
    """variants_common.quiet_segment's reads as a segment of its own: reads 8 .. 11 lack both exons and are the frame itself"""
    reads = vc.quiet_segment()[0]
    assert reads[8] == reads[11] and len(reads[8]) == 300
    return reads[8], reads


def _pool(groups):
    """(sequences, pairs, seg_of_pair, segs) of [(frame, reads)]: the segments' pairs dealt out in turn"""
    seqs, pairs = [f for f, _ in groups], []
    for j in range(max(len(r) for _, r in groups)):
        for g, (_, reads) in enumerate(groups):
            if j < len(reads):
                pairs.append((len(seqs), g, 0, 0.1))
                seqs.append(reads[j])
    return seqs, pairs, [p[1] for p in pairs], [(g, 0) for g in range(len(groups))]


def _group_keys(sop, vreads, n_iso):
    goff = np.concatenate([[0], np.cumsum(n_iso)]).astype(np.int64)
    keys, seen = np.zeros(int(goff[-1]), np.uint64), set()
    for i, g in enumerate(sop):
        h = int(vreads[i]["group"])
        if int(vreads[i]["how"]) == api.ISO_DIRECT and 0 <= h < n_iso[g] and (g, h) not in seen:
            seen.add((g, h))
            keys[int(goff[g]) + h] = vreads[i]["key2"]
    return keys


def _planes_args(ctx, frames, seqs, pairs, sop, got, max_iso=16):
    """the arguments of planes_isoforms_full_variants from what a run returned and the planes of the same alignments"""
    base, slots = [], []
    for (q, _, _, _), g, ops in zip(pairs, sop, ctx.align_pairs_ops(pairs, 11)[3]):
        pb, ps = pp.planes_of(ops, seqs[q], len(frames[g]))
        base.append(np.asarray(pb, np.uint8)), slots.append(np.asarray(ps, np.uint8))
    v, ns = got["insert_variants"], len(frames)
    n_iso = [min(int(x), max_iso) for x in v["seg"]["n_groups"]]
    soff = [int(x) for x in got["inserts"]["site_off"]]
    group = [int(h) if int(h) < n_iso[g] else -1 for g, h in zip(sop, v["reads"]["group"])]
    cut = lambda a, k=1: [a[k * soff[g]:k * soff[g + 1]] for g in range(ns)]
    return (frames, sop, group, n_iso, base, slots, _group_keys(sop, v["reads"], n_iso), cut(v["win"]), cut(v["var"]), cut(v["seq"], 2), cut(v["qual"], 2))


@pytest.fixture(scope="module")
def run(ctx):
    frame, exons, reads, planted = vc.property_reads(vc.SEED)
    groups = [(frame, reads), _quiet()]
    seqs, pairs, sop, segs = _pool(groups)
    ctx.align_set_pool(seqs)
    plain = ctx.align_pairs_blocks_inserts_variants(pairs, 11, segs, sop, tables=True, stats=True)
    got = ctx.align_pairs_isoforms_full_variants(pairs, 11, segs, sop, tables=True, stats=True)
    frames = [f for f, _ in groups]
    return dict(frames=frames, seqs=seqs, pairs=pairs, sop=sop, segs=segs, plain=plain, got=got, args=_planes_args(ctx, frames, seqs, pairs, sop, got))


def _same(a, b, path=""):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for f in a:
            _same(a[f], b[f], path + "/" + f)
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for x, (u, v) in enumerate(zip(a, b)):
            _same(u, v, f"{path}[{x}]")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), path
    else:
        assert a == b, path


def test_what_the_variants_call_returns_comes_back_byte_for_byte(run):
    got = dict(run["got"])
    full = got.pop("isoforms_full")
    _same(got, run["plain"])
    v = got["insert_variants"]
    assert v["seg"]["n_split"].tolist() == [1, 0] and v["seg"]["n_groups"].tolist() == [4, 2] and got["inserts"]["seg"]["n_groups"].tolist() == [3, 2]
    assert [len(s) for s in full["gseq"]] == [4, 2] and full["gseg_off"].tolist() == [0, 4, 6]


def test_the_isoforms_are_planes_isoforms_full_variants_over_the_same_run(ctx, run):
    full = run["got"]["isoforms_full"]
    sc.same_full(full, ctx.planes_isoforms_full_variants(*run["args"]), tables=False)
    sc.same_full(full, svc.host_isoforms_full_variants(*run["args"], 3), tables=False)   # ... and the definition itself, from the host functions


def test_the_property_holds_on_the_device(ctx, run):
    got, args, sop = run["got"], run["args"], run["sop"]
    full, v, w = got["isoforms_full"], got["insert_variants"], got["insert_windows"]
    mine = [x for x, s in enumerate(sop) if s == 0]
    case = dict(group=v["reads"]["group"][mine], how=v["reads"]["how"][mine], n_groups=int(v["seg"]["n_groups"][0]), keys=args[6][:4])
    # beside it, over the same planes and groups: the unspliced call, and the parent's splice under key2 with the window call's windows
    unspliced = ctx.planes_polish_groups(*args[:6])
    soff = [int(x) for x in got["inserts"]["site_off"]]
    cut = lambda a: [a[soff[g]:soff[g + 1]] for g in range(2)]
    parent = ctx.planes_isoforms_full(*args[:7], cut(w["win"]), cut(w["seq"]), cut(w["qual"]))
    m = svc.measure(case, full["gseq"][0], parent["gseq"][0], unspliced["gseq"][0])
    print(m)
    assert all(svc.property_holds(m))
    assert m == PINNED_DEVICE
    for rec, (key2, _, _, _, _, _) in zip(full["splice"][:4], m):   # a DONE site is one the key2 carries, with either variant
        assert [int(s) == sc.DONE for s in rec["state"]] == [(key2 >> (2 * b)) & 3 in (svc.CARRY, svc.CARRY_B) for b in range(len(rec))]
    b = [h for h in range(4) if m[h][0] & 3 == svc.CARRY_B]
    assert len(b) == 1 and int(parent["splice"][b[0]][0]["state"]) == sc.LACK and int(full["splice"][b[0]][0]["len"]) == len(v["seq"][1]) > 0


def test_where_nothing_splits_the_isoforms_are_align_pairs_isoforms_full(ctx):
    f, reads = _quiet()
    seqs, pairs, sop, segs = _pool([(f, reads), (f, reads[:11])])   # (three reads that lack: the least a site needs on that side)
    ctx.align_set_pool(seqs)
    byvar = ctx.align_pairs_isoforms_full_variants(pairs, 11, segs, sop)
    parent = ctx.align_pairs_isoforms_full(pairs, 11, segs, sop)
    v = byvar["insert_variants"]
    assert int(byvar["inserts"]["site_off"][-1]) == 4 and v["seg"]["n_split"].tolist() == [0, 0] and int(parent["isoforms_full"]["sstats"]["n_done"].sum()) == 4
    assert v["reads"]["key2"].tolist() == byvar["inserts"]["reads"]["key"].tolist()
    _same(byvar["isoforms_full"], parent["isoforms_full"])


def test_no_site_kept_anywhere_is_align_pairs_isoforms_full(ctx):
    rng = np.random.default_rng(61)
    frames = [bytes(b"ACGT"[x] for x in rng.integers(0, 4, n)) for n in (400, 300)]
    mutate = lambda s: bytes(b"ACGT"[(b"ACGT".index(c) + 1) % 4] if rng.random() < 0.04 else c for c in s)
    seqs, pairs, sop, segs = _pool([(f, [mutate(f) for _ in range(7)]) for f in frames])
    ctx.align_set_pool(seqs)
    byvar = ctx.align_pairs_isoforms_full_variants(pairs, 11, segs, sop)
    assert int(byvar["inserts"]["site_off"][-1]) == 0 and byvar["isoforms_full"]["gseg_off"].tolist() == [0, 1, 2]
    _same(byvar["isoforms_full"], ctx.align_pairs_isoforms_full(pairs, 11, segs, sop)["isoforms_full"])


def test_max_iso_the_empty_call_and_the_refusals(ctx, run):
    pairs, sop, segs = run["pairs"], run["sop"], run["segs"]
    ctx.align_set_pool(run["seqs"])
    rlen, n_reads = [len(f) for f in run["frames"]], np.bincount(sop)
    cap, iso, rec = api.isoforms_full_bound(rlen, n_reads, 16)
    for kw in (dict(full_cap=cap - 1), dict(iso_cap=iso - 1), dict(splice_cap=rec - 1), dict(var_cap=api.insert_window_variants_bound(64) - 1)):
        with pytest.raises(api.IocError) as e:
            ctx.align_pairs_isoforms_full_variants(pairs, 11, segs, sop, **kw)
        assert e.value.code == -4, kw
    for kw in (dict(max_iso=0), dict(min_agree=0)):
        with pytest.raises(api.IocError) as e:
            ctx.align_pairs_isoforms_full_variants(pairs, 11, segs, sop, **kw)
        assert e.value.code == -1, kw
    full = run["got"]["isoforms_full"]
    _same(ctx.align_pairs_isoforms_full_variants(pairs, 11, segs, sop, full_cap=cap, iso_cap=iso, splice_cap=rec)["isoforms_full"], full)   # exactly the bounds
    two = ctx.align_pairs_isoforms_full_variants(pairs, 11, segs, sop, max_iso=2, max_sites=4, max_win=200)["isoforms_full"]   # a small room, the first two isoforms
    assert [s[:2] for s in full["gseq"]] == two["gseq"] and two["gseg_off"].tolist() == [0, 2, 4]
    empty = ctx.align_pairs_isoforms_full_variants([], 11, [], [])
    assert empty["isoforms_full"]["gseq"] == [] and empty["isoforms_full"]["off"].tolist() == [0] and empty["isoforms_full"]["splice_off"].tolist() == [0]
    assert len(empty["insert_variants"]["var"]) == 0
