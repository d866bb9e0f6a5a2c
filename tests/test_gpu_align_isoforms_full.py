"""The fused call ioc_align_pairs_isoforms_full on the property cases A and B, at the host test's seeds, case B on a
reverse-complemented representative: everything ioc_align_pairs_blocks_inserts_seq returns comes back byte for byte; the isoforms'
outputs are ioc_planes_isoforms_full over the planes of the same alignments (the device's operation strings through the host
projections) with the groups, the keys and the windows the run returned; and the property holds on the device's bytes as on the
host's — the first call that projects the slot planes, the length plane and the position plane together."""
import numpy as np
import pytest

from isonclust2_amd import api
from tests import blocks_common as bc
from tests import inserts_common as ic
from tests import plane_pile_common as pp
from tests import splice_common as sc

pytestmark = pytest.mark.gpu

COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


@pytest.fixture(scope="module")
def run(ctx):
    Ta, reads_a, _ = bc.property_case(sc.SEED_A)
    Tb, reads_b, _ = bc.property_case(sc.SEED_B)
    frames = [ic.representative(Ta, "A"), ic.representative(Tb, "B")]
    seqs = [frames[0], frames[1].translate(COMP)[::-1]]   # segment 1 sits on the reverse complement: its frame is read backwards
    segs, pairs = [(0, 0), (1, 1)], []
    for j in range(max(len(reads_a), len(reads_b))):      # the segments' pairs dealt out in turn
        for g, reads in enumerate((reads_a, reads_b)):
            if j < len(reads):
                pairs.append((len(seqs), g, g, 0.1))
                seqs.append(reads[j])
    sop = [p[1] for p in pairs]
    ctx.align_set_pool(seqs)
    plain = ctx.align_pairs_blocks_inserts_seq(pairs, 11, segs, sop, tables=True, stats=True)
    got = ctx.align_pairs_isoforms_full(pairs, 11, segs, sop, tables=True, stats=True)
    # the planes of the same alignments: the device's operation strings through the host projections
    base, slots = [], []
    for (q, _, _, _), g, ops in zip(pairs, sop, ctx.align_pairs_ops(pairs, 11)[3]):
        pb, ps = pp.planes_of(ops, seqs[q], len(frames[g]))
        base.append(np.asarray(pb, np.uint8)), slots.append(np.asarray(ps, np.uint8))
    ir, w = got["inserts"], got["insert_windows"]
    n_groups = [int(x) for x in ir["seg"]["n_groups"]]
    soff = [int(x) for x in ir["site_off"]]
    cut = lambda a: [a[soff[g]:soff[g + 1]] for g in range(2)]
    args = (frames, sop, ir["reads"]["group"].tolist(), n_groups, base, slots, sc.group_keys(2, sop, ir["reads"], n_groups), cut(w["win"]), cut(w["seq"]), cut(w["qual"]))
    return dict(T=(Ta, Tb), frames=frames, pairs=pairs, sop=sop, plain=plain, got=got, args=args)


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


def test_what_the_window_call_returns_comes_back_byte_for_byte(run):
    got = dict(run["got"])
    full = got.pop("isoforms_full")
    _same(got, run["plain"])
    assert [len(s) for s in full["gseq"]] == [4, 4] and full["gseg_off"].tolist() == [0, 4, 8]


def test_the_isoforms_are_planes_isoforms_full_over_the_same_run(ctx, run):
    full = run["got"]["isoforms_full"]
    sc.same_full(full, ctx.planes_isoforms_full(*run["args"]), tables=False)
    sc.same_full(full, sc.host_isoforms_full(*run["args"], 3), tables=False)   # ... and the definition itself, from the host functions


@pytest.mark.parametrize("g,which", [(0, "A"), (1, "B")])
def test_the_property_holds_on_the_device(ctx, run, g, which):
    full, ir = run["got"]["isoforms_full"], run["got"]["inserts"]
    mine = [x for x, s in enumerate(run["sop"]) if s == g]
    # the unspliced call of the same tables: ioc_planes_polish_groups over the same planes and groups
    plain = ctx.planes_polish_groups(*run["args"][:6])
    measured = sc.measure(which, run["T"][g], ir["reads"][mine], full["gseq"][g], plain["gseq"][g])
    print(which, measured)
    assert sc.property_holds(which, measured)
    assert measured == (sc.PINNED_A if which == "A" else sc.PINNED_B)   # the device's bytes are the host path's
    recs = full["splice"][int(full["gseg_off"][g]):int(full["gseg_off"][g + 1])]
    for rec, (x, _, _) in zip(recs, measured):
        assert sum(sc.EXONS[which][b] for b in range(len(rec)) if int(rec[b]["state"]) == sc.DONE) == sc.carried(which, x)


def test_refusals_and_the_empty_call(ctx, run):
    pairs, sop, segs = run["pairs"], run["sop"], [(0, 0), (1, 1)]
    n_reads = np.bincount(sop)
    rlen = [len(f) for f in run["frames"]]
    cap, iso, rec = api.isoforms_full_bound(rlen, n_reads, 16)
    for kw in (dict(full_cap=cap - 1), dict(iso_cap=iso - 1), dict(splice_cap=rec - 1)):
        with pytest.raises(api.IocError) as e:
            ctx.align_pairs_isoforms_full(pairs, 11, segs, sop, **kw)
        assert e.value.code == -4, kw
    with pytest.raises(api.IocError) as e:
        ctx.align_pairs_isoforms_full(pairs, 11, segs, sop, max_iso=0)
    assert e.value.code == -1
    two = ctx.align_pairs_isoforms_full(pairs, 11, segs, sop, max_iso=2, max_sites=4, max_win=200)["isoforms_full"]   # a small room, the first two isoforms
    full = run["got"]["isoforms_full"]
    assert [s[:2] for s in full["gseq"]] == two["gseq"]
    empty = ctx.align_pairs_isoforms_full([], 11, [], [])["isoforms_full"]
    assert empty["gseq"] == [] and empty["off"].tolist() == [0] and empty["splice_off"].tolist() == [0]
