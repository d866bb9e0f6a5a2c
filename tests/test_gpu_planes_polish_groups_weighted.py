"""ioc_planes_polish_groups_weighted: k_group_pile_weighted and the weighted call kernels over host planes and weight planes that
are uploaded, against the definition — the counts ioc_host_planes_pile and the weights ioc_host_planes_pile_weighted add up from
the reads of every group, and ioc_host_pileup_call_weighted on them.  One call holds the shapes of
test_gpu_planes_polish_groups.py — segments of 0, 1, 63, 64, 65, 255, 256, 257 and 600 bases, 0, 1, 2, 3, 5 and 70 groups, groups
of 0, 1, 3, 4, 5, 7, 8, 9, 65, 130, 257 and 261 reads, reads in -1, a segment whose reads are all in -1, a segment with reads but
no groups, the pairs interleaved — and segments of 62, 127 and 128 bases with groups of 2 and 6 reads; every weight byte is drawn
from 0, 1, 2, 40, 93 and 255.  Sequences, qualities, offsets, records and the three tables are compared as bytes, and gcols with
what planes_polish_groups returns for the same planes."""
import ctypes as C

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import iso_polish_weight_common as iw
from tests import plane_pile_common as pp
from tests import test_gpu_planes_polish_groups as plain

pytestmark = pytest.mark.gpu

WEIGHTS = (0, 1, 2, 40, 93, 255)
SHAPES = plain.SHAPES + [(62, (2, 6), 1), (127, (6, 2, 1), 0), (128, (4,), 2)]
NO_GROUPS, ALL_NONE, MANY = plain.NO_GROUPS, plain.ALL_NONE, plain.MANY


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _weights(rng, base):
    """weight planes for the pairs whose base planes these are: every byte from WEIGHTS, covered or not"""
    draw = lambda shape: rng.choice(np.array(WEIGHTS, np.uint8), size=shape)
    return [draw(len(b)) for b in base], [draw((pp.SLOTS, len(b))) for b in base]


def _case(shapes, seed=11):
    frames, sop, group, ng, base, slots = plain._case(shapes, seed)
    wbase, wslots = _weights(np.random.default_rng(seed), base)
    return frames, sop, group, ng, base, slots, wbase, wslots


@pytest.fixture(scope="module")
def case():
    c = _case(SHAPES)
    return c, {md: iw.host_groups_polish_weighted(*c, md) for md in (1, 3)}


def test_the_shapes_are_the_ones_the_kernel_can_go_wrong_at():
    assert sorted({s[0] for s in SHAPES}) == [0, 1, 62, 63, 64, 65, 127, 128, 255, 256, 257, 600]
    assert sorted({len(s[1]) for s in SHAPES}) == [0, 1, 2, 3, 5, 70]
    assert sorted({n for s in SHAPES for n in s[1]}) == list(range(10)) + [65, 130, 257, 261]


@pytest.mark.parametrize("min_depth", [1, 3])
def test_against_the_definition(ctx, case, min_depth):
    c, want = case
    frames, sop, group, ng, base, slots, wbase, wslots = c
    got = ctx.planes_polish_groups_weighted(*c, min_depth=min_depth, tables=True)
    iw.same_groups_weighted(got, want[min_depth])
    # gcols is k_group_pile's, byte for byte; ins_runs / ins_bases of gwcols and longer / reserved of gwins are 0
    unweighted = ctx.planes_polish_groups(frames, sop, group, ng, base, slots, min_depth=min_depth, tables=True)
    assert got["gcols"].tobytes() == unweighted["gcols"].tobytes() and got["grow0"].tolist() == unweighted["grow0"].tolist()
    assert not got["gwcols"]["ins_runs"].any() and not got["gwcols"]["ins_bases"].any() and not got["gwins"]["longer"].any()
    assert got["gwins"].tobytes() != unweighted["gins"].tobytes() and got["gqual"] != unweighted["gqual"]   # (the weights count for something)
    big = got["gpolish"][8]
    assert all(int(big[h]["n_ins"]) + int(big[h]["n_sub"]) + int(big[h]["n_del"]) > 0 for h in (0, 1))
    # the segment without groups returns nothing; groups without reads and the segment whose reads are all in -1: the frame at quality '!'
    assert got["gseq"][NO_GROUPS] == [] and len(got["gpolish"][NO_GROUPS]) == 0
    empty = [(ALL_NONE, 0), (ALL_NONE, 1), (ALL_NONE, 2), (1, 1), (4, 0)] + [(MANY, h) for h in range(70) if SHAPES[MANY][1][h] == 0]
    assert len(empty) > 10
    for g, h in empty:
        assert got["gseq"][g][h] == frames[g] and got["gqual"][g][h] == b"!" * len(frames[g]) and int(got["gpolish"][g][h]["n_low"]) == len(frames[g])
        r0 = int(got["grow0"][int(got["gseg_off"][g]) + h])
        rows = slice(r0, r0 + len(frames[g]) + 1)
        assert not any(got[f][rows].tobytes().strip(b"\0") for f in ("gcols", "gwcols", "gwins"))
    lean = ctx.planes_polish_groups_weighted(*c, min_depth=min_depth)
    assert "gcols" not in lean and "gwcols" not in lean
    iw.same_groups_weighted(lean, want[min_depth], tables=False)


def test_nothing_is_carried_between_calls(ctx, case):
    """A small call behind the large one on the same context: the tables are the small call's alone."""
    c, _ = case
    frames, sop, group, ng = c[:4]
    ctx.planes_polish_groups_weighted(*c, tables=True)
    keep = [i for i in range(len(sop)) if sop[i] in (2, 5)][:40]
    remap = {2: 1, 5: 0}
    small = ([frames[5], frames[2]], [remap[sop[i]] for i in keep], [group[i] for i in keep], [ng[5], ng[2]]) + tuple([planes[i] for i in keep] for planes in c[4:])
    iw.same_groups_weighted(ctx.planes_polish_groups_weighted(*small, min_depth=2, tables=True), iw.host_groups_polish_weighted(*small, 2))


def test_the_empty_call_and_segments_without_pairs(ctx):
    empty = ctx.planes_polish_groups_weighted([], [], [], [], [], [], [], [], tables=True)
    assert empty["gseq"] == [] and empty["gpolish"] == [] and empty["gcols"].shape == (0,) and empty["gwins"].shape == (0,) and empty["gseg_off"].tolist() == [0]
    frames = [b"ACGTN", b"", b"GG", b"TTT"]
    got = ctx.planes_polish_groups_weighted(frames, [], [], [3, 2, 0, 1], [], [], [], [], tables=True)
    assert got["gseq"] == [[frames[0]] * 3, [b""] * 2, [], [b"TTT"]] and got["gqual"] == [[b"!!!!!"] * 3, [b""] * 2, [], [b"!!!"]]
    assert not got["gwcols"].tobytes().strip(b"\0") and len(got["gwcols"]) == 3 * 6 + 2 * 1 + 4
    iw.same_groups_weighted(got, iw.host_groups_polish_weighted(frames, [], [], [3, 2, 0, 1], [], [], [], [], 3))


def test_refusals_write_nothing(ctx):
    L = _lib.load()
    frames = [b"ACGT", b"GATTACA"]
    sop, group, ng = np.array([0, 1, 1], np.int32), np.array([0, 2, -1], np.int32), np.array([1, 3], np.int32)
    rlen, f_off = np.array([4, 7], np.int32), np.array([0, 4], np.int64)
    P = 5 + 8 + 8
    base, slots = np.zeros(P, np.uint8), np.zeros(pp.SLOTS * P, np.uint8)
    wbase, wslots = np.full(P, 7, np.uint8), np.full(pp.SLOTS * P, 7, np.uint8)
    bound = api.pileup_call_bound(4) + 3 * api.pileup_call_bound(7)
    rows = 5 + 3 * 8
    seq, qual = np.full(bound, 0xA5, np.uint8), np.full(bound, 0xA5, np.uint8)
    off, pol = np.full(5, -9, np.int64), np.full(4 * 8, -9, np.int32)
    gcols, gwcols, gwins = np.full(rows * 8, 0xA5A5A5A5, np.uint32), np.full(rows * 8, 0xA5A5A5A5, np.uint32), np.full(rows * 32, 0xA5A5A5A5, np.uint32)
    p32, p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)), lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    d = lambda a: a.ctypes.data

    def call(ns=2, np_=3, rlen_=rlen, frames_=b"".join(frames), f_off_=f_off, ng_=ng, sop_=sop, group_=group, base_=d(base), slots_=d(slots), wbase_=d(wbase),
             wslots_=d(wslots), md=3, seq_=d(seq), qual_=d(qual), cap=bound, off_=off):
        arr = lambda a: None if a is None else np.asarray(a, np.int32)   # (alive until the call returns)
        s_arr, g_arr, n_arr = arr(sop_), arr(group_), arr(ng_)
        ptr = lambda a: p32(a) if a is not None else None
        return L.ioc_planes_polish_groups_weighted(ctx.h, ns, ptr(rlen_), frames_, p64(f_off_) if f_off_ is not None else None, ptr(n_arr), np_, ptr(s_arr), ptr(g_arr),
                                                   base_, slots_, wbase_, wslots_, md, seq_, qual_, cap, p64(off_) if off_ is not None else None, d(pol), d(gcols),
                                                   d(gwcols), d(gwins))

    # what ioc_planes_polish_groups refuses
    assert call(md=0) == -1 and call(ns=-1) == -1 and call(np_=-1) == -1 and call(cap=-1) == -1
    assert call(sop_=[0, 2, 1]) == -1 and call(sop_=[-1, 1, 1]) == -1
    assert call(rlen_=np.array([4, -1], np.int32)) == -1 and call(f_off_=np.array([0, -4], np.int64)) == -1
    assert call(rlen_=None) == -1 and call(f_off_=None) == -1 and call(frames_=None) == -1 and call(sop_=None) == -1 and call(group_=None) == -1
    assert call(base_=None) == -1 and call(slots_=None) == -1 and call(off_=None) == -1 and call(seq_=None) == -1 and call(qual_=None) == -1
    assert call(ng_=[1, -1]) == -1 and call(ng_=[-3, 3]) == -1 and call(ng_=None) == -1
    assert call(group_=[1, 2, -1]) == -1 and call(group_=[0, 3, -1]) == -1 and call(group_=[0, 2, -2]) == -1 and call(group_=[0, 2, 255]) == -1
    assert call(ng_=[0, 3]) == -1                                  # (pair 0 is in group 0 of a segment without groups)
    assert call(ng_=[2**31 - 1, 3], cap=2**62) == -1 and call(ng_=[2**30, 2**30], cap=2**62) == -1
    assert call(cap=bound - 1) == -4
    # a NULL weight plane with pairs
    assert call(wbase_=None) == -1 and call(wslots_=None) == -1
    assert (seq == 0xA5).all() and (qual == 0xA5).all() and (off == -9).all() and (pol == -9).all()
    assert (gcols == 0xA5A5A5A5).all() and (gwcols == 0xA5A5A5A5).all() and (gwins == 0xA5A5A5A5).all()
    assert call() == 0 and off[0] == 0 and off[4] == 4 + 3 * 7   # (no insertions in planes of zeros, and A at every covered row)
    assert gcols.view(api.PILEUP_DTYPE)["a"].tolist() == [1] * 5 + [0] * 8 + [0] * 8 + [1] * 8
    assert gwcols.view(api.PILEUP_DTYPE)["a"].tolist() == [7] * 5 + [0] * 8 + [0] * 8 + [7] * 8 and not gwins.any()
    assert call(np_=0, sop_=None, group_=None, base_=None, slots_=None, wbase_=None, wslots_=None) == 0   # without pairs the planes may be NULL
