"""ioc_planes_polish_groups: k_group_pile and the call kernels over host planes that are uploaded, against the definition — the
tables ioc_host_planes_pile adds up from the reads of every group, and ioc_host_pileup_call on them.  One call holds segments of 0,
1, 63, 64, 65, 255, 256, 257 and 600 bases (around the 64 rows of a work item and the 256 of a step of the call kernels) with 0, 1,
2, 3, 5 and 70 groups, and groups of 0, 1, 3, 4, 5, 7, 8, 9, 65 and 130 reads (around the four waves of a workgroup, around the
eight members of a round, one and two past a multiple) and of 257 and 261 (past the 64 steps a wave knows ahead), reads in -1, a
segment whose reads are all in -1, a segment with reads but no groups, and the segments' pairs interleaved.  Tables, sequences,
qualities, records and offsets are compared as bytes."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import iso_polish_common as ic
from tests import plane_pile_common as pp

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 3, 4, 5, 7, 8, 9, 65, 130)
# (rlen, reads of group 0, 1, .., reads in -1)
SHAPES = [
    (0, (1, 3), 2), (1, (3, 0, 4), 1), (63, (65, 1, 5, 7, 8), 3), (64, (9,), 0), (65, (0, 130), 2), (255, (130, 3, 4), 5),
    (256, tuple(SIZES[(3 * h) % 8] for h in range(70)), 1), (257, (), 4), (600, (65, 130, 8, 9, 5), 7), (64, (0, 0, 0), 3), (65, (257, 261), 0),
]
NO_GROUPS, ALL_NONE, MANY = 7, 9, 6


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _reads(rng, frame, count):
    """`count` reads of one group on `frame`: a sequence of the group's own that most of its reads follow — substitutions,
    deletions, insertions of 1 to 6 bases — and every byte from the legal sets."""
    rlen = len(frame)
    truth_b = [rng.choice((0, 1, 2, 3, 4, pp.DEL)) if rng.random() < 0.2 else {65: 0, 67: 1, 71: 2, 84: 3}.get(frame[r], 4) for r in range(rlen)]
    truth_i = {r: [rng.randrange(1, 6) for _ in range(rng.randrange(1, 7))] for r in range(rlen + 1) if rng.random() < 0.08}
    out = []
    for _ in range(count):
        first, last = (0, rlen) if rng.random() < 0.6 else sorted((rng.randrange(rlen + 1), rng.randrange(rlen + 1)))
        base = np.full(rlen + 1, pp.NONE, np.uint8)
        slots = np.zeros((pp.SLOTS, rlen + 1), np.uint8)
        for r in range(first, last):
            base[r] = rng.choice(pp.BASE_BYTES[:6]) if rng.random() < 0.1 else truth_b[r]
        for r in range(first, last + 1):
            run = truth_i.get(r, []) if rng.random() < 0.85 else [rng.randrange(1, 6) for _ in range(rng.randrange(0, 7))]
            for j, s in enumerate(run):
                slots[j, r] = s
        out.append((base, slots))
    return out


def _case(shapes, seed=11):
    """(frames, seg_of_pair, group, n_groups, base planes, slot planes) with the pairs of the segments interleaved and the groups mixed"""
    rng = random.Random(seed)
    frames, pairs = [], []
    for g, (rlen, sizes, none) in enumerate(shapes):
        frame = bytes(rng.choice(b"ACGTN") for _ in range(rlen))
        frames.append(frame)
        for h, count in list(enumerate(sizes)) + [(-1, none)]:
            pairs += [(g, h, b, s) for b, s in _reads(rng, frame, count)]
    rng.shuffle(pairs)
    return frames, [p[0] for p in pairs], [p[1] for p in pairs], [len(s[1]) for s in shapes], [p[2] for p in pairs], [p[3] for p in pairs]


@pytest.fixture(scope="module")
def case():
    frames, sop, group, ng, base, slots = _case(SHAPES)
    return frames, sop, group, ng, base, slots, {md: ic.host_groups_polish(frames, sop, group, ng, base, slots, md) for md in (1, 3)}


def test_the_shapes_are_the_ones_the_kernel_can_go_wrong_at():
    assert sorted({s[0] for s in SHAPES}) == [0, 1, 63, 64, 65, 255, 256, 257, 600]
    assert sorted({len(s[1]) for s in SHAPES}) == [0, 1, 2, 3, 5, 70]
    assert sorted({n for s in SHAPES for n in s[1]}) == list(SIZES) + [257, 261]   # (the last two: a second chunk of steps in every wave)


@pytest.mark.parametrize("min_depth", [1, 3])
def test_against_the_definition(ctx, case, min_depth):
    frames, sop, group, ng, base, slots, want = case
    got = ctx.planes_polish_groups(frames, sop, group, ng, base, slots, min_depth=min_depth, tables=True)
    ic.same_groups(got, want[min_depth])
    # something was called: insertions, substitutions and deletions in the large groups
    big = got["gpolish"][8]
    assert all(int(big[h]["n_ins"]) > 0 and int(big[h]["n_sub"]) > 0 and int(big[h]["n_del"]) > 0 for h in (0, 1))
    # the segment without groups returns nothing; groups without reads and the segment whose reads are all in -1: the frame at quality '!'
    assert got["gseq"][NO_GROUPS] == [] and len(got["gpolish"][NO_GROUPS]) == 0
    empty = [(ALL_NONE, 0), (ALL_NONE, 1), (ALL_NONE, 2), (1, 1), (4, 0)] + [(MANY, h) for h in range(70) if SHAPES[MANY][1][h] == 0]
    assert len(empty) > 10
    for g, h in empty:
        assert got["gseq"][g][h] == frames[g] and got["gqual"][g][h] == b"!" * len(frames[g]) and int(got["gpolish"][g][h]["n_low"]) == len(frames[g])
        r0 = int(got["grow0"][int(got["gseg_off"][g]) + h])
        rows = slice(r0, r0 + len(frames[g]) + 1)
        assert not got["gcols"][rows].tobytes().strip(b"\0") and not got["gins"][rows].tobytes().strip(b"\0")
    lean = ctx.planes_polish_groups(frames, sop, group, ng, base, slots, min_depth=min_depth)
    assert "gcols" not in lean
    ic.same_groups(lean, want[min_depth], tables=False)


# the shapes of the two-group test (tests/test_gpu_planes_polish.py): (rlen, reads of group 0, of group 1, of neither)
TWO = [(0, 1, 3, 2), (1, 3, 0, 1), (63, 65, 1, 3), (64, 0, 65, 0), (255, 130, 3, 5), (256, 3, 130, 1), (257, 0, 0, 4), (600, 65, 130, 7)]


@pytest.mark.parametrize("min_depth", [1, 3])
def test_two_groups_everywhere_equal_the_split_polish_byte_for_byte(ctx, min_depth):
    frames, sop, group, ng, base, slots = _case([(rlen, (n0, n1), nn) for rlen, n0, n1, nn in TWO], seed=9)
    assert ng == [2] * len(TWO)
    old = ctx.planes_polish(frames, sop, [h if h >= 0 else pp.SPLIT_NONE for h in group], base, slots, min_depth=min_depth, tables=True)
    new = ctx.planes_polish_groups(frames, sop, group, ng, base, slots, min_depth=min_depth, tables=True)
    assert new["gseq"] == old["gseq"] and new["gqual"] == old["gqual"]
    assert np.concatenate(new["gpolish"]).tobytes() == old["gpolish"].tobytes()
    assert new["gcols"].tobytes() == old["gcols"].tobytes() and new["gins"].tobytes() == old["gins"].tobytes()
    assert new["grow0"].tolist() == old["grow0"].reshape(-1).tolist()
    assert new["gseg_off"].tolist() == list(range(0, 2 * len(TWO) + 1, 2))


def test_nothing_is_carried_between_calls(ctx, case):
    """A small call behind the large one on the same context: the tables are the small call's alone."""
    frames, sop, group, ng, base, slots, want = case
    ctx.planes_polish_groups(frames, sop, group, ng, base, slots, tables=True)
    keep = [i for i in range(len(sop)) if sop[i] in (2, 5)][:40]
    remap = {2: 1, 5: 0}
    small = ([frames[5], frames[2]], [remap[sop[i]] for i in keep], [group[i] for i in keep], [ng[5], ng[2]], [base[i] for i in keep], [slots[i] for i in keep])
    ic.same_groups(ctx.planes_polish_groups(*small, min_depth=2, tables=True), ic.host_groups_polish(*small, 2))


def test_the_empty_call_and_segments_without_pairs(ctx):
    empty = ctx.planes_polish_groups([], [], [], [], [], [], tables=True)
    assert empty["gseq"] == [] and empty["gqual"] == [] and empty["gpolish"] == [] and empty["gcols"].shape == (0,) and empty["gseg_off"].tolist() == [0]
    frames = [b"ACGTN", b"", b"GG", b"TTT"]
    got = ctx.planes_polish_groups(frames, [], [], [3, 2, 0, 1], [], [], tables=True)
    assert got["gseq"] == [[frames[0]] * 3, [b""] * 2, [], [b"TTT"]] and got["gqual"] == [[b"!!!!!"] * 3, [b""] * 2, [], [b"!!!"]]
    assert not got["gcols"].tobytes().strip(b"\0") and len(got["gcols"]) == 3 * 6 + 2 * 1 + 4
    ic.same_groups(got, ic.host_groups_polish(frames, [], [], [3, 2, 0, 1], [], [], 3))
    none = ctx.planes_polish_groups(frames[:2], [], [], [0, 0], [], [], tables=True)   # segments, and not one group
    assert none["gseq"] == [[], []] and none["gcols"].shape == (0,)


def test_refusals_write_nothing(ctx):
    L = _lib.load()
    frames = [b"ACGT", b"GATTACA"]
    sop, group, ng = np.array([0, 1, 1], np.int32), np.array([0, 2, -1], np.int32), np.array([1, 3], np.int32)
    rlen, f_off = np.array([4, 7], np.int32), np.array([0, 4], np.int64)
    P = 5 + 8 + 8
    base, slots = np.zeros(P, np.uint8), np.zeros(pp.SLOTS * P, np.uint8)
    bound = api.pileup_call_bound(4) + 3 * api.pileup_call_bound(7)
    rows = 5 + 3 * 8
    seq, qual = np.full(bound, 0xA5, np.uint8), np.full(bound, 0xA5, np.uint8)
    off, pol = np.full(5, -9, np.int64), np.full(4 * 8, -9, np.int32)
    gcols, gins = np.full(rows * 8, 0xA5A5A5A5, np.uint32), np.full(rows * 32, 0xA5A5A5A5, np.uint32)
    p32, p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)), lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    d = lambda a: a.ctypes.data

    def call(ns=2, np_=3, rlen_=rlen, frames_=b"".join(frames), f_off_=f_off, ng_=ng, sop_=sop, group_=group, base_=d(base), slots_=d(slots), md=3, seq_=d(seq),
             qual_=d(qual), cap=bound, off_=off):
        arr = lambda a: None if a is None else np.asarray(a, np.int32)   # (alive until the call returns)
        s_arr, g_arr, n_arr = arr(sop_), arr(group_), arr(ng_)
        ptr = lambda a: p32(a) if a is not None else None
        return L.ioc_planes_polish_groups(ctx.h, ns, ptr(rlen_), frames_, p64(f_off_) if f_off_ is not None else None, ptr(n_arr), np_, ptr(s_arr), ptr(g_arr),
                                          base_, slots_, md, seq_, qual_, cap, p64(off_) if off_ is not None else None, d(pol), d(gcols), d(gins))

    # what ioc_planes_polish refuses
    assert call(md=0) == -1 and call(ns=-1) == -1 and call(np_=-1) == -1 and call(cap=-1) == -1
    assert call(sop_=[0, 2, 1]) == -1 and call(sop_=[-1, 1, 1]) == -1
    assert call(rlen_=np.array([4, -1], np.int32)) == -1 and call(f_off_=np.array([0, -4], np.int64)) == -1
    assert call(rlen_=None) == -1 and call(f_off_=None) == -1 and call(frames_=None) == -1 and call(sop_=None) == -1 and call(group_=None) == -1
    assert call(base_=None) == -1 and call(slots_=None) == -1 and call(off_=None) == -1 and call(seq_=None) == -1 and call(qual_=None) == -1
    # the groups: a negative count, a group outside -1 .. n_groups - 1, more than 2^31 - 1 group-segments, no counts at all
    assert call(ng_=[1, -1]) == -1 and call(ng_=[-3, 3]) == -1 and call(ng_=None) == -1
    assert call(group_=[1, 2, -1]) == -1 and call(group_=[0, 3, -1]) == -1 and call(group_=[0, 2, -2]) == -1 and call(group_=[0, 2, 255]) == -1
    assert call(ng_=[0, 3]) == -1                                  # (pair 0 is in group 0 of a segment without groups)
    assert call(ng_=[2**31 - 1, 3], cap=2**62) == -1 and call(ng_=[2**30, 2**30], cap=2**62) == -1
    assert call(cap=bound - 1) == -4
    assert (seq == 0xA5).all() and (qual == 0xA5).all() and (off == -9).all() and (pol == -9).all()
    assert (gcols == 0xA5A5A5A5).all() and (gins == 0xA5A5A5A5).all()
    assert call() == 0 and off[0] == 0 and off[4] == 4 + 3 * 7   # (no insertions in planes of zeros, and A at every covered row)
    assert gcols.view(api.PILEUP_DTYPE)["a"].tolist() == [1] * 5 + [0] * 8 + [0] * 8 + [1] * 8
