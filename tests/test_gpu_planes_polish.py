"""ioc_planes_polish: k_plane_pile and the call kernels over host planes that are uploaded, against the host definition — the
tables ioc_host_planes_pile adds up from the reads of every group, and ioc_host_pileup_call on them.  One call holds segments of
0, 1, 63, 64, 255, 256, 257 and 600 bases (around the 64 rows of a work item and the 256 of a step of the call kernels) with 0, 1,
3, 65 and 130 reads per group (fewer than the four waves of a workgroup, one more than a multiple of them, two more), the three
group bytes mixed and the segments' pairs interleaved.  Tables, sequences, qualities and records are compared as bytes."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import plane_pile_common as pp

pytestmark = pytest.mark.gpu

# (rlen, reads of group 0, of group 1, of neither)
SHAPES = [(0, 1, 3, 2), (1, 3, 0, 1), (63, 65, 1, 3), (64, 0, 65, 0), (255, 130, 3, 5), (256, 3, 130, 1), (257, 0, 0, 4), (600, 65, 130, 7)]
ALL_NONE = 6


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _case(seed=9):
    """(frames, seg_of_pair, group, base planes, slot planes): every group of every segment has a sequence of its own that most
    of its reads follow — substitutions, deletions, insertions of 1 to 6 bases — and every byte is from the legal sets."""
    rng = random.Random(seed)
    frames, pairs = [], []
    for g, (rlen, n0, n1, nn) in enumerate(SHAPES):
        frame = bytes(rng.choice(b"ACGTN") for _ in range(rlen))
        frames.append(frame)
        for h, count in ((0, n0), (1, n1), (pp.SPLIT_NONE, nn)):
            truth_b = [rng.choice((0, 1, 2, 3, 4, pp.DEL)) if rng.random() < 0.2 else {65: 0, 67: 1, 71: 2, 84: 3}.get(frame[r], 4) for r in range(rlen)]
            truth_i = {r: [rng.randrange(1, 6) for _ in range(rng.randrange(1, 7))] for r in range(rlen + 1) if rng.random() < 0.08}
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
                pairs.append((g, h, base, slots))
    rng.shuffle(pairs)   # the pairs of the segments interleaved, the group bytes mixed
    return frames, [p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs], [p[3] for p in pairs]


@pytest.fixture(scope="module")
def case():
    frames, sop, group, base, slots = _case()
    return frames, sop, group, base, slots, {md: pp.host_group_polish(frames, sop, group, base, slots, md) for md in (1, 3)}


@pytest.mark.parametrize("min_depth", [1, 3])
def test_against_the_definition(ctx, case, min_depth):
    frames, sop, group, base, slots, want = case
    got = ctx.planes_polish(frames, sop, group, base, slots, min_depth=min_depth, tables=True)
    pp.same_polish(got, want[min_depth])
    assert got["grow0"].tolist() == [[2 * sum(len(f) + 1 for f in frames[:g]) + h * (len(frames[g]) + 1) for h in (0, 1)] for g in range(len(frames))]
    # something was called: insertions, substitutions and deletions in the large groups
    big = got["gpolish"][7]
    assert all(int(big[h]["n_ins"]) > 0 and int(big[h]["n_sub"]) > 0 and int(big[h]["n_del"]) > 0 for h in (0, 1))
    # the segment whose reads are all in IOC_SPLIT_NONE, and a group without reads: the frame at quality '!'
    for g, h in ((ALL_NONE, 0), (ALL_NONE, 1), (1, 1), (3, 0)):
        assert got["gseq"][g][h] == frames[g] and got["gqual"][g][h] == b"!" * len(frames[g]) and int(got["gpolish"][g, h]["n_low"]) == len(frames[g])
        rows = slice(int(got["grow0"][g, h]), int(got["grow0"][g, h]) + len(frames[g]) + 1)
        assert not got["gcols"][rows].tobytes().strip(b"\0") and not got["gins"][rows].tobytes().strip(b"\0")
    lean = ctx.planes_polish(frames, sop, group, base, slots, min_depth=min_depth)
    assert "gcols" not in lean
    pp.same_polish(lean, want[min_depth], tables=False)


def test_nothing_is_carried_between_calls(ctx, case):
    """A small call behind the large one on the same context: the tables are the small call's alone."""
    frames, sop, group, base, slots, want = case
    ctx.planes_polish(frames, sop, group, base, slots, tables=True)
    keep = [i for i in range(len(sop)) if sop[i] in (2, 4)][:40]
    remap = {2: 1, 4: 0}
    small = ([frames[4], frames[2]], [remap[sop[i]] for i in keep], [group[i] for i in keep], [base[i] for i in keep], [slots[i] for i in keep])
    pp.same_polish(ctx.planes_polish(*small, min_depth=2, tables=True), pp.host_group_polish(*small, 2))


def test_the_empty_call_and_segments_without_pairs(ctx):
    empty = ctx.planes_polish([], [], [], [], [], tables=True)
    assert empty["gseq"] == [] and empty["gqual"] == [] and empty["gpolish"].shape == (0, 2) and empty["gcols"].shape == (0,)
    frames = [b"ACGTN", b"", b"GG"]
    got = ctx.planes_polish(frames, [], [], [], [], tables=True)
    assert got["gseq"] == [[f, f] for f in frames] and got["gqual"] == [[b"!" * len(f)] * 2 for f in frames]
    assert not got["gcols"].tobytes().strip(b"\0") and len(got["gcols"]) == 2 * (6 + 1 + 3)
    pp.same_polish(got, pp.host_group_polish(frames, [], [], [], [], 3))


def test_refusals_write_nothing(ctx):
    L = _lib.load()
    frames = [b"ACGT", b"GATTACA"]
    sop, group = np.array([0, 1, 1], np.int32), np.array([0, 1, pp.SPLIT_NONE], np.uint8)
    rlen, f_off = np.array([4, 7], np.int32), np.array([0, 4], np.int64)
    P = 5 + 8 + 8
    base, slots = np.zeros(P, np.uint8), np.zeros(pp.SLOTS * P, np.uint8)
    bound = 2 * sum(api.pileup_call_bound(len(f)) for f in frames)
    seq, qual = np.full(bound, 0xA5, np.uint8), np.full(bound, 0xA5, np.uint8)
    off, pol = np.full(5, -9, np.int64), np.full(4 * 8, -9, np.int32)
    gcols, gins = np.full(2 * 13 * 8, 0xA5A5A5A5, np.uint32), np.full(2 * 13 * 32, 0xA5A5A5A5, np.uint32)
    p32, p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)), lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    d = lambda a: a.ctypes.data

    def call(ns=2, np_=3, rlen_=rlen, frames_=b"".join(frames), f_off_=f_off, sop_=sop, group_=group, base_=d(base), slots_=d(slots), md=3, seq_=d(seq),
             qual_=d(qual), cap=bound, off_=off):
        s_arr = None if sop_ is None else np.asarray(sop_, np.int32)   # (alive until the call returns)
        g_arr = None if group_ is None else np.asarray(group_, np.uint8)
        return L.ioc_planes_polish(ctx.h, ns, p32(rlen_) if rlen_ is not None else None, frames_, p64(f_off_) if f_off_ is not None else None, np_,
                                   p32(s_arr) if s_arr is not None else None, d(g_arr) if g_arr is not None else None,
                                   base_, slots_, md, seq_, qual_, cap, p64(off_) if off_ is not None else None, d(pol), d(gcols), d(gins))

    assert call(md=0) == -1 and call(ns=-1) == -1 and call(np_=-1) == -1 and call(cap=-1) == -1
    assert call(sop_=[0, 2, 1]) == -1 and call(sop_=[-1, 1, 1]) == -1
    assert call(group_=[0, 2, 1]) == -1 and call(group_=[0, 1, 254]) == -1
    assert call(rlen_=np.array([4, -1], np.int32)) == -1 and call(f_off_=np.array([0, -4], np.int64)) == -1
    assert call(rlen_=None) == -1 and call(f_off_=None) == -1 and call(frames_=None) == -1 and call(sop_=None) == -1 and call(group_=None) == -1
    assert call(base_=None) == -1 and call(slots_=None) == -1 and call(off_=None) == -1 and call(seq_=None) == -1 and call(qual_=None) == -1
    assert call(cap=bound - 1) == -4
    assert (seq == 0xA5).all() and (qual == 0xA5).all() and (off == -9).all() and (pol == -9).all()
    assert (gcols == 0xA5A5A5A5).all() and (gins == 0xA5A5A5A5).all()
    assert call() == 0 and off[0] == 0 and off[4] == 2 * (4 + 7)   # (no insertions in planes of zeros, and A at every covered row)
    assert gcols.view(api.PILEUP_DTYPE)["a"].tolist() == [1] * 5 + [0] * 5 + [0] * 8 + [1] * 8
