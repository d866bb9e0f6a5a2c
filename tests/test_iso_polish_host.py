"""The consensus of every isoform of a cluster, on the host alone: the plain-Python restatement of the definition
(iso_polish_common.host_groups_polish) against api.planes_pile + api.pileup_call on hand-made planes, the semantics of the grouped
member lists (group_member_lists, ioc_sink_plan.h) through the restatement, and the property case — four isoforms of one 1000-base
transcript at 8 % errors through the host aligner, both host projections, api.planes_blocks and the definition."""
import numpy as np
import pytest

from isonclust2_amd import api
from tests import blocks_common as bc
from tests import iso_polish_common as ic
from tests import plane_pile_common as pp


def _plane(frame, subs=(), dels=(), ins=(), first=0, last=None):
    """one read's planes on `frame`: its bases, with (row, channel) substitutions, deleted rows and (row, [slot bytes]) insertions"""
    rlen = len(frame)
    last = rlen if last is None else last
    base = np.full(rlen + 1, pp.NONE, np.uint8)
    slots = np.zeros((pp.SLOTS, rlen + 1), np.uint8)
    for r in range(first, last):
        base[r] = {65: 0, 67: 1, 71: 2, 84: 3}.get(frame[r], 4)
    for r, ch in subs:
        base[r] = ch
    for r in dels:
        base[r] = pp.DEL
    for r, run in ins:
        slots[:len(run), r] = run
    return base, slots


def _hand_made():
    frames = [b"ACGTACGTAC", b"GGATTACA", b""]
    reads = [
        (0, 0, _plane(frames[0])), (0, 1, _plane(frames[0], dels=range(3, 7))), (1, 0, _plane(frames[1], subs=[(2, 3)])),
        (0, 1, _plane(frames[0], dels=range(3, 7), ins=[(8, [1, 2])])), (0, 0, _plane(frames[0], subs=[(1, 0)])), (1, 2, _plane(frames[1], ins=[(0, [4])])),
        (0, -1, _plane(frames[0], subs=[(0, 3)])), (0, 1, _plane(frames[0], dels=range(3, 7), ins=[(8, [1, 2])])), (0, 0, _plane(frames[0], first=2, last=9)),
        (1, 0, _plane(frames[1], subs=[(2, 3)])), (2, 0, _plane(frames[2])), (1, 0, _plane(frames[1], subs=[(2, 3)])), (0, 1, _plane(frames[0], dels=range(3, 7))),
    ]
    return frames, [r[0] for r in reads], [r[1] for r in reads], [3, 3, 1], [r[2][0] for r in reads], [r[2][1] for r in reads]


@pytest.mark.parametrize("min_depth", [1, 3])
def test_the_restatement_is_the_definition_on_hand_made_planes(min_depth):
    frames, sop, group, ng, base, slots = _hand_made()
    got = ic.host_groups_polish(frames, sop, group, ng, base, slots, min_depth)
    assert got["gseg_off"].tolist() == [0, 3, 6, 7] and got["grow0"].tolist() == [0, 11, 22, 33, 42, 51, 60]
    for g, frame in enumerate(frames):
        for h in range(ng[g]):
            cols, ins = np.zeros(len(frame) + 1, api.PILEUP_DTYPE), np.zeros(len(frame) + 1, api.PILEUP_INS_DTYPE)
            for i in range(len(base)):
                if sop[i] == g and group[i] == h:
                    api.planes_pile(base[i], slots[i], cols=cols, ins=ins)
            s, q, st = api.pileup_call(cols, ins, frame, min_depth)
            assert (got["gseq"][g][h], got["gqual"][g][h]) == (s, q)
            assert all(int(got["gpolish"][g][h][f]) == st[f] for f in api.POLISH_STATS_FIELDS)
            r0 = int(got["grow0"][int(got["gseg_off"][g]) + h])
            assert got["gcols"][r0:r0 + len(frame) + 1].tobytes() == cols.tobytes() and got["gins"][r0:r0 + len(frame) + 1].tobytes() == ins.tobytes()
    if min_depth == 3:
        # group 1 of segment 0 deletes rows 3 .. 6 and inserts AC in front of row 8 (four reads delete, two of them insert: below
        # the majority); group 2 has no reads: the frame at quality '!'; segment 1's group 0 substitutes row 2
        assert got["gseq"][0][1] == b"ACGTAC" and got["gseq"][0][2] == frames[0] and got["gqual"][0][2] == b"!" * 10
        assert got["gseq"][1][0] == b"GGTTTACA" and got["gseq"][1][1] == frames[1] and got["gseq"][2] == [b""]
    else:
        assert got["gseq"][1][2] == b"T" + frames[1]   # one read, min_depth 1: its insertion in front of row 0 is called


def test_two_groups_everywhere_is_the_layout_of_the_split_polish():
    frames, sop, group, _, base, slots = _hand_made()
    two = [h if h in (0, 1) else -1 for h in group]
    got = ic.host_groups_polish(frames, sop, two, [2, 2, 2], base, slots, 2)
    want = pp.host_group_polish(frames, sop, [h if h >= 0 else pp.SPLIT_NONE for h in two], base, slots, 2)
    assert got["gseq"] == want["gseq"] and got["gqual"] == want["gqual"]
    assert np.concatenate(got["gpolish"]).tobytes() == want["gpolish"].tobytes()
    assert got["gcols"].tobytes() == want["gcols"].tobytes() and got["gins"].tobytes() == want["gins"].tobytes()
    assert got["gseg_off"].tolist() == [0, 2, 4, 6]


def test_grouped_member_lists():
    sop = [1, 0, 1, 1, 0, 2, 1, 0, 1, 3]
    group = [2, 0, 0, -1, 1, 0, 2, 0, 5, 0]           # pair 8 names a group its segment does not have; segment 3 has no groups
    gseg_off, gmem_off, gmembers = ic.py_group_member_lists(4, sop, group, [2, 4, 1, 0])
    assert gseg_off == [0, 2, 6, 7, 7]
    lists = [gmembers[gmem_off[x]:gmem_off[x + 1]] for x in range(7)]
    assert lists == [[1, 7], [4], [2], [], [0, 6], [], [5]]          # ascending pairs; -1 in no list; empty groups have empty lists
    assert all(lst == sorted(lst) for lst in lists) and sorted(gmembers) == [0, 1, 2, 4, 5, 6, 7]
    assert ic.py_group_member_lists(0, [], [], []) == ([0], [0], [])
    assert ic.py_group_member_lists(2, [0, 1], [-1, -1], [3, 0]) == ([0, 3, 3], [0, 0, 0, 0], [])


def test_edit_distance():
    assert ic.edit_distance(b"", b"") == 0 and ic.edit_distance(b"ACGT", b"") == 4 and ic.edit_distance(b"", b"AC") == 2
    assert ic.edit_distance(b"kitten", b"sitting") == 3 and ic.edit_distance(b"ACGTACGT", b"ACGACGTT") == 2
    assert ic.edit_distance(b"AAAA", b"AAAATTTT") == 4 and ic.edit_distance(b"GATTACA", b"GATTACA") == 0


@pytest.fixture(scope="module")
def prop():
    return ic.property_distances(ic.SEED)


def test_every_isoform_consensus_is_its_own_isoform(prop):
    got, true, cons, dist, whole = prop
    assert all(bc.property_holds(got, true))
    print("distances", dist, "whole cluster", whole)
    for h in range(4):
        x = ic.TRUE_OF[h]
        assert all(dist[h][x] < dist[h][y] for y in range(4) if y != x), (h, dist[h])
        assert dist[h][x] < whole[x], (h, dist[h][x], whole[x])
    assert ic.strict_holds(dist, whole)
    # pinned as equalities of the host path
    assert tuple(dist[h][ic.TRUE_OF[h]] for h in range(4)) == ic.OWN
    assert tuple(tuple(d) for d in dist) == ic.DIST and tuple(whole) == ic.WHOLE


def test_the_seed_is_the_first_that_meets_the_conditions():
    assert (ic.SEED, ic.SEEDS_TRIED) == (bc.SEED, bc.SEEDS_TRIED)   # seeds 0 and 1 miss a block condition already (blocks_common)
    for seed in range(ic.SEED):
        T, reads, true = bc.property_case(seed)
        assert not all(bc.property_holds(api.planes_blocks(bc.host_base_planes(T, reads)), true))
