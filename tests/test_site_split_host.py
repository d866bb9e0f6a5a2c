"""ioc_host_alleles_split, the definition of the split of a cluster's reads by linked sites, against the plain-Python restatement of
tests/split_common.py: cases worked out by hand, random matrices, planted two-group matrices with noise, the tiled case at several
round counts, and the refusals.  Integers and bytes only; no GPU."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import split_common as sp


@pytest.mark.parametrize("case", sp.HAND_SPLITS, ids=lambda c: c[0])
def test_hand_cases(case):
    name, minor, major, alleles, (ml, mm, rounds), link, phase, group, vote, seg = case
    want = (link, phase, group, vote, seg)
    assert sp.py_split(minor, major, alleles, ml, mm, rounds) == want, "the restatement disagrees with the hand-worked values"
    assert sp.host(minor, major, alleles, ml, mm, rounds) == want


def test_random_matrices():
    rng = random.Random(3)
    n_split = 0
    for _ in range(60):
        nr, ns = rng.randrange(0, 40), rng.randrange(0, 12)
        minor, major, alleles = sp.random_case(rng, nr, ns)
        rule = (rng.randrange(1, 5), rng.randrange(1, 4), rng.randrange(0, 4))
        want = sp.py_split(minor, major, alleles, *rule)
        assert sp.host(minor, major, alleles, *rule) == want
        n_split += want[4][0] >= 0
    assert n_split > 20


def test_planted_groups_with_noise():
    rng = random.Random(11)
    for nr, ns in ((35, 5), (70, 9), (130, 20)):
        minor, major, alleles = sp.planted_case(rng, nr, ns)
        for rounds in (0, 2):
            want = sp.py_split(minor, major, alleles, 3, 1, rounds)
            assert sp.host(minor, major, alleles, 3, 1, rounds) == want
            group = want[2]
            # the planted groups come back up to their numbering: the seed's minor side is group 1, whichever that is here
            agree = sum(g == i % 2 for i, g in enumerate(group))
            swapped = sum(g == 1 - i % 2 for i, g in enumerate(group))
            assert max(agree, swapped) >= nr * 8 // 10


@pytest.mark.parametrize("rounds", [0, 1, 2, 3, 8])
def test_tiled_case_needs_its_rounds(rounds):
    minor, major, alleles, truth = sp.tiled()
    assert len(alleles) == 64
    want = sp.py_split(minor, major, alleles, rounds=rounds, **sp.TILED_RULE)
    group = want[2]
    assert group.count(sp.NONE_GROUP) == sp.TILED_NONE.get(rounds, 0)
    assert all(g == t for g, t in zip(group, truth) if g != sp.NONE_GROUP), "a read on the wrong side"
    assert sp.host(minor, major, alleles, rounds=rounds, **sp.TILED_RULE) == want


def test_refusals_leave_the_outputs_untouched():
    L = _lib.load()
    minor, major, alleles = sp.random_case(random.Random(5), 6, 4)
    sites, a = sp.sites_of(minor, major), np.array(alleles, np.uint8)
    link, phase = np.full(4, -9, np.int64), np.full(4, -9, np.int8)
    group, vote, seg = np.full(6, 0xA5, np.uint8), np.full(6, -9, np.int32), np.full(8, -9, np.int32)

    def call(ns=4, nr=6, ml=1, mm=1, rounds=0, sites_=sites.ctypes.data, a_=a.ctypes.data, group_=group.ctypes.data, seg_=seg.ctypes.data):
        return L.ioc_host_alleles_split(sites_, ns, a_, nr, ml, mm, rounds, link.ctypes.data, phase.ctypes.data, group_, vote.ctypes.data, seg_)

    for bad in (dict(ml=0), dict(mm=0), dict(rounds=-1), dict(rounds=65), dict(ns=-1), dict(nr=-1), dict(sites_=None), dict(a_=None), dict(group_=None),
                dict(seg_=None)):
        assert call(**bad) == -1, bad
    assert (link == -9).all() and (phase == -9).all() and (group == 0xA5).all() and (vote == -9).all() and (seg == -9).all()
    assert call(rounds=64) == 0 and (group != 0xA5).any() and (seg != -9).all()
    # link, phase and vote may be NULL
    g2, s2 = np.full(6, 0xA5, np.uint8), np.zeros(1, api.SPLIT_SEG_DTYPE)
    assert L.ioc_host_alleles_split(sites.ctypes.data, 4, a.ctypes.data, 6, 1, 1, 64, None, None, g2.ctypes.data, None, s2.ctypes.data) == 0
    assert np.array_equal(g2, group) and s2.tobytes() == seg.tobytes()
    with pytest.raises(api.IocError) as e:
        api.alleles_split(sites, a, min_link=0)
    assert e.value.code == -1
    assert api.SPLIT_SEG_DTYPE.itemsize == 32 and C.sizeof(_lib.SplitSeg) == 32
