"""ioc_alleles_split: the split kernels of ioc_site_split.hip (bit planes by ballot, linkage by popcount, one wave per read for the
votes, the refinement rounds) over uploaded sites and alleles, against the host definition ioc_host_alleles_split segment by
segment — at the sizes where a tile of 64 reads or 64 sites ends, with the pairs of the segments interleaved, with segments
that have no pairs or no sites, with more than 64 segments in a call — and against the hand-worked values and the tiled case of
tests/split_common.py.  Bytes and integers only, no tolerance."""
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import split_common as sp

pytestmark = pytest.mark.gpu

READS = (0, 1, 63, 64, 65, 127, 128, 129, 200)
SITES = (0, 1, 2, 63, 64, 65, 130)


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _segment(rng, nr, ns, planted):
    """(sites, alleles of shape (nr, ns)): a planted two-group matrix with holes and noise, or any bytes."""
    major = rng.integers(0, 6, ns)
    minor = (major + 1 + rng.integers(0, 5, ns)) % 6
    any_byte = np.array(sp.BYTES, np.uint8)[rng.integers(0, len(sp.BYTES), (nr, ns))]
    if not planted:
        return sp.sites_of(minor, major), any_byte
    side = rng.integers(0, 2, nr).astype(bool)
    a = np.where(side[:, None], minor[None, :], major[None, :]).astype(np.uint8)
    a[rng.random((nr, ns)) < 0.2] = 7
    noisy = rng.random((nr, ns)) < 0.1
    a[noisy] = any_byte[noisy]
    return sp.sites_of(minor, major), a


@pytest.fixture(scope="module")
def segments():
    """One segment per (reads, sites) of READS x SITES, half planted and half random, and the host definition's answer for each
    under every rule the tests use: computed once."""
    rng = np.random.default_rng(7)
    segs = [_segment(rng, nr, ns, (x + y) % 2 == 0) for x, nr in enumerate(READS) for y, ns in enumerate(SITES)]
    return segs, {}


def _host(cache, key, sites, a, rule):
    if key not in cache:
        cache[key] = api.alleles_split(sites, a, **rule)
    return cache[key]


def _call(ctx, segs, rule, order_seed=1):
    """The segments in one call, their pairs dealt out in a shuffled order; returns (out, rows): rows[g] = the pairs of segment g
    in the order of its matrix' rows."""
    owner = [g for g, (_, a) in enumerate(segs) for _ in range(a.shape[0])]
    random.Random(order_seed).shuffle(owner)
    seen = [0] * len(segs)
    alleles = []
    for g in owner:
        alleles.append(segs[g][1][seen[g]])
        seen[g] += 1
    out = ctx.alleles_split([s for s, _ in segs], alleles, owner, **rule)
    return out, owner


def _same_as_host(out, g, want):
    mem = out["members"][g]
    return (np.array_equal(out["link"][g], want["link"]) and np.array_equal(out["phase"][g], want["phase"]) and
            np.array_equal(out["group"][mem], want["group"]) and np.array_equal(out["vote"][mem], want["vote"]) and
            out["seg"][g].tobytes() == want["seg"].tobytes())


RULE = dict(min_link=3, min_margin=1, rounds=2)


def test_each_size_alone(ctx, segments):
    segs, cache = segments
    n_split = 0
    for g, (sites, a) in enumerate(segs):
        out, owner = _call(ctx, [(sites, a)], RULE)
        want = _host(cache, (g, 2), sites, a, RULE)
        assert _same_as_host(out, 0, want), (a.shape, out["seg"][0], want["seg"])
        n_split += int(want["seg"]["seed"]) >= 0
    assert n_split > 20


@pytest.mark.parametrize("rounds", [0, 1, 2, 5])
def test_all_sizes_in_one_call(ctx, segments, rounds):
    """63 segments, and two more without pairs: more than 64 in one call, the pairs interleaved."""
    segs, cache = segments
    rule = {**RULE, "rounds": rounds}
    extra = [(segs[20][0], np.zeros((0, len(segs[20][0])), np.uint8)), (sp.sites_of([], []), np.zeros((0, 0), np.uint8))]
    out, owner = _call(ctx, segs + extra, rule)
    assert len(out["seg"]) == 65 and owner != sorted(owner)
    for g, (sites, a) in enumerate(segs + extra):
        want = _host(cache, (g, rounds), sites, a, rule)
        assert _same_as_host(out, g, want), (g, a.shape, out["seg"][g], want["seg"])
    assert [int(x) for x in out["seg"]["seed"][-2:]] == [-1, -1] and [int(x) for x in out["seg"]["n_reads"][-2:]] == [0, 0]


def test_many_small_segments(ctx):
    rng = np.random.default_rng(3)
    segs = [_segment(rng, int(rng.integers(0, 12)), int(rng.integers(0, 9)), True) for _ in range(150)]
    rule = dict(min_link=2, min_margin=1, rounds=2)
    out, _ = _call(ctx, segs, rule)
    for g, (sites, a) in enumerate(segs):
        assert _same_as_host(out, g, api.alleles_split(sites, a, **rule)), g
    assert int((out["seg"]["seed"] >= 0).sum()) > 30


@pytest.mark.parametrize("case", sp.HAND_SPLITS, ids=lambda c: c[0])
def test_hand_cases(ctx, case):
    name, minor, major, alleles, (ml, mm, rounds), link, phase, group, vote, seg = case
    a = np.array(alleles, np.uint8).reshape(len(alleles), len(minor))
    out = ctx.alleles_split([sp.sites_of(minor, major)], list(a), [0] * len(alleles), min_link=ml, min_margin=mm, rounds=rounds)
    got = (out["link"][0].tolist(), out["phase"][0].tolist(), out["group"].tolist(), out["vote"].tolist(),
           tuple(int(out["seg"][0][f]) for f in sp.SEG_FIELDS))
    assert got == (link, phase, group, vote, seg)


@pytest.mark.parametrize("rounds", [0, 1, 2, 3, 8])
def test_tiled_case_needs_its_rounds(ctx, rounds):
    minor, major, alleles, truth = sp.tiled()
    a = np.array(alleles, np.uint8)
    out = ctx.alleles_split([sp.sites_of(minor, major)], list(a), [0] * len(a), rounds=rounds, **sp.TILED_RULE)
    group = out["group"].tolist()
    assert group.count(sp.NONE_GROUP) == sp.TILED_NONE.get(rounds, 0) == int(out["seg"][0]["n_none"])
    assert all(g == t for g, t in zip(group, truth) if g != sp.NONE_GROUP)
    assert _same_as_host(out, 0, api.alleles_split(sp.sites_of(minor, major), a, rounds=rounds, **sp.TILED_RULE))


def test_a_smaller_call_after_a_larger_one():
    """One context of its own: the second call reuses the first one's buffers and must not see what it left there."""
    ctx = api.Context(0)
    rng = np.random.default_rng(19)
    big = [_segment(rng, 200, 130, True), _segment(rng, 129, 65, False)]
    small = [_segment(rng, 70, 3, True), _segment(rng, 5, 66, True)]
    for segs in (big, small, big):
        out, _ = _call(ctx, segs, RULE)
        for g, (sites, a) in enumerate(segs):
            assert _same_as_host(out, g, api.alleles_split(sites, a, **RULE)), g
    alone = api.Context(0)
    fresh, _ = _call(alone, small, RULE)
    again, _ = _call(ctx, small, RULE)
    assert all(np.array_equal(fresh[f], again[f]) for f in ("group", "vote")) and fresh["seg"].tobytes() == again["seg"].tobytes()


def test_refusals_write_nothing(ctx):
    L = _lib.load()
    rng = np.random.default_rng(23)
    sites, a = _segment(rng, 6, 4, True)
    sop, s_off, a_off = np.zeros(6, np.int32), np.array([0, 4], np.int64), np.arange(7, dtype=np.int64) * 4
    link, phase = np.full(4, -9, np.int64), np.full(4, -9, np.int8)
    group, vote, seg = np.full(6, 0xA5, np.uint8), np.full(6, -9, np.int32), np.full(8, -9, np.int32)
    p32 = lambda x: x.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32))
    p64 = lambda x: x.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int64))

    def call(ml=1, mm=1, rounds=0, sop_=sop, s_off_=s_off, a_off_=a_off, n_segs=1, n_pairs=6):
        return L.ioc_alleles_split(ctx.h, n_segs, n_pairs, p32(np.ascontiguousarray(sop_, np.int32)), sites.ctypes.data, p64(s_off_), a.ctypes.data,
                                   p64(a_off_), ml, mm, rounds, link.ctypes.data, phase.ctypes.data, group.ctypes.data, vote.ctypes.data, seg.ctypes.data)

    short = a_off.copy()
    short[-1] -= 1   # the last pair's row is 3 bytes long, its segment has 4 sites
    for bad in (dict(ml=0), dict(mm=0), dict(rounds=-1), dict(rounds=65), dict(n_segs=-1), dict(n_pairs=-1), dict(sop_=[0, 0, 0, 0, 0, 1]),
                dict(sop_=[-1, 0, 0, 0, 0, 0]), dict(a_off_=short), dict(s_off_=np.array([1, 4], np.int64)), dict(s_off_=np.array([0, -1], np.int64))):
        assert call(**bad) == -1, bad
    assert (link == -9).all() and (phase == -9).all() and (group == 0xA5).all() and (vote == -9).all() and (seg == -9).all()
    assert call(ml=3, rounds=2) == 0
    want = api.alleles_split(sites, a, 3, 1, 2)
    assert np.array_equal(link, want["link"]) and np.array_equal(group, want["group"]) and seg.tobytes() == want["seg"].tobytes()
    # the empty call
    none = ctx.alleles_split([], [], [])
    assert len(none["seg"]) == 0 and len(none["group"]) == 0
