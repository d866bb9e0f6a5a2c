"""ioc_align_pairs_split: ioc_align_pairs_alleles with the split kernels (ioc_site_split.hip) run where the alleles lie.  Sites,
site offsets, n_found and, where asked for, the alleles and the table must be byte-identical to align_pairs_alleles' for the same
call; the split must equal the host definition ioc_host_alleles_split applied to those sites and alleles, segment by segment.  The
two-haplotype case has its answer in closed form; at 8 % noise the reads must still land on their sides.  Forced down another
route — version 1, re-runs, slices — the output must equal the unforced call's.  Bytes and integers only, no tolerance."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import sites_common as sc
from tests import split_common as sp
from tests.test_gpu_align import _mutate
from tests.test_gpu_align_ops import _route_pairs, _small_pairs
from tests.test_gpu_align_polish import _segments

pytestmark = pytest.mark.gpu

LOOSE = dict(min_depth=1, min_alt=1, min_pct=1)
SPLIT = dict(min_link=3, min_margin=1, rounds=2)


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _split_fields(got):
    return ([x.tolist() for x in got["link"]], [x.tolist() for x in got["phase"]], got["group"].tolist(), got["vote"].tolist(), got["seg"].tobytes())


def _check(ctx, pairs, k, segs, sop, rule=sc.RULE, split=SPLIT, max_sites=4096):
    """The fused call against align_pairs_alleles of the same pairs and the host definition on what that returns."""
    want = ctx.align_pairs_alleles(pairs, k, segs, sop, max_sites=max_sites, tables=True, **rule)
    got = ctx.align_pairs_split(pairs, k, segs, sop, max_sites=max_sites, tables=True, alleles=True, **rule, **split)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got["sites"], want["sites"])) and len(got["sites"]) == len(segs)
    assert np.array_equal(got["n_found"], want["n_found"]) and np.array_equal(got["cols"], want["cols"])
    assert len(got["alleles"]) == len(pairs) and all(np.array_equal(a, b) for a, b in zip(got["alleles"], want["alleles"]))
    for f in ("score", "windows", "ratio"):
        assert np.array_equal(got[f], want[f])
    sop = np.asarray(sop, np.int64)
    for g in range(len(segs)):
        mem = np.flatnonzero(sop == g)
        assert np.array_equal(got["members"][g], mem)
        a = np.array([want["alleles"][i] for i in mem], np.uint8).reshape(len(mem), len(want["sites"][g]))
        host = api.alleles_split(want["sites"][g], a, **split)
        assert np.array_equal(got["link"][g], host["link"]) and np.array_equal(got["phase"][g], host["phase"]), g
        assert np.array_equal(got["group"][mem], host["group"]) and np.array_equal(got["vote"][mem], host["vote"]), g
        assert got["seg"][g].tobytes() == host["seg"].tobytes(), (g, got["seg"][g], host["seg"])
    # without the alleles and the table the same split comes back
    lean = ctx.align_pairs_split(pairs, k, segs, sop.astype(np.int32), max_sites=max_sites, **rule, **split)
    assert "alleles" not in lean and "cols" not in lean and _split_fields(lean) == _split_fields(got)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(lean["sites"], want["sites"]))
    return got


def test_two_haplotypes_closed_form(ctx):
    T, B, reads = sc.haplotypes()
    seqs = [T] + reads
    n = len(reads)
    ctx.align_set_pool(seqs)
    got = _check(ctx, [(1 + i, 0, 0, 0.1) for i in range(n)], 11, [(0, 0)], [0] * n)
    assert [(int(s["row"]), int(s["kind"])) for s in got["sites"][0]] == sc.SITES_ON_T
    assert got["link"][0].tolist() == [44] * 5 and got["phase"][0].tolist() == [1] * 5
    assert got["group"].tolist() == [0] * 6 + [1] * 5 and got["vote"].tolist() == [-5] * 6 + [5] * 5
    assert tuple(int(got["seg"][0][f]) for f in sp.SEG_FIELDS) == (0, 5, 11, 6, 5, 0, 44)


@pytest.mark.parametrize("seed", range(8))
def test_noisy_haplotypes(ctx, seed):
    """20 reads of T and 15 of B at 8 % noise: at most 3 of the 35 may be on the wrong side or on none (a cap on the definition:
    its restatement leaves at most 2 on these seeds); which side is called 1 is the seed site's business."""
    T, reads = sc.noisy_haplotypes(seed)
    seqs = [T] + reads
    n = len(reads)
    ctx.align_set_pool(seqs)
    got = _check(ctx, [(1 + i, 0, 0, 0.2) for i in range(n)], 11, [(0, 0)], [0] * n)
    assert [(int(s["row"]), int(s["kind"])) for s in got["sites"][0]] == sc.SITES_ON_T
    group, truth = got["group"].tolist(), [0] * 20 + [1] * 15
    bad = min(sum(g != t for g, t in zip(group, truth)), sum(g != 1 - t for g, t in zip(group, truth)))
    print("seed", seed, "wrong or unassigned:", bad)
    assert bad <= 3


def _family():
    """Reads of two variants of a few references: segments of some depth whose reads disagree systematically."""
    rng = random.Random(41)
    seqs, pairs, segs, sop = [], [], [], []
    for g, length in enumerate((150, 260, 90)):
        ref = bytes(rng.choice(b"ACGT") for _ in range(length))
        alt = bytearray(ref)
        for p in range(10, length - 10, 23):
            alt[p] = sc.other_base(ref[p])
        first = len(seqs)
        seqs.append(ref)
        segs.append((first, 0))
        for i in range(9):
            seqs.append(_mutate(rng, bytes(alt) if i % 2 else ref, 0.03))
            pairs.append((len(seqs) - 1, first, 0, 0.1))
            sop.append(g)
    order = list(range(len(pairs)))
    rng.shuffle(order)   # the pairs of the segments interleaved
    return seqs, [pairs[i] for i in order], segs, [sop[i] for i in order]


@pytest.mark.parametrize("env", [{}, {"IOC_ALIGN_V1": "1"}, {"IOC_ALIGN_ARENA": "fat"}, {"IOC_ALIGN_CORRIDOR": "0"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()) or "unforced")
def test_every_route(ctx, monkeypatch, env):
    seqs, pairs, segs, sop = _family()
    ctx.align_set_pool(seqs)
    unforced = ctx.align_pairs_split(pairs, 11, segs, sop, **SPLIT)
    assert all(int(s["seed"]) >= 0 and int(s["n_group0"]) >= 3 and int(s["n_group1"]) >= 3 for s in unforced["seg"])
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    got = _check(ctx, pairs, 11, segs, sop)
    assert _split_fields(got) == _split_fields(unforced)
    if env and "IOC_ALIGN_CORRIDOR" not in env:
        assert ctx.timings()["align_version"] == 1


def test_routes_of_the_alleles_tests(ctx):
    """_route_pairs(), the pairs test_gpu_align_alleles.py sends down every route, under loose thresholds: many sites, little
    linkage — whatever comes out is the definition's."""
    seqs, pairs = _route_pairs()
    segs, sop = _segments(pairs)
    ctx.align_set_pool(seqs)
    _check(ctx, pairs, 11, segs, sop, rule=LOOSE, split=dict(min_link=1, min_margin=1, rounds=1))


def test_bound_above_the_budget_runs_in_slices(ctx, monkeypatch):
    """96 pairs of 3 kb on 12 segments under a budget of 1 MB: the call runs in slices, and the output equals the unsliced one's."""
    rng = random.Random(23)
    base = bytes(rng.choice(b"ACGT") for _ in range(3000))
    seqs = [_mutate(rng, base, 0.1) for _ in range(12)]
    pairs = [(i, (i + 1) % 12, i % 2, 0.2) for i in range(12)] * 4 + [((i + 5) % 12, (i + 1) % 12, i % 2, 0.2) for i in range(12)] * 4
    segs, sop = _segments(pairs)
    ctx.align_set_pool(seqs)
    ref = ctx.align_pairs_split(pairs, 11, segs, sop, **SPLIT)
    monkeypatch.setenv("IOC_ALIGN_CK_BUDGET_MB", "1")
    got = _check(ctx, pairs, 11, segs, sop)
    assert ctx.timings()["align_slices"] > 1
    assert _split_fields(got) == _split_fields(ref)


def test_a_segment_without_pairs_and_the_empty_call(ctx):
    rng = random.Random(31)
    seqs = [bytes(rng.choice(b"ACGTN") for _ in range(n)) for n in (120, 300, 0, 90)]
    seqs += [_mutate(rng, seqs[1], 0.05) for _ in range(3)]
    ctx.align_set_pool(seqs)
    segs = [(0, 1), (1, 0), (2, 0), (3, 0)]
    got = _check(ctx, [(4, 1, 0, 0.1), (5, 1, 0, 0.1), (6, 1, 0, 0.1)], 11, segs, [1, 1, 1], rule=LOOSE, split=dict(min_link=1, min_margin=1, rounds=1))
    assert [int(x) for x in got["seg"]["n_reads"]] == [0, 3, 0, 0] and [int(x) for x in got["seg"]["seed"][[0, 2, 3]]] == [-1, -1, -1]
    none = ctx.align_pairs_split([], 11, segs, [], tables=True, alleles=True)
    assert [len(s) for s in none["sites"]] == [0] * 4 and none["alleles"] == [] and len(none["group"]) == 0
    assert [tuple(int(s[f]) for f in sp.SEG_FIELDS) for s in none["seg"]] == [(-1, 0, 0, 0, 0, 0, 0)] * 4
    empty = ctx.align_pairs_split([], 11, [], [], tables=True, alleles=True)
    assert empty["sites"] == [] and len(empty["seg"]) == 0 and len(empty["group"]) == 0 and empty["cols"].shape == (0,)


def test_refusals_write_nothing(ctx):
    L = _lib.load()
    seqs, pairs = _small_pairs(29, 30)
    pairs = pairs[:6]
    segs, sop = _segments(pairs)
    ctx.align_set_pool(seqs)
    mx = 16
    good = ctx.align_pairs_split(pairs, 11, segs, sop, max_sites=mx, alleles=True, **LOOSE, **SPLIT)
    per_seg = [api.pileup_sites_bound(len(seqs[r]), mx) for r, _ in segs]
    s_cap, a_cap = sum(per_seg), sum(per_seg[g] for g in sop)
    for bad in (dict(min_depth=0), dict(min_pct=51), dict(max_sites=0), dict(min_link=0), dict(min_margin=0), dict(rounds=-1), dict(rounds=65)):
        with pytest.raises(api.IocError) as e:
            ctx.align_pairs_split(pairs, 11, segs, sop, **{**LOOSE, **SPLIT, **bad})
        assert e.value.code == -1
    arr = ctx._aln_pairs(pairs)
    sarr = (_lib.PolishSeg * len(segs))(*[_lib.PolishSeg(r, rc) for r, rc in segs])
    sites, alle = np.full(s_cap * 8, -9, np.int32), np.full(a_cap, 0xA5, np.uint8)
    s_off, found, a_off = np.full(len(segs) + 1, -9, np.int64), np.full(len(segs), -9, np.int64), np.full(len(pairs) + 1, -9, np.int64)
    score = np.full(len(pairs), -9, np.int32)
    link, phase = np.full(s_cap, -9, np.int64), np.full(s_cap, -9, np.int8)
    group, vote, seg = np.full(len(pairs), 0xA5, np.uint8), np.full(len(pairs), -9, np.int32), np.full(len(segs) * 8, -9, np.int32)
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))

    def call(sop_, md=1, sc_=s_cap, ac=a_cap, ml=3, mm=1, rounds=2, alle_=alle.ctypes.data, group_=group.ctypes.data, seg_=seg.ctypes.data):
        s = np.asarray(sop_, np.int32)
        return L.ioc_align_pairs_split(ctx.h, len(pairs), arr, 11, 2, -2, 1, score.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, len(segs),
                                       sarr, s.ctypes.data_as(C.POINTER(C.c_int32)), md, 1, 1, mx, sites.ctypes.data, sc_, p64(s_off), p64(found),
                                       alle_, ac, p64(a_off), None, ml, mm, rounds, link.ctypes.data, phase.ctypes.data, group_, vote.ctypes.data, seg_)

    other = next(g for g, (r, _) in enumerate(segs) if len(seqs[r]) != len(seqs[segs[sop[0]][0]]))
    assert call([other] + sop[1:]) == -1 and call([len(segs)] + sop[1:]) == -1 and call([-1] + sop[1:]) == -1
    assert call(sop, md=0) == -1 and call(sop, ml=0) == -1 and call(sop, mm=0) == -1 and call(sop, rounds=65) == -1 and call(sop, rounds=-1) == -1
    assert call(sop, group_=None) == -1 and call(sop, seg_=None) == -1
    assert call(sop, sc_=s_cap - 1) == -4 and call(sop, ac=a_cap - 1) == -4
    untouched = lambda: ((sites == -9).all() and (alle == 0xA5).all() and (s_off == -9).all() and (found == -9).all() and (a_off == -9).all() and
                         (score == -9).all() and (link == -9).all() and (phase == -9).all() and (group == 0xA5).all() and (vote == -9).all() and
                         (seg == -9).all())
    assert untouched()
    assert call(sop, alle_=None, ac=0) == 0 and (alle == 0xA5).all()   # the alleles are optional, and their capacity with them
    assert group.tolist() == good["group"].tolist() and vote.tolist() == good["vote"].tolist() and seg.tobytes() == good["seg"].tobytes()
    assert call(sop) == 0
    assert all(np.array_equal(alle[a_off[i]:a_off[i + 1]], good["alleles"][i]) for i in range(len(pairs)))
    rec = sites.view(api.PILE_SITE_DTYPE)
    assert all(rec[s_off[g]:s_off[g + 1]].tobytes() == good["sites"][g].tobytes() for g in range(len(segs)))
    assert all(np.array_equal(link[s_off[g]:s_off[g + 1]], good["link"][g]) for g in range(len(segs)))
