"""ioc_align_pairs_alleles: the batched GPU aligner piling every alignment into the table of counts, projecting every pair into
byte planes of its own (k_ops_project), finding every segment's variable sites where the table lies (k_pile_sites) and gathering
every pair's alleles there (k_site_alleles).  On the generators of the polish tests: the table must equal
ioc_align_pairs_pileup's, the sites ioc_host_pileup_sites of that table, the alleles ioc_host_site_alleles of
ioc_host_ops_project of the strings ioc_align_pairs_ops returns in the same context, and score / windows / ratio / statistics the
plain calls'.  Forced down another route — version 1, re-runs, slices — the output must equal the unforced call's.  Bytes and
integers only, no tolerance; refusals are made on the host."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import sites_common as sc
from tests.align_ops_checks import revcomp
from tests.test_gpu_align import _mutate
from tests.test_gpu_align_ops import _route_pairs, _small_pairs, refuted_pairs
from tests.test_gpu_align_polish import _segments
from tests.test_gpu_align_stats import block_gap_pairs

pytestmark = pytest.mark.gpu

LOOSE = dict(min_depth=1, min_alt=1, min_pct=1)   # two reads that disagree anywhere make a site


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _same(a, b):
    return (all(x.tobytes() == y.tobytes() for x, y in zip(a["sites"], b["sites"])) and np.array_equal(a["n_found"], b["n_found"]) and
            len(a["alleles"]) == len(b["alleles"]) and all(np.array_equal(x, y) for x, y in zip(a["alleles"], b["alleles"])) and
            np.array_equal(a["cols"], b["cols"]) and np.array_equal(a["score"], b["score"]) and np.array_equal(a["windows"], b["windows"]) and
            np.array_equal(a["ratio"], b["ratio"]))


def _check(ctx, seqs, pairs, k, rule=sc.RULE, max_sites=4096, set_pool=True, segs=None, sop=None, stats=False):
    if set_pool:
        ctx.align_set_pool(seqs)
    if segs is None:
        segs, sop = _segments(pairs)
    got = ctx.align_pairs_alleles(pairs, k, segs, sop, max_sites=max_sites, tables=True, stats=stats, **rule)
    row0 = [int(x) for x in got["row0"]]
    n_rows = sum(len(seqs[r]) + 1 for r, _ in segs)
    assert got["cols"].shape == (n_rows,) and len(got["sites"]) == len(segs) and len(got["alleles"]) == len(pairs)
    plain = ctx.align_pairs(pairs, k)
    assert np.array_equal(got["score"], plain[0]) and np.array_equal(got["windows"], plain[1]) and np.array_equal(got["ratio"], plain[2])
    row_base = [row0[g] for g in sop]
    assert np.array_equal(got["cols"], ctx.align_pairs_pileup(pairs, k, row_base, n_rows)[3])
    for g, (ref, _) in enumerate(segs):
        want, n = api.pileup_sites(got["cols"][row0[g]:row0[g] + len(seqs[ref]) + 1], max_sites=max_sites, **rule)
        assert int(got["n_found"][g]) == n and got["sites"][g].tobytes() == want.tobytes(), g
    dev_ops = ctx.align_pairs_ops(pairs, k)[3]
    for i, (pr, ops, g) in enumerate(zip(pairs, dev_ops, sop)):
        base, insf = api.ops_project(ops, seqs[pr[0]], len(seqs[pr[1]]))
        want = api.site_alleles(base, insf, got["sites"][g])
        assert np.array_equal(got["alleles"][i], want), (i, pr, got["alleles"][i].tolist(), want.tolist())
    if stats:
        assert np.array_equal(got["stats"], ctx.align_pairs_stats(pairs, k)[3])
    # without the table and the statistics the same sites and alleles come back
    lean = ctx.align_pairs_alleles(pairs, k, segs, sop, max_sites=max_sites, **rule)
    assert "cols" not in lean and "stats" not in lean and _same({**lean, "cols": got["cols"]}, got)
    return got


def _n_alleles(got):
    return sum(len(a) for a in got["alleles"])


def test_small_random_pairs(ctx):
    """Lengths 0 .. 200 incl. empty sequences, every gap-open class, half against the reverse complement; then every read against
    a few references, so that segments have depth."""
    seqs, pairs = _small_pairs(13)
    _check(ctx, seqs, pairs, 11, rule=LOOSE, stats=True)
    rng = random.Random(5)
    base = bytes(rng.choice(b"ACGT") for _ in range(180))
    seqs = [_mutate(rng, base, 0.12) for _ in range(14)] + [b"", b"ACGTN"]
    pairs = [(q, r, r % 2, 0.2) for r in (0, 1, 15) for q in range(16) if q != r] + [(3, 14, 0, 0.2), (14, 14, 1, 0.2)]
    got = _check(ctx, seqs, pairs, 11, rule=LOOSE, stats=True)
    assert _n_alleles(got) > 500 and any(sc.NONE in a.tolist() for a in got["alleles"]) and any(sc.DEL in a.tolist() for a in got["alleles"])
    assert sum(int((s["kind"] == sc.INS).sum()) for s in got["sites"]) > 3
    strict = _check(ctx, seqs, pairs, 11, set_pool=False)
    assert _n_alleles(strict) < _n_alleles(got)
    cut = _check(ctx, seqs, pairs, 11, rule=LOOSE, max_sites=5, set_pool=False)
    assert [len(s) for s in cut["sites"]][:2] == [5, 5] and (cut["n_found"][:2] > 5).all()


def test_block_gaps(ctx):
    """block_gap_pairs(): gaps of 1 .. 200 bases in one block — runs of 'I' and 'D' at every phase of a step and across steps, and
    480 pairs piled on one set of rows in two frames."""
    seqs, pairs, what = block_gap_pairs()
    got = _check(ctx, seqs, pairs, 11)
    assert _n_alleles(got) > 1000


def test_many_reads_on_one_segment(ctx):
    """300 reads at 10 % divergence of one 300-base reference in one segment, also through the stored reverse complement."""
    rng = random.Random(17)
    ref = bytes(rng.choice(b"ACGT") for _ in range(300))
    reads = [_mutate(rng, ref, 0.1) for _ in range(300)]
    seqs = [ref, revcomp(ref)] + reads
    got = _check(ctx, seqs, [(2 + i, 0, 0, 0.2) for i in range(300)], 11, rule=dict(min_depth=3, min_alt=3, min_pct=2))
    assert len(got["sites"][0]) > 64
    mixed = [(2 + i, i % 2, i % 2, 0.2) for i in range(300)]
    got2 = _check(ctx, seqs, mixed, 11, rule=dict(min_depth=3, min_alt=3, min_pct=2), set_pool=False, segs=[(0, 0)], sop=[0] * 300)
    assert _same(got2, got)


def _company(pairs, family):
    """Every pair within `family` (pool sequences that are alike) gets a second query on its reference: segments of depth 2."""
    more = []
    for q, r, rc, e in pairs:
        if q in family and r in family:
            more.append((next(x for x in family if x not in (q, r)), r, rc, e))
    return pairs + more


@pytest.mark.parametrize("env", [{"IOC_ALIGN_V1": "1"}, {"IOC_ALIGN_ARENA": "fat"}, {"IOC_ALIGN_CORRIDOR": "0"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_every_route(ctx, monkeypatch, env):
    seqs, pairs = _route_pairs()
    pairs = _company(pairs, range(6))
    segs, sop = _segments(pairs)
    ctx.align_set_pool(seqs)
    unforced = ctx.align_pairs_alleles(pairs, 11, segs, sop, tables=True, **LOOSE)
    assert _n_alleles(unforced) > 500
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    assert _same(_check(ctx, seqs, pairs, 11, rule=LOOSE, set_pool=False), unforced)
    if "IOC_ALIGN_V1" in env or "IOC_ALIGN_ARENA" in env:
        assert ctx.timings()["align_version"] == 1


def test_v2_refusals_come_back_through_version_1(ctx, monkeypatch):
    """Pairs the 16-bit window refuses, and the whole batch after a wait that "ran out": the run that answers a pair piles and
    projects it, once."""
    seqs, pairs = _route_pairs()
    pairs = _company([p for p in pairs if len(seqs[p[0]]) and len(seqs[p[1]])], range(6))
    segs, sop = _segments(pairs)
    ctx.align_set_pool(seqs)
    unforced = ctx.align_pairs_alleles(pairs, 11, segs, sop, tables=True, **LOOSE)
    monkeypatch.setenv("IOC_ALIGN_V2_GUARD", "40")
    t0 = ctx.timings()["n_align_refused"]
    guarded = ctx.align_pairs_alleles(pairs, 11, segs, sop, tables=True, **LOOSE)
    assert ctx.timings()["n_align_refused"] - t0 >= 5, "the guard did not refuse the pairs: the case no longer does what it claims"
    assert _same(guarded, unforced)
    monkeypatch.delenv("IOC_ALIGN_V2_GUARD")
    monkeypatch.setenv("IOC_ALIGN_V2_FAKE_TIMEOUT", "1")
    t1 = ctx.timings()["n_align_refused"]
    timed_out = ctx.align_pairs_alleles(pairs, 11, segs, sop, tables=True, **LOOSE)
    assert ctx.timings()["n_align_refused"] - t1 == len(pairs) and ctx.timings()["align_version"] == 1
    assert _same(timed_out, unforced)
    monkeypatch.delenv("IOC_ALIGN_V2_FAKE_TIMEOUT")
    _check(ctx, seqs, pairs, 11, rule=LOOSE, set_pool=False)


def test_pair_the_corridor_cannot_vouch_for(ctx, monkeypatch, capfd):
    """Pairs that come back from version 2 without an answer and are run again: the re-run piles and projects them; and the
    trace line."""
    seqs, pairs = refuted_pairs()
    pairs = pairs + [(2, 1, 0, 0.05), (3, 0, 0, 0.05)]
    segs, sop = _segments(pairs)
    ctx.align_set_pool(seqs)
    unforced = ctx.align_pairs_alleles(pairs, 11, segs, sop, tables=True, **LOOSE)
    assert _n_alleles(unforced) > 0
    monkeypatch.setenv("IOC_ALIGN_CORRIDOR", "0.15")
    monkeypatch.setenv("IOC_TRACE", "1")
    capfd.readouterr()
    got = ctx.align_pairs_alleles(pairs, 11, segs, sop, tables=True, **LOOSE)
    err = capfd.readouterr().err
    assert "pairs run again without a corridor" in err, err[-2000:]
    assert "sites:" in err and "k_ops_pileup" in err and "k_ops_project" in err and "k_pile_sites" in err and "k_site_alleles" in err
    assert "operation bytes:" not in err
    monkeypatch.delenv("IOC_TRACE")
    assert _same(got, unforced)
    _check(ctx, seqs, pairs, 11, rule=LOOSE, set_pool=False)


def test_bound_above_the_budget_runs_in_slices(ctx, monkeypatch):
    """192 pairs of 3 kb on 12 segments under a budget of 1 MB: the call runs in slices, the table and the planes stay on the
    device across them, and the output equals the unsliced call's."""
    rng = random.Random(23)
    base = bytes(rng.choice(b"ACGT") for _ in range(3000))
    seqs = [_mutate(rng, base, 0.1) for _ in range(12)]
    pairs = [(i, (i + 1) % 12, i % 2, 0.2) for i in range(12)] * 8 + [((i + 5) % 12, (i + 1) % 12, i % 2, 0.2) for i in range(12)] * 8
    ref = _check(ctx, seqs, pairs, 11)
    assert _n_alleles(ref) > 1000
    segs, sop = _segments(pairs)
    monkeypatch.setenv("IOC_ALIGN_CK_BUDGET_MB", "1")
    got = ctx.align_pairs_alleles(pairs, 11, segs, sop, tables=True)
    assert ctx.timings()["align_slices"] > 1
    assert _same(got, ref)


def _vectors(got, first):
    a = [x.tolist() for x in got["alleles"]]
    assert a[:first] == [a[0]] * first and a[first:] == [a[first]] * (len(a) - first)
    assert all(x != y for x, y in zip(a[0], a[first])) and len(a[0]) > 0
    return a[0], a[first]


def test_two_haplotypes_closed_form(ctx):
    """tests/test_pile_sites_host.py's anchor on the device: 6 reads of T and 5 of B on frame T (stored forward, stored reverse-
    complemented, and one segment fed through both) and on frame B — exactly the known sites, two allele vectors that differ at
    every site."""
    T, B, reads = sc.haplotypes()
    seqs = [T, revcomp(T), B, revcomp(B)] + reads
    n = len(reads)
    ctx.align_set_pool(seqs)
    results = []
    for pairs, segs in (([(4 + i, 0, 0, 0.1) for i in range(n)], [(0, 0)]), ([(4 + i, 1, 1, 0.1) for i in range(n)], [(1, 1)]),
                        ([(4 + i, i % 2, i % 2, 0.1) for i in range(n)], [(0, 0)])):
        got = _check(ctx, seqs, pairs, 11, set_pool=False, segs=segs, sop=[0] * n)
        assert [(int(s["row"]), int(s["kind"])) for s in got["sites"][0]] == sc.SITES_ON_T and int(got["n_found"][0]) == 5
        first, second = _vectors(got, 6)
        assert second[1:4] == [sc.DEL] * 3 and (first[4], second[4]) == (0, 1)
        results.append(got)
    assert _same(results[1], results[0]) and _same(results[2], results[0])
    for ref, rc in ((2, 0), (3, 1)):
        got = _check(ctx, seqs, [(4 + i, ref, rc, 0.1) for i in range(n)], 11, set_pool=False, segs=[(ref, rc)], sop=[0] * n)
        assert [(int(s["row"]), int(s["kind"])) for s in got["sites"][0]] == sc.SITES_ON_B
        _vectors(got, 6)


def test_short_reads_are_not_covered_outside_their_span(ctx):
    """Reads of the middle of the frame only: at the sites outside them — base sites and the insertion site alike — their allele
    is IOC_ALLELE_NONE, inside them it is not."""
    T, B, reads = sc.haplotypes()
    short = [T[90:170]] * 3 + [B[90:167]] * 3
    seqs = [T] + reads + short
    n = len(seqs) - 1
    got = _check(ctx, seqs, [(1 + i, 0, 0, 0.1) for i in range(n)], 11, segs=[(0, 0)], sop=[0] * n)
    assert [(int(s["row"]), int(s["kind"])) for s in got["sites"][0]] == sc.SITES_ON_T
    for a in got["alleles"][len(reads):]:
        a = a.tolist()
        assert a[0] == sc.NONE and a[4] == sc.NONE and sc.NONE not in a[1:4]
    assert all(sc.NONE not in a.tolist() for a in got["alleles"][:len(reads)])
    assert [a.tolist()[1:4] for a in got["alleles"][-3:]] == [[sc.DEL] * 3] * 3


def test_a_segment_without_pairs_and_the_empty_call(ctx):
    rng = random.Random(31)
    seqs = [bytes(rng.choice(b"ACGTN") for _ in range(n)) for n in (120, 300, 0, 90)]
    seqs += [_mutate(rng, seqs[1], 0.05) for _ in range(3)]
    ctx.align_set_pool(seqs)
    segs = [(0, 1), (1, 0), (2, 0), (3, 0)]
    got = _check(ctx, seqs, [(4, 1, 0, 0.1), (5, 1, 0, 0.1), (6, 1, 0, 0.1)], 11, rule=LOOSE, set_pool=False, segs=segs, sop=[1, 1, 1])
    assert [len(s) for s in got["sites"]] == [0, len(got["sites"][1]), 0, 0] and len(got["sites"][1]) > 0 and list(got["n_found"][[0, 2, 3]]) == [0, 0, 0]
    none = ctx.align_pairs_alleles([], 11, segs, [], tables=True)
    assert [len(s) for s in none["sites"]] == [0] * 4 and none["alleles"] == [] and not none["cols"].view(np.uint32).any()
    empty = ctx.align_pairs_alleles([], 11, [], [], tables=True)
    assert empty["sites"] == [] and empty["alleles"] == [] and empty["cols"].shape == (0,) and len(empty["score"]) == 0


def test_refusals_write_nothing(ctx):
    L = _lib.load()
    seqs, pairs = _small_pairs(29, 30)
    pairs = pairs[:6]
    segs, sop = _segments(pairs)
    ctx.align_set_pool(seqs)
    mx = 16
    good = ctx.align_pairs_alleles(pairs, 11, segs, sop, max_sites=mx, **LOOSE)
    per_seg = [api.pileup_sites_bound(len(seqs[r]), mx) for r, _ in segs]
    s_cap, a_cap = sum(per_seg), sum(per_seg[g] for g in sop)
    for bad in (dict(min_depth=0), dict(min_alt=0), dict(min_pct=0), dict(min_pct=51), dict(max_sites=0)):
        with pytest.raises(api.IocError) as e:
            ctx.align_pairs_alleles(pairs, 11, segs, sop, **{**LOOSE, **bad})
        assert e.value.code == -1
    arr = ctx._aln_pairs(pairs)
    sarr = (_lib.PolishSeg * len(segs))(*[_lib.PolishSeg(r, rc) for r, rc in segs])
    sites, alle = np.full(s_cap * 8, -9, np.int32), np.full(a_cap, 0xA5, np.uint8)
    s_off, found, a_off = np.full(len(segs) + 1, -9, np.int64), np.full(len(segs), -9, np.int64), np.full(len(pairs) + 1, -9, np.int64)
    score = np.full(len(pairs), -9, np.int32)
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    def call(sop_, md=1, mp=1, sc_=s_cap, ac=a_cap, sarr_=sarr):
        s = np.asarray(sop_, np.int32)
        return L.ioc_align_pairs_alleles(ctx.h, len(pairs), arr, 11, 2, -2, 1, score.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, len(segs),
                                         sarr_, s.ctypes.data_as(C.POINTER(C.c_int32)), md, 1, mp, mx, sites.ctypes.data, sc_, p64(s_off), p64(found),
                                         alle.ctypes.data, ac, p64(a_off), None)
    other = next(g for g, (r, _) in enumerate(segs) if len(seqs[r]) != len(seqs[segs[sop[0]][0]]))
    assert call([other] + sop[1:]) == -1                      # a pair whose reference is not as long as its segment's frame
    assert call([len(segs)] + sop[1:]) == -1 and call([-1] + sop[1:]) == -1
    assert call(sop, md=0) == -1 and call(sop, mp=51) == -1
    assert call(sop, sc_=s_cap - 1) == -4 and call(sop, ac=a_cap - 1) == -4
    outside = (_lib.PolishSeg * len(segs))(*[_lib.PolishSeg(len(seqs), 0) for _ in segs])
    assert call(sop, sarr_=outside) == -1
    assert (sites == -9).all() and (alle == 0xA5).all() and (s_off == -9).all() and (found == -9).all() and (a_off == -9).all() and (score == -9).all()
    assert call(sop) == 0
    rec = sites.view(api.PILE_SITE_DTYPE)
    assert all(rec[s_off[g]:s_off[g + 1]].tobytes() == good["sites"][g].tobytes() for g in range(len(segs)))
    assert all(np.array_equal(alle[a_off[i]:a_off[i + 1]], good["alleles"][i]) for i in range(len(pairs)))
