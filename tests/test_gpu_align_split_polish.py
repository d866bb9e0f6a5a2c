"""ioc_align_pairs_split_polish: ioc_align_pairs_split with the consensus of both groups of every segment called from the reads'
planes where they lie (k_ops_project_ins beside k_ops_project, then k_plane_pile and the call kernels behind the split).
Everything the split returns must be byte-identical to align_pairs_split's for the same call; every group-segment must equal the
host definition — ioc_host_planes_pile over the planes of the group's reads, projected from align_pairs_ops' strings, then
ioc_host_pileup_call — and what align_pairs_polish gives over just those pairs.  The two-haplotype case has its answer in closed
form.  Forced down another route — version 1, re-runs, slices — the output must equal the unforced call's.  Bytes and integers
only, no tolerance."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import plane_pile_common as pp
from tests import sites_common as sc
from tests.align_ops_checks import revcomp
from tests.test_gpu_align import _mutate
from tests.test_gpu_align_ops import _small_pairs
from tests.test_gpu_align_polish import _segments
from tests.test_gpu_align_split import SPLIT, _family, _split_fields

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _polish_fields(got):
    return got["gseq"], got["gqual"], got["gpolish"].tobytes(), got["gcols"].tobytes(), got["gins"].tobytes()


def _check(ctx, seqs, pairs, k, segs, sop, rule=sc.RULE, split=SPLIT, md=3, per_group=True):
    """The fused call against align_pairs_split of the same call, the host definition and align_pairs_polish group by group."""
    want = ctx.align_pairs_split(pairs, k, segs, sop, tables=True, alleles=True, **rule, **split)
    got = ctx.align_pairs_split_polish(pairs, k, segs, sop, tables=True, alleles=True, polish_min_depth=md, **rule, **split)
    # (a) everything the split returns
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got["sites"], want["sites"])) and len(got["sites"]) == len(segs)
    assert np.array_equal(got["n_found"], want["n_found"]) and got["cols"].tobytes() == want["cols"].tobytes()
    assert len(got["alleles"]) == len(pairs) and all(np.array_equal(a, b) for a, b in zip(got["alleles"], want["alleles"]))
    for f in ("score", "windows", "ratio"):
        assert np.array_equal(got[f], want[f])
    assert _split_fields(got) == _split_fields(want) and all(np.array_equal(a, b) for a, b in zip(got["members"], want["members"]))
    # (b) every group-segment: the definition from the operation strings of its members ...
    ops = ctx.align_pairs_ops(pairs, k)[3]
    frames = [revcomp(seqs[r]) if rc else seqs[r] for r, rc in segs]
    planes = [pp.planes_of(ops[i], seqs[pairs[i][0]], len(frames[sop[i]])) for i in range(len(pairs))]
    group = got["group"].tolist()
    host = pp.host_group_polish(frames, sop, group, [p[0] for p in planes], [p[1] for p in planes], md)
    pp.same_polish(got, host)
    # ... and align_pairs_polish over just those pairs against the same frame
    for g in range(len(segs) if per_group else 0):
        for h in (0, 1):
            sub = [i for i in range(len(pairs)) if sop[i] == g and group[i] == h]
            one = ctx.align_pairs_polish([pairs[i] for i in sub], k, [segs[g]], [0] * len(sub), min_depth=md)
            assert one["seq"][0] == got["gseq"][g][h] and one["qual"][0] == got["gqual"][g][h], (g, h)
            assert one["polish"][0].tobytes() == got["gpolish"][g, h].tobytes(), (g, h)
    lean = ctx.align_pairs_split_polish(pairs, k, segs, sop, polish_min_depth=md, **rule, **split)
    assert "gcols" not in lean and "alleles" not in lean and _polish_fields(got)[:3] == (lean["gseq"], lean["gqual"], lean["gpolish"].tobytes())
    return got


def test_two_haplotypes_closed_form(ctx):
    """(c) six reads of T and five of B on T: group 0 is called T and group 1 B, unanimously."""
    T, B, reads = sc.haplotypes()
    seqs = [T] + reads
    n = len(reads)
    ctx.align_set_pool(seqs)
    got = _check(ctx, seqs, [(1 + i, 0, 0, 0.1) for i in range(n)], 11, [(0, 0)], [0] * n)
    assert got["group"].tolist() == [0] * 6 + [1] * 5
    assert got["gseq"][0] == [T, B]
    assert got["gqual"][0] == [b"I" * len(T), b"I" * len(B)]
    assert [int(x) for x in got["gpolish"][0]["n_low"]] == [0, 0]
    assert [tuple(int(got["gpolish"][0, h][f]) for f in ("n_sub", "n_del", "n_ins")) for h in (0, 1)] == [(0, 0, 0), (1, 3, 2)]


@pytest.mark.parametrize("env", [{}, {"IOC_ALIGN_V1": "1"}, {"IOC_ALIGN_ARENA": "fat"}, {"IOC_ALIGN_CORRIDOR": "0"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()) or "unforced")
def test_every_route(ctx, monkeypatch, env):
    """(d) _family()'s three segments, their pairs interleaved."""
    seqs, pairs, segs, sop = _family()
    ctx.align_set_pool(seqs)
    unforced = ctx.align_pairs_split_polish(pairs, 11, segs, sop, tables=True, **SPLIT)
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    got = _check(ctx, seqs, pairs, 11, segs, sop)
    assert _split_fields(got) == _split_fields(unforced) and _polish_fields(got) == _polish_fields(unforced)
    if env and "IOC_ALIGN_CORRIDOR" not in env:
        assert ctx.timings()["align_version"] == 1


def test_bound_above_the_budget_runs_in_slices(ctx, monkeypatch):
    """(d) 96 pairs of 3 kb on 12 segments under a budget of 1 MB: the call runs in slices, the eight planes stay on the device
    across them, and the output equals the unsliced call's."""
    rng = random.Random(23)
    base = bytes(rng.choice(b"ACGT") for _ in range(3000))
    seqs = [_mutate(rng, base, 0.1) for _ in range(12)]
    pairs = [(i, (i + 1) % 12, i % 2, 0.2) for i in range(12)] * 4 + [((i + 5) % 12, (i + 1) % 12, i % 2, 0.2) for i in range(12)] * 4
    segs, sop = _segments(pairs)
    ctx.align_set_pool(seqs)
    ref = ctx.align_pairs_split_polish(pairs, 11, segs, sop, tables=True, **SPLIT)
    monkeypatch.setenv("IOC_ALIGN_CK_BUDGET_MB", "1")
    got = _check(ctx, seqs, pairs, 11, segs, sop, per_group=False)
    assert ctx.timings()["align_slices"] > 1
    assert _split_fields(got) == _split_fields(ref) and _polish_fields(got) == _polish_fields(ref)


def _long_insertions():
    """A reference R, six reads equal to it and five that differ by two substitutions, an insertion of 7 bases in front of R[100]
    and one of 70 in front of R[200]; no inserted run can slide (its ends differ from the bases it stands between)."""
    rng = random.Random(71)
    R = bytes(rng.choice(b"ACGT") for _ in range(300))

    def run(n, at):
        body = bytes(rng.choice(b"ACGT") for _ in range(n - 2))
        return bytes([sc.other_base(R[at], R[at - 1])]) + body + bytes([sc.other_base(R[at], R[at - 1])])

    i7, i70 = run(7, 100), run(70, 200)
    V = bytearray(R)
    V[30], V[260] = sc.other_base(R[30]), sc.other_base(R[260])
    V = bytes(V)
    read = V[:100] + i7 + V[100:200] + i70 + V[200:]
    called = V[:100] + i7[:6] + V[100:200] + i70[:6] + V[200:]
    return R, [R] * 6 + [read] * 5, called


def test_insertions_longer_than_the_slots(ctx):
    """(e) the consensus of the group that inserts 7 and 70 bases carries the first six of each, as the polish call has it."""
    R, reads, called = _long_insertions()
    seqs = [R] + reads
    ctx.align_set_pool(seqs)
    got = _check(ctx, seqs, [(1 + i, 0, 0, 0.1) for i in range(len(reads))], 11, [(0, 0)], [0] * len(reads))
    assert got["group"].tolist() == [0] * 6 + [1] * 5
    assert got["gseq"][0] == [R, called] and got["gqual"][0] == [b"I" * len(R), b"I" * len(called)]
    assert int(got["gpolish"][0, 1]["n_ins"]) == 12 and int(got["gpolish"][0, 1]["n_sub"]) == 2
    row = int(got["grow0"][0, 1])
    assert int(got["gcols"]["ins_bases"][row + 200]) == 5 * 6 and int(got["gcols"]["ins_runs"][row + 200]) == 5 and not got["gins"]["longer"].any()


def test_nothing_is_carried_from_one_call_into_the_next(ctx):
    """(f) on one context: the insertions' call, align_pairs_polish, then a call over fewer rows whose reads insert nothing where
    the first one's did — the slot planes are set to 0 per call, the tables are the call's own."""
    R, reads, _ = _long_insertions()
    seqs = [R] + reads
    ctx.align_set_pool(seqs)
    pairs = [(1 + i, 0, 0, 0.1) for i in range(len(reads))]
    first = ctx.align_pairs_split_polish(pairs, 11, [(0, 0)], [0] * len(pairs), tables=True, **SPLIT)
    assert int(first["gpolish"][0, 1]["n_ins"]) == 12
    ctx.align_pairs_polish(pairs, 11, [(0, 0)], [0] * len(pairs))
    T, B, hap = sc.haplotypes()
    hap = hap[:10]   # (six of T, four of B: ten pairs' planes where eleven lay, and B inserts two bases in front of row 200 too)
    seqs = [T] + hap
    ctx.align_set_pool(seqs)
    got = _check(ctx, seqs, [(1 + i, 0, 0, 0.1) for i in range(len(hap))], 11, [(0, 0)], [0] * len(hap))
    assert got["gseq"][0] == [T, B] and len(T) == len(R)
    # ... and the first call again gives what it gave
    ctx.align_set_pool([R] + reads)
    again = ctx.align_pairs_split_polish(pairs, 11, [(0, 0)], [0] * len(pairs), tables=True, **SPLIT)
    assert _polish_fields(again) == _polish_fields(first) and _split_fields(again) == _split_fields(first)


def test_segments_without_pairs_and_the_empty_call(ctx):
    rng = random.Random(31)
    seqs = [bytes(rng.choice(b"ACGTN") for _ in range(n)) for n in (120, 300, 0, 90)]
    seqs += [_mutate(rng, seqs[1], 0.05) for _ in range(3)]
    ctx.align_set_pool(seqs)
    segs = [(0, 1), (1, 0), (2, 0), (3, 0)]
    loose = dict(min_depth=1, min_alt=1, min_pct=1)
    got = _check(ctx, seqs, [(4, 1, 0, 0.1), (5, 1, 0, 0.1), (6, 1, 0, 0.1)], 11, segs, [1, 1, 1], rule=loose, split=dict(min_link=1, min_margin=1, rounds=1), md=1)
    frames = [revcomp(seqs[0]), seqs[1], seqs[2], seqs[3]]
    for g in (0, 2, 3):
        assert got["gseq"][g] == [frames[g]] * 2 and got["gqual"][g] == [b"!" * len(frames[g])] * 2
    none = ctx.align_pairs_split_polish([], 11, segs, [], tables=True)
    assert none["gseq"] == [[f, f] for f in frames] and none["gqual"] == [[b"!" * len(f)] * 2 for f in frames] and not none["gcols"].tobytes().strip(b"\0")
    empty = ctx.align_pairs_split_polish([], 11, [], [], tables=True)
    assert empty["gseq"] == [] and empty["gpolish"].shape == (0, 2) and empty["gcols"].shape == (0,) and len(empty["group"]) == 0


def test_refusals_write_nothing(ctx):
    """(g) the split's refusals and the polish's: every output keeps its sentinel."""
    L = _lib.load()
    seqs, pairs = _small_pairs(29, 30)
    pairs = pairs[:6]
    segs, sop = _segments(pairs)
    ctx.align_set_pool(seqs)
    mx = 16
    loose = dict(min_depth=1, min_alt=1, min_pct=1)
    good = ctx.align_pairs_split_polish(pairs, 11, segs, sop, max_sites=mx, alleles=True, tables=True, polish_min_depth=2, **loose, **SPLIT)
    for bad in (dict(polish_min_depth=0), dict(min_link=0), dict(min_depth=0), dict(cap=0)):
        with pytest.raises(api.IocError) as e:
            ctx.align_pairs_split_polish(pairs, 11, segs, sop, **{**loose, **SPLIT, **bad})
        assert e.value.code == (-4 if "cap" in bad else -1)
    per_seg = [api.pileup_sites_bound(len(seqs[r]), mx) for r, _ in segs]
    s_cap, a_cap = sum(per_seg), sum(per_seg[g] for g in sop)
    bound = 2 * sum(api.pileup_call_bound(len(seqs[r])) for r, _ in segs)
    n_rows = 2 * sum(len(seqs[r]) + 1 for r, _ in segs)
    arr = ctx._aln_pairs(pairs)
    sarr = (_lib.PolishSeg * len(segs))(*[_lib.PolishSeg(r, rc) for r, rc in segs])
    outs = dict(sites=np.full(s_cap * 8, -9, np.int32), alle=np.full(a_cap, 0xA5, np.uint8), s_off=np.full(len(segs) + 1, -9, np.int64),
                found=np.full(len(segs), -9, np.int64), a_off=np.full(len(pairs) + 1, -9, np.int64), score=np.full(len(pairs), -9, np.int32),
                link=np.full(s_cap, -9, np.int64), phase=np.full(s_cap, -9, np.int8), group=np.full(len(pairs), 0xA5, np.uint8),
                vote=np.full(len(pairs), -9, np.int32), seg=np.full(len(segs) * 8, -9, np.int32), seq=np.full(bound, 0xA5, np.uint8),
                qual=np.full(bound, 0xA5, np.uint8), off=np.full(2 * len(segs) + 1, -9, np.int64), pol=np.full(2 * len(segs) * 8, -9, np.int32),
                gcols=np.full(n_rows * 8, -9, np.int32), gins=np.full(n_rows * 32, -9, np.int32))
    sentinel = {k_: v.copy() for k_, v in outs.items()}
    o = outs
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))

    def call(sop_, md=1, ml=3, pmd=2, cap=bound, seq_=o["seq"].ctypes.data, qual_=o["qual"].ctypes.data, off_=p64(o["off"]), sc_=s_cap):
        s = np.asarray(sop_, np.int32)
        return L.ioc_align_pairs_split_polish(ctx.h, len(pairs), arr, 11, 2, -2, 1, o["score"].ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, len(segs),
                                              sarr, s.ctypes.data_as(C.POINTER(C.c_int32)), md, 1, 1, mx, o["sites"].ctypes.data, sc_, p64(o["s_off"]),
                                              p64(o["found"]), o["alle"].ctypes.data, a_cap, p64(o["a_off"]), None, ml, 1, 2, o["link"].ctypes.data,
                                              o["phase"].ctypes.data, o["group"].ctypes.data, o["vote"].ctypes.data, o["seg"].ctypes.data, pmd, seq_, qual_,
                                              cap, off_, o["pol"].ctypes.data, o["gcols"].ctypes.data, o["gins"].ctypes.data)

    assert call([len(segs)] + sop[1:]) == -1 and call([-1] + sop[1:]) == -1 and call(sop, md=0) == -1 and call(sop, ml=0) == -1
    assert call(sop, sc_=s_cap - 1) == -4
    assert call(sop, pmd=0) == -1 and call(sop, pmd=-3) == -1 and call(sop, off_=None) == -1 and call(sop, seq_=None) == -1 and call(sop, qual_=None) == -1
    assert call(sop, cap=-1) == -1 and call(sop, cap=bound - 1) == -4
    assert all(np.array_equal(outs[k_], sentinel[k_]) for k_ in outs)
    assert call(sop) == 0
    assert o["group"].tolist() == good["group"].tolist() and o["seg"].tobytes() == good["seg"].tobytes()
    assert o["gcols"].tobytes() == good["gcols"].tobytes() and o["gins"].tobytes() == good["gins"].tobytes() and o["pol"].tobytes() == good["gpolish"].tobytes()
    assert [o["seq"][o["off"][x]:o["off"][x + 1]].tobytes() for x in range(2 * len(segs))] == [s for both in good["gseq"] for s in both]
