"""ioc_align_pairs_correct: ioc_align_pairs_polish's alignment and pileup with every pair projected beside it, and k_read_correct
over the tables and the planes where they lie.  Scores, windows, ratio, statistics and both tables must be byte-identical to
align_pairs_polish's for the same call; every pair's corrected bytes and record must equal the host pipeline's — the pair's
planes projected from align_pairs_ops' string (ioc_host_ops_project, ioc_host_ops_project_ins), then ioc_host_read_correct on the
segment's tables.  Forced down another route — version 1, re-runs, slices — the output must equal the unforced call's.  Bytes and
integers only, no tolerance."""
import random

import numpy as np
import pytest

from isonclust2_amd import api, synth
from tests import correct_common as cc
from tests import plane_pile_common as pp
from tests import polish_common as pc
from tests import sites_common as sc
from tests.align_ops_checks import revcomp
from tests.test_gpu_align import _mutate
from tests.test_gpu_align_ops import _small_pairs
from tests.test_gpu_align_polish import _segments
from tests.test_gpu_align_split import _family

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _fields(got):
    return got["seq"], got["qual"], got["correct"].tobytes()


def _check(ctx, seqs, pairs, k, segs, sop, **rule):
    """The fused call against align_pairs_polish of the same call and, pair by pair, the host pipeline."""
    rule = {**cc.DEFAULT, **rule}
    polish = ctx.align_pairs_polish(pairs, k, segs, sop, stats=True, tables=True)
    got = ctx.align_pairs_correct(pairs, k, segs, sop, stats=True, tables=True, **rule)
    for f in ("score", "windows", "ratio"):
        assert np.array_equal(got[f], polish[f]), f
    for f in ("stats", "cols", "ins"):
        assert got[f].tobytes() == polish[f].tobytes(), f
    assert np.array_equal(got["row0"], polish["row0"])
    ops = ctx.align_pairs_ops(pairs, k)[3]
    frames = [revcomp(seqs[r]) if rc else seqs[r] for r, rc in segs]
    planes = [pp.planes_of(ops[i], seqs[pairs[i][0]], len(frames[sop[i]])) for i in range(len(pairs))]
    want = cc.host_correct_planes(frames, got["cols"], got["ins"], sop, [p[0] for p in planes], [p[1] for p in planes], **rule)
    assert got["correct"].tobytes() == want[2].tobytes()
    assert got["seq"] == want[0] and got["qual"] == want[1]
    lean = ctx.align_pairs_correct(pairs, k, segs, sop, **rule)
    assert "cols" not in lean and "stats" not in lean and _fields(lean) == _fields(got)
    return got, ops


def _synth_segment(first):
    """Eight synthetic reads of one 300-base transcript, those of the other strand turned into the first one's: the first is the
    segment's frame, the others are aligned against it.  (sequences, pairs) with pool indices from `first` on."""
    rs = synth.generate(8, 1, 300, 12, 21, seed=3)
    assert {int(x) for x in rs.strand} == {-1, 1}
    seqs = [bytes(rs.read(i)[0]) if rs.strand[i] == rs.strand[0] else revcomp(bytes(rs.read(i)[0])) for i in range(rs.n)]
    return seqs, [(first + i, first, 0, 0.1) for i in range(1, rs.n)]


def test_haplotypes_and_an_isoform(ctx):
    """The property case of test_read_correct_host.py with a few synthetic reads as a second segment, their pairs interleaved with
    the first one's, through the device: against the host pipeline byte by byte, and the property itself on what the device
    returns — the edit distance falls, every B read shows B's alleles at SITES_ON_T, the isoform's reads hold their gap back."""
    T, reads, truths = cc.isoform_case(cc.SEED)
    B = sc.haplotypes()[1]
    n = len(reads)
    more, more_pairs = _synth_segment(1 + n)
    seqs = [T] + reads + more
    ctx.align_set_pool(seqs)
    mine = [(1 + i, 0, 0, 0.1) for i in range(n)]
    pairs = [p for two in zip(mine, more_pairs) for p in two] + mine[len(more_pairs):]
    sop = [int(p[1] != 0) for p in pairs]
    at = [pairs.index(p) for p in mine]   # read i's pair
    got, ops = _check(ctx, seqs, pairs, 11, [(0, 0), (1 + n, 0)], sop)
    out = [got["seq"][x] for x in at]
    before = sum(pc.distance(cc.aligned_part(r, ops[x]), tr) for r, x, tr in zip(reads, at, truths))
    after = sum(pc.distance(s, tr) for s, tr in zip(out, truths))
    print(f"summed edit distance: {before} before, {after} after")
    assert after < before
    assert all(cc.shows_b_alleles(out[i], T, B) for i in range(20, 35)) and not any(cc.shows_b_alleles(out[i], T, B) for i in range(20))
    assert all(int(got["correct"][at[i]]["n_guarded"]) >= cc.CUT[1] - cc.CUT[0] for i in (35, 36))
    assert sum(int(got["correct"][x]["out_len"]) for x in range(len(pairs)) if sop[x] == 1) > 7 * 250   # (the synthetic reads came back)
    wide, _ = _check(ctx, seqs, pairs, 11, [(0, 0), (1 + n, 0)], sop, max_run=64)
    assert all(len(wide["seq"][at[i]]) > len(out[i]) for i in (35, 36))


def test_small_random_pairs_both_frames_and_empty_sequences(ctx):
    """Lengths 0 .. 200 incl. empty queries and empty references, every gap-open class, half against the reverse complement: one
    segment per pair, depth 1 — at min_depth 1 the rule decides, at the default every row is low."""
    seqs, pairs = _small_pairs(13)
    seqs = seqs + [b"", b"ACGTTGCATTGACCA"]
    pairs = pairs + [(len(seqs) - 1, len(seqs) - 2, 0, 0.1), (len(seqs) - 2, len(seqs) - 1, 1, 0.1), (len(seqs) - 2, len(seqs) - 2, 0, 0.1)]
    segs, sop = _segments(pairs)
    assert any(len(seqs[q]) == 0 for q, *_ in pairs) and any(len(seqs[r]) == 0 for _, r, *_ in pairs) and {rc for _, rc in segs} == {0, 1}
    ctx.align_set_pool(seqs)
    got, _ = _check(ctx, seqs, pairs, 11, segs, sop)
    assert int(got["correct"]["n_low"].sum()) > 0
    got, _ = _check(ctx, seqs, pairs, 11, segs, sop, min_depth=1, min_alt=1)
    for i, (q, r, *_) in enumerate(pairs):
        if len(seqs[q]) == 0 or len(seqs[r]) == 0:
            assert got["seq"][i] == b"" and not got["correct"][i].tobytes().strip(b"\0")


def _deep_family():
    """_family()'s three segments with both frames among them: every other segment is aligned against the reverse complement."""
    seqs, pairs, segs, sop = _family()
    flip = {ref for ref, _ in segs[1::2]}
    seqs = [revcomp(s) if i in flip else s for i, s in enumerate(seqs)]
    return seqs, [(q, r, int(r in flip), e) for q, r, _, e in pairs], [(ref, int(ref in flip)) for ref, _ in segs], sop


@pytest.mark.parametrize("env", [{}, {"IOC_ALIGN_V1": "1"}, {"IOC_ALIGN_ARENA": "fat"}, {"IOC_ALIGN_CORRIDOR": "0"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()) or "unforced")
def test_every_route(ctx, monkeypatch, env):
    seqs, pairs, segs, sop = _deep_family()
    ctx.align_set_pool(seqs)
    unforced = ctx.align_pairs_correct(pairs, 11, segs, sop, tables=True)
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    got, _ = _check(ctx, seqs, pairs, 11, segs, sop)
    assert _fields(got) == _fields(unforced) and got["cols"].tobytes() == unforced["cols"].tobytes()
    total = {f: int(got["correct"][f].sum()) for f in cc.FIELDS}
    assert total["n_sub"] > 0 and total["out_len"] > 0
    if env and "IOC_ALIGN_CORRIDOR" not in env:
        assert ctx.timings()["align_version"] == 1


def test_bound_above_the_budget_runs_in_slices(ctx, monkeypatch):
    """96 pairs of 3 kb on 12 segments under a budget of 1 MB: the call runs in slices, the tables and the planes stay on the
    device across them, and the output equals the unsliced call's."""
    rng = random.Random(23)
    base = bytes(rng.choice(b"ACGT") for _ in range(3000))
    seqs = [_mutate(rng, base, 0.1) for _ in range(12)]
    pairs = [(i, (i + 1) % 12, i % 2, 0.2) for i in range(12)] * 4 + [((i + 5) % 12, (i + 1) % 12, i % 2, 0.2) for i in range(12)] * 4
    segs, sop = _segments(pairs)
    ctx.align_set_pool(seqs)
    ref = ctx.align_pairs_correct(pairs, 11, segs, sop, tables=True)
    monkeypatch.setenv("IOC_ALIGN_CK_BUDGET_MB", "1")
    got, _ = _check(ctx, seqs, pairs, 11, segs, sop)
    assert ctx.timings()["align_slices"] > 1
    assert _fields(got) == _fields(ref) and got["ins"].tobytes() == ref["ins"].tobytes()


def test_refusals_and_the_empty_call(ctx):
    ctx.align_set_pool([b"ACGTACGTAC", b"ACGTTCGTAC"])
    empty = ctx.align_pairs_correct([], 11, [], [], tables=True)
    assert empty["seq"] == [] and empty["correct"].shape == (0,) and empty["cols"].shape == (0,) and len(empty["score"]) == 0
    none = ctx.align_pairs_correct([], 11, [(0, 0)], [], tables=True)   # a segment without pairs
    assert none["seq"] == [] and not none["cols"].tobytes().strip(b"\0") and len(none["cols"]) == 11
    pairs = [(1, 0, 0, 0.1)]
    for bad in (dict(min_depth=0), dict(min_alt=0), dict(min_pct=51), dict(max_run=65), dict(max_run=-1)):
        with pytest.raises(api.IocError) as e:
            ctx.align_pairs_correct(pairs, 11, [(0, 0)], [0], **bad)
        assert e.value.code == -1
    with pytest.raises(api.IocError) as e:
        ctx.align_pairs_correct(pairs, 11, [(0, 0)], [0], cap=api.pileup_call_bound(10) - 1)
    assert e.value.code == -4
    with pytest.raises(api.IocError):
        ctx.align_pairs_correct(pairs, 11, [(0, 0)], [1])    # names no segment
    with pytest.raises(api.IocError):
        ctx.align_pairs_correct(pairs, 11, [(2, 0)], [0])    # a segment outside the pool
    got = ctx.align_pairs_correct(pairs, 11, [(0, 0)], [0], min_depth=1, min_alt=1)
    assert got["seq"] == [b"ACGTTCGTAC"] and int(got["correct"][0]["out_len"]) == 10
