"""ioc_align_pairs_stats: the batched GPU aligner reducing every alignment to its statistics on the device (k_ops_stats).  For
every pair of every case the record is checked three ways: it equals ioc_host_ops_stats of the HOST aligner's string field by
field; it equals ioc_host_ops_stats of what ioc_align_pairs_ops returns in the same context; and score / windows / ratio equal a
plain ioc_align_pairs.  The cases are the smallest at which the reduction can go wrong — strings shorter than a chunk and of
length 0, runs of '=' at and next to the chunk sizes, one gap of 1 .. 200 bases at every phase of a chunk, end gaps on either
side — and every route by which a slice's bytes come about (the generators and switches of tests/test_gpu_align_ops.py).
Integers only, no tolerance."""
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests.align_ops_checks import revcomp
from tests.test_align_stats_host import FIELDS
from tests.test_gpu_align import _mutate
from tests.test_gpu_align_ops import _host_ops, _route_pairs, _small_pairs, refuted_pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _rec(stats, i):
    return {f: int(stats[f][i]) for f in FIELDS}


def _check(ctx, seqs, pairs, k, plain=None, set_pool=True):
    """One statistics call against the host aligner's strings, against the emitting call's strings of the same context and against
    a plain ioc_align_pairs (`plain`: its result, taken here if None).  Returns (score, windows, ratio, stats, [host strings])."""
    if set_pool:
        ctx.align_set_pool(seqs)
    score, win, ratio, stats = ctx.align_pairs_stats(pairs, k)
    assert stats.dtype == api.ALN_STATS_DTYPE and stats.shape == (len(pairs),) and not stats["reserved"].any()
    _, _, _, dev_ops = ctx.align_pairs_ops(pairs, k)
    if plain is None:
        plain = ctx.align_pairs(pairs, k)
    assert np.array_equal(score, plain[0]) and np.array_equal(win, plain[1]) and np.array_equal(ratio, plain[2])
    host = []
    for i, pr in enumerate(pairs):
        qi, ri, rc, e = pr[:4]
        tag = (i, len(seqs[qi]), len(seqs[ri]), rc, e)
        hops, hscore = _host_ops(seqs[qi], seqs[ri], rc, e)
        got = _rec(stats, i)
        assert got == api.ops_stats(hops), (tag, "against the host aligner's string", api.ops_to_cigar(hops)[:200])
        assert got == api.ops_stats(dev_ops[i]), (tag, "against the emitting call's string")
        assert score[i] == hscore, tag
        host.append(hops)
    return score, win, ratio, stats, host


def _stored(seq, rc):
    """The pool entry of a reference that is to be aligned as `seq`: its reverse complement when the pair sets ref_revcomp."""
    return revcomp(seq) if rc else seq


def test_small_random_pairs(ctx):
    """Lengths 0 .. 200 incl. empty and one-base sequences: strings shorter than one chunk, strings of length 0 (answered on the
    host: one leading end gap), every gap-open class."""
    seqs, pairs = _small_pairs(13)
    assert any(len(seqs[p[0]]) == 0 or len(seqs[p[1]]) == 0 for p in pairs)
    for k in (1, 11, 32):
        _, _, _, stats, _ = _check(ctx, seqs, pairs, k)
    for i, (qi, ri, _, _) in enumerate(pairs):
        if len(seqs[qi]) == 0 or len(seqs[ri]) == 0:
            assert stats["length"][i] == stats["lead_i"][i] + stats["lead_d"][i] == len(seqs[qi]) + len(seqs[ri]) and stats["columns"][i] == 0


def test_chunk_edge_lengths(ctx):
    """Identical sequences: ONE run of '=' whose length is at and next to the sizes of a step (64), two steps and a chunk (256)."""
    rng = random.Random(7)
    lens = [63, 64, 65, 127, 128, 129, 255, 256, 257]
    seqs, pairs = [], []
    for t, n in enumerate(lens):
        s = bytes(rng.choice(b"ACGT") for _ in range(n))
        seqs += [s, _stored(s, t % 2)]
        pairs.append((2 * t, 2 * t + 1, t % 2, 0.05))
    _, _, _, stats, host = _check(ctx, seqs, pairs, 11)
    for t, n in enumerate(lens):
        assert host[t] == b"=" * n
        assert _rec(stats, t) == {**dict.fromkeys(FIELDS, 0), "length": n, "columns": n, "matches": n}


def block_gap_pairs(e=0.05, seed=101):
    """`base` against `base` without the block [p, p + G), both directions, the block's start at 80 consecutive positions: the
    run of 'I' (of 'D') starts and ends at every phase of a 64-byte step and of a dword whatever the alignment of the pair's
    region in its slice; G >= 130 spans whole steps.  Returns (seqs, pairs, [(G, query has the block)])."""
    rng = random.Random(seed)
    base = bytes(rng.choice(b"ACGT") for _ in range(520))
    seqs, pairs, what = [base, revcomp(base)], [], []
    for G in (1, 63, 64, 65, 130, 200):
        for p in range(120, 200):
            cut = base[:p] + base[p + G:]
            rc = len(pairs) // 2 % 2
            seqs += [cut, revcomp(cut)]
            pairs += [(0, len(seqs) - 2 + rc, rc, e), (len(seqs) - 2, rc, rc, e)]
            what += [(G, True), (G, False)]
    return seqs, pairs, what


def test_block_gaps_at_every_phase(ctx):
    """The anchor that does not depend on ioc_host_ops_stats: each of the 960 alignments is 520 columns long, has no end gap and
    exactly one gap, the deleted block (gap open 3 at e = 0.05; checked with the host aligner on the CPU for this seed)."""
    seqs, pairs, what = block_gap_pairs()
    assert len(pairs) == 960 and sum(p[2] for p in pairs) == 480
    _, _, _, stats, _ = _check(ctx, seqs, pairs, 11)
    for i, (G, in_query) in enumerate(what):
        a, b = ("ins", "del") if in_query else ("del", "ins")
        got = _rec(stats, i)
        assert got["length"] == got["columns"] == 520, (i, G, got)
        assert got["longest_" + a] == G and got[a + "_runs"] == 1 and got[a] == G, (i, G, got)
        assert got[b] == 0 and got[b + "_runs"] == 0 and got["longest_" + b] == 0, (i, G, got)
        assert got["matches"] == 520 - G and got["mismatches"] == 0


def test_block_gaps_with_gap_open_2(ctx):
    """The same pairs at e = 0.2 (gap open 2), where a few alignments are not the single block: against the host only."""
    seqs, pairs, _ = block_gap_pairs(e=0.2)
    _check(ctx, seqs, pairs, 11)


def test_end_gaps(ctx):
    """Free end gaps on either side, long enough to span whole chunks, and unrelated pairs with many short runs."""
    rng = random.Random(101)
    base = bytes(rng.choice(b"ACGT") for _ in range(520))
    u = [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in (300, 310, 300, 310)]
    want = [(base[100:300], base, b"d" * 100 + b"=" * 200 + b"d" * 220),
            (base, base[100:300], b"i" * 100 + b"=" * 200 + b"i" * 220),
            (base[:300], base[200:500], b"i" * 200 + b"=" * 100 + b"d" * 200),
            (base[200:500], base[:300], b"d" * 200 + b"=" * 100 + b"i" * 200),
            (u[0], u[1], None), (u[2], u[3], None)]
    seqs, pairs = [], []
    for t, (q, r, _) in enumerate(want):
        seqs += [q, _stored(r, t % 2)]
        pairs.append((2 * t, 2 * t + 1, t % 2, 0.05 if t < 4 else 0.3))
    _, _, _, stats, host = _check(ctx, seqs, pairs, 11)
    for t, (_, _, ops) in enumerate(want):
        if ops is not None:
            assert host[t] == ops, (t, api.ops_to_cigar(host[t]))
    z = dict.fromkeys(FIELDS, 0)
    assert _rec(stats, 0) == {**z, "length": 520, "columns": 200, "matches": 200, "lead_d": 100, "trail_d": 220}
    assert _rec(stats, 1) == {**z, "length": 520, "columns": 200, "matches": 200, "lead_i": 100, "trail_i": 220}
    assert _rec(stats, 2) == {**z, "length": 500, "columns": 100, "matches": 100, "lead_i": 200, "trail_d": 200}
    assert _rec(stats, 3) == {**z, "length": 500, "columns": 100, "matches": 100, "lead_d": 200, "trail_i": 200}
    for t in (4, 5):
        assert stats["ins_runs"][t] + stats["del_runs"][t] >= 4 and stats["mismatches"][t] > 0


@pytest.mark.parametrize("env", [{"IOC_ALIGN_V1": "1"}, {"IOC_ALIGN_ARENA": "fat"}, {"IOC_ALIGN_CORRIDOR": "0"}, {"IOC_ALIGN_VARIANT": "carry"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_every_route(ctx, monkeypatch, env):
    """Version 1 (forced, fat arena), version 2 on every tile, and IOC_ALIGN_VARIANT=carry, which an emitting call does not honour
    (the plain call beside it does run the carry kernel)."""
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    seqs, pairs = _route_pairs()
    _check(ctx, seqs, pairs, 11)
    if "IOC_ALIGN_V1" in env or "IOC_ALIGN_ARENA" in env:
        assert ctx.timings()["align_version"] == 1


def test_v2_refusals_come_back_through_version_1(ctx, monkeypatch):
    """The re-runs through version 1: pairs the 16-bit window refuses (their records are those of version 1's walk), and the whole
    batch after a wait that "ran out"."""
    seqs, pairs = _route_pairs()
    pairs = [p for p in pairs if len(seqs[p[0]]) and len(seqs[p[1]])]
    ctx.align_set_pool(seqs)
    plain = ctx.align_pairs(pairs, 11)
    monkeypatch.setenv("IOC_ALIGN_V2_GUARD", "40")
    t0 = ctx.timings()["n_align_refused"]
    ctx.align_pairs_stats(pairs, 11)
    assert ctx.timings()["n_align_refused"] - t0 >= 5, "the guard did not refuse the pairs: the case no longer does what it claims"
    _check(ctx, seqs, pairs, 11, plain=plain, set_pool=False)
    monkeypatch.delenv("IOC_ALIGN_V2_GUARD")
    monkeypatch.setenv("IOC_ALIGN_V2_FAKE_TIMEOUT", "1")
    t1 = ctx.timings()["n_align_refused"]
    ctx.align_pairs_stats(pairs, 11)
    assert ctx.timings()["n_align_refused"] - t1 == len(pairs) and ctx.timings()["align_version"] == 1
    _check(ctx, seqs, pairs, 11, plain=plain, set_pool=False)


def test_pair_the_corridor_cannot_vouch_for(ctx, monkeypatch, capfd):
    """Pairs that come back from version 2 without an answer and are run again on every tile: their records are the re-run's."""
    seqs, pairs = refuted_pairs()
    ctx.align_set_pool(seqs)
    plain = ctx.align_pairs(pairs, 11)
    monkeypatch.setenv("IOC_ALIGN_CORRIDOR", "0.15")
    monkeypatch.setenv("IOC_TRACE", "1")
    capfd.readouterr()
    score, _, _, stats = ctx.align_pairs_stats(pairs, 11)
    err = capfd.readouterr().err
    assert "2 of 3 pairs run again without a corridor" in err, err[-2000:]
    assert "alignment statistics:" in err and "k_ops_stats" in err and "operation bytes:" not in err
    monkeypatch.delenv("IOC_TRACE")
    got = _check(ctx, seqs, pairs, 11, plain=plain, set_pool=False)
    assert np.array_equal(got[3], stats) and list(score) == [9470, 17022, 9470]


@pytest.mark.parametrize("arena", ["lean", "fat"])
def test_bound_above_the_budget_runs_in_slices(ctx, monkeypatch, arena):
    """The device bytes count against the checkpoint arena's budget as in ioc_align_pairs_ops: 1.15 MB of them under a budget of
    1 MB run in slices, and the records are those of the unsliced call."""
    rng = random.Random(23)
    base = bytes(rng.choice(b"ACGT") for _ in range(3000))
    seqs = [_mutate(rng, base, 0.1) for _ in range(12)]
    pairs = [(i, (i + 1) % 12, i % 2, 0.2) for i in range(12)] * 16
    ref = _check(ctx, seqs, pairs, 11)
    monkeypatch.setenv("IOC_ALIGN_CK_BUDGET_MB", "1")
    monkeypatch.setenv("IOC_ALIGN_ARENA", arena)
    score, win, ratio, stats = ctx.align_pairs_stats(pairs, 11)
    tm = ctx.timings()
    assert tm["align_version"] == (2 if arena == "lean" else 1) and tm["align_slices"] > 1
    assert np.array_equal(stats, ref[3]) and np.array_equal(score, ref[0]) and np.array_equal(win, ref[1]) and np.array_equal(ratio, ref[2])


def test_verdict_threshold_is_not_applied_and_survives(ctx):
    """A verdict threshold set beforehand: the statistics call is exact all the same, and a plain call after it is still in
    verdict mode (and does stop walks early)."""
    rng = random.Random(43)
    base = bytes(rng.choice(b"ACGT") for _ in range(5000))
    other = bytes(rng.choice(b"ACGT") for _ in range(4800))
    seqs = [base, _mutate(rng, base, 0.06), _mutate(rng, base, 0.15), _mutate(rng, base, 0.3), other, _mutate(rng, other, 0.1),
            base[:700] + other[700:3000], base[:40], b"ACGT" * 3, b""]
    n = len(seqs)
    pairs = [(i, j, (i + j) % 2, 0.12) for i in range(n) for j in range(n) if i != j and (i + 2 * j) % 3 == 1]
    ctx.align_set_pool(seqs)
    ctx.align_set_verdict_threshold(0.0)
    exact = ctx.align_pairs(pairs, 11)
    stopped = 0
    try:
        for thr in (0.2, 0.6):
            ctx.align_set_verdict_threshold(thr)
            _check(ctx, seqs, pairs, 11, plain=exact, set_pool=False)
            s1, w1, r1 = ctx.align_pairs(pairs, 11)
            assert np.array_equal(exact[0], s1) and np.array_equal(exact[2] >= thr, r1 >= thr) and np.all(w1 <= exact[1])
            stopped += int(np.count_nonzero(w1 < exact[1]))
    finally:
        ctx.align_set_verdict_threshold(0.0)
    assert stopped > 0


def test_errors_and_empty_call(ctx):
    seqs, pairs = _small_pairs(29, 30)
    ctx.align_set_pool(seqs)
    with pytest.raises(api.IocError):
        ctx.align_pairs_stats([(0, len(seqs), 0, 0.1)], 11)  # a pair outside the pool
    with pytest.raises(api.IocError):
        ctx.align_pairs_stats([(-1, 0, 0, 0.1)], 11)
    score, win, ratio, stats = ctx.align_pairs_stats([], 11)
    assert len(score) == len(win) == len(ratio) == len(stats) == 0 and stats.dtype == api.ALN_STATS_DTYPE
    L = _lib.load()
    assert L.ioc_align_pairs_stats(ctx.h, 1, ctx._aln_pairs(pairs[:1]), 11, 2, -2, 1, None, None, None, None) == -1  # out_stats NULL
    out = np.zeros(3, api.ALN_STATS_DTYPE)
    assert L.ioc_align_pairs_stats(ctx.h, 3, ctx._aln_pairs(pairs[:3]), 11, 2, -2, 1, None, None, None, out.ctypes.data) == 0  # the others may be
    assert np.array_equal(out, ctx.align_pairs_stats(pairs[:3], 11)[3])
