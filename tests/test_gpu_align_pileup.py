"""ioc_align_pairs_pileup: the batched GPU aligner piling every alignment onto its reference on the device (k_ops_pileup).  For
every case the table is checked against two sums of ioc_host_ops_pileup over the call's pairs, each placed at the pair's own
row_base — over the HOST aligner's strings, and over the strings ioc_align_pairs_ops returns in the same context — and score /
windows / ratio against a plain ioc_align_pairs.  The cases are the smallest at which the reduction can go wrong (the generators
and switches of tests/test_gpu_align_ops.py and tests/test_gpu_align_stats.py); where a call is forced down another route — a
re-run, slices — its table must equal the unforced call's: every pair adds exactly once.  Integers only, no tolerance."""
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests.align_ops_checks import revcomp
from tests.test_gpu_align import _mutate
from tests.test_gpu_align_ops import _host_ops, _route_pairs, _small_pairs, refuted_pairs
from tests.test_gpu_align_stats import _stored, block_gap_pairs

pytestmark = pytest.mark.gpu

BASES = ("a", "c", "g", "t", "other")
CHANNEL = {ord("A"): "a", ord("C"): "c", ord("G"): "g", ord("T"): "t"}


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _depth(cols):
    return sum(cols[f].astype(np.int64) for f in BASES + ("del",))


def _sum_of(seqs, pairs, strings, row_base, n_rows):
    """ioc_host_ops_pileup of every pair's string, added at the pair's rows."""
    table = np.zeros(n_rows, api.PILEUP_DTYPE)
    for pr, ops, rb in zip(pairs, strings, row_base):
        m = len(seqs[pr[1]])
        api.ops_pileup(ops, seqs[pr[0]], m, cols=table[rb:rb + m + 1])
    return table


def _check(ctx, seqs, pairs, k, row_base, n_rows, plain=None, set_pool=True, stats=False):
    """One pileup call against the host aligner's strings, against the emitting call's strings of the same context and against a
    plain ioc_align_pairs (`plain`: its result, taken here if None).  Returns (score, windows, ratio, cols, [host strings])."""
    if set_pool:
        ctx.align_set_pool(seqs)
    got = ctx.align_pairs_pileup(pairs, k, row_base, n_rows, stats=stats)
    score, win, ratio, cols = got[:4]
    assert cols.dtype == api.PILEUP_DTYPE and cols.shape == (n_rows,)
    _, _, _, dev_ops = ctx.align_pairs_ops(pairs, k)
    if plain is None:
        plain = ctx.align_pairs(pairs, k)
    assert np.array_equal(score, plain[0]) and np.array_equal(win, plain[1]) and np.array_equal(ratio, plain[2])
    host = []
    for i, pr in enumerate(pairs):
        hops, hscore = _host_ops(seqs[pr[0]], seqs[pr[1]], pr[2], pr[3])
        assert score[i] == hscore, (i, pr)
        host.append(hops)
    for what, strings in (("the host aligner's strings", host), ("the emitting call's strings", dev_ops)):
        want = _sum_of(seqs, pairs, strings, row_base, n_rows)
        bad = np.flatnonzero(cols != want)
        assert bad.size == 0, (what, len(bad), int(bad[0]), cols[bad[0]], want[bad[0]])
    if stats:
        assert np.array_equal(got[4], ctx.align_pairs_stats(pairs, k)[3])
    return score, win, ratio, cols, host


def _own_rows(seqs, pairs, rng=None, gap=0, start=3):
    """Rows of its own for every pair, handed out in a shuffled order from an odd start; `gap`: up to that many unused rows
    between two pairs.  Returns (row_base, n_rows, [unused rows])."""
    order = list(range(len(pairs)))
    if rng:
        rng.shuffle(order)
    row_base, at, unused = [0] * len(pairs), start, list(range(start))
    for i in order:
        row_base[i] = at
        at += len(seqs[pairs[i][1]]) + 1
        g = rng.randint(0, gap) if gap else 0
        unused += range(at, at + g)
        at += g
    return row_base, at, unused


def _by_ref(seqs, pairs):
    """One set of rows per reference sequence: (row_base, n_rows)."""
    first, at = {}, 0
    for pr in pairs:
        if pr[1] not in first:
            first[pr[1]] = at
            at += len(seqs[pr[1]]) + 1
    return [first[pr[1]] for pr in pairs], at


def _one_per_row(bases, start, n_rows):
    """The table in which row start + p holds 1 in the channel of bases[p] and everything else is 0."""
    t = np.zeros(n_rows, api.PILEUP_DTYPE)
    for p, b in enumerate(bases):
        t[CHANNEL.get(b, "other")][start + p] = 1
    return t


def test_small_random_pairs(ctx):
    """Lengths 0 .. 200 incl. empty sequences (answered on the host: nothing to add), every gap-open class; rows of its own per
    pair at arbitrary, also odd, row_base, and once more with unused rows in between, which stay zero."""
    seqs, pairs = _small_pairs(13)
    assert any(len(seqs[p[0]]) == 0 or len(seqs[p[1]]) == 0 for p in pairs)
    rng = random.Random(5)
    row_base, n_rows, _ = _own_rows(seqs, pairs, rng)
    assert any(rb % 2 for rb in row_base) and any(rb % 2 == 0 for rb in row_base)
    for k in (1, 11, 32):
        _check(ctx, seqs, pairs, k, row_base, n_rows, stats=(k == 11))
    row_base, n_rows, unused = _own_rows(seqs, pairs, rng, gap=5)
    assert len(unused) > 100
    cols = _check(ctx, seqs, pairs, 11, row_base, n_rows)[3]
    assert not any(cols[f][unused].any() for f in api.PILEUP_FIELDS)


def test_chunk_edge_lengths(ctx):
    """Identical sequences: ONE run of '=' whose length is at and next to the sizes of a step (64), two steps and a chunk (256)."""
    rng = random.Random(7)
    lens = [63, 64, 65, 127, 128, 129, 255, 256, 257]
    seqs, pairs = [], []
    for t, n in enumerate(lens):
        s = bytes(rng.choice(b"ACGT") for _ in range(n))
        seqs += [s, _stored(s, t % 2)]
        pairs.append((2 * t, 2 * t + 1, t % 2, 0.05))
    row_base, n_rows, _ = _own_rows(seqs, pairs, start=1)
    cols = _check(ctx, seqs, pairs, 11, row_base, n_rows)[3]
    for t, n in enumerate(lens):
        assert np.array_equal(cols[row_base[t]:row_base[t] + n + 1], _one_per_row(seqs[2 * t], 0, n + 1)), n


def test_block_gaps_closed_form(ctx):
    """The anchor that does not depend on ioc_host_ops_pileup.  Every alignment of block_gap_pairs() is 520 columns long, has no end
    gap and exactly one gap, the deleted block (tests/test_gpu_align_stats.py establishes that for this seed).  The 480 pairs whose
    QUERY lacks the block all have `base` as their reference in the aligned frame (half of them through ref_revcomp) and are piled
    onto ONE set of 521 rows; the 480 whose reference lacks it get rows of their own."""
    seqs, pairs, what = block_gap_pairs()
    base = seqs[0]
    assert len(pairs) == 960 and sum(1 for w in what if not w[1]) == 480
    row_base, at = [], 521
    for pr, (G, in_query) in zip(pairs, what):
        if in_query:
            row_base.append(at)
            at += len(seqs[pr[1]]) + 1
        else:
            assert len(seqs[pr[1]]) == 520 and (revcomp(seqs[pr[1]]) if pr[2] else seqs[pr[1]]) == base
            row_base.append(0)
    assert sum(1 for i, pr in enumerate(pairs) if row_base[i] == 0 and pr[2]) == 240
    cols = _check(ctx, seqs, pairs, 11, row_base, at)[3]
    pile = cols[:521]
    for p in range(520):
        ch = CHANNEL[base[p]]
        assert int(pile["del"][p]) + int(pile[ch][p]) == 480, p
        assert not any(pile[f][p] for f in BASES if f != ch), p
    assert int(pile["del"].sum()) == 80 * (1 + 63 + 64 + 65 + 130 + 200) == 41840
    assert not pile["ins_runs"].any() and not pile["ins_bases"].any()
    assert not any(pile[f][520] for f in api.PILEUP_FIELDS)
    for i, (G, in_query) in enumerate(what):
        if not in_query:
            continue
        own = cols[row_base[i]:row_base[i] + 520 - G + 1]
        assert np.all(_depth(own)[:-1] == 1) and _depth(own)[-1] == 0 and not own["del"].any(), (i, G)
        at_ins = np.flatnonzero(own["ins_runs"])
        assert len(at_ins) == 1 and own["ins_runs"][at_ins[0]] == 1 and own["ins_bases"][at_ins[0]] == G == own["ins_bases"].sum(), (i, G)


def test_end_gaps(ctx):
    """The four constructed pairs of test_gpu_align_stats.test_end_gaps, their tables written out: rows under 'd' are zero."""
    rng = random.Random(101)
    base = bytes(rng.choice(b"ACGT") for _ in range(520))
    want = [(base[100:300], base, b"d" * 100 + b"=" * 200 + b"d" * 220, _one_per_row(base[100:300], 100, 521)),
            (base, base[100:300], b"i" * 100 + b"=" * 200 + b"i" * 220, _one_per_row(base[100:300], 0, 201)),
            (base[:300], base[200:500], b"i" * 200 + b"=" * 100 + b"d" * 200, _one_per_row(base[200:300], 0, 301)),
            (base[200:500], base[:300], b"d" * 200 + b"=" * 100 + b"i" * 200, _one_per_row(base[200:300], 200, 301))]
    seqs, pairs = [], []
    for t, (q, r, _, _) in enumerate(want):
        seqs += [q, _stored(r, t % 2)]
        pairs.append((2 * t, 2 * t + 1, t % 2, 0.05))
    row_base, n_rows, _ = _own_rows(seqs, pairs, start=0)
    _, _, _, cols, host = _check(ctx, seqs, pairs, 11, row_base, n_rows)
    for t, (_, r, ops, table) in enumerate(want):
        assert host[t] == ops, (t, api.ops_to_cigar(host[t]))
        assert np.array_equal(cols[row_base[t]:row_base[t] + len(r) + 1], table), t


def test_many_reads_on_one_set_of_rows(ctx):
    """Contention: 300 reads at 10 % divergence of one 300-base reference, all adding into the same 301 rows; the same with every
    second pair against the stored reverse complement (one frame: the two tables are equal)."""
    rng = random.Random(17)
    ref = bytes(rng.choice(b"ACGT") for _ in range(300))
    reads = [_mutate(rng, ref, 0.1) for _ in range(300)]
    seqs = [ref, revcomp(ref)] + reads
    fwd = [(2 + i, 0, 0, 0.2) for i in range(300)]
    cols = _check(ctx, seqs, fwd, 11, [0] * 300, 301)[3]
    assert _depth(cols)[:300].min() > 200 and cols["ins_runs"].sum() > 300
    mixed = [(2 + i, i % 2, i % 2, 0.2) for i in range(300)]
    assert np.array_equal(_check(ctx, seqs, mixed, 11, [0] * 300, 301, set_pool=False)[3], cols)


def test_letters_other_than_acgt(ctx):
    """Other letters in query and reference: the pairs take version 1's comparing kernel, and the query's letter goes to `other`."""
    rng = random.Random(3)
    base = bytes(rng.choice(b"ACGT") for _ in range(700))
    def spoil(s, letters, every):
        s = bytearray(s)
        for p in range(rng.randint(0, every), len(s), every):
            s[p] = rng.choice(letters)
        return bytes(s)
    seqs = [spoil(_mutate(rng, base, 0.08), b"NRYacgt", 23), spoil(base, b"NnK", 31), _mutate(rng, base, 0.05), spoil(base[:150], b"N", 7)]
    pairs = [(0, 1, 0, 0.12), (2, 1, 0, 0.12), (0, 2, 0, 0.12), (3, 1, 0, 0.3), (1, 0, 0, 0.12)]
    row_base, n_rows = _by_ref(seqs, pairs)
    cols = _check(ctx, seqs, pairs, 11, row_base, n_rows, stats=True)[3]
    assert cols["other"].sum() > 40 and ctx.timings()["align_version"] == 1


@pytest.mark.parametrize("env", [{"IOC_ALIGN_V1": "1"}, {"IOC_ALIGN_ARENA": "fat"}, {"IOC_ALIGN_CORRIDOR": "0"}, {"IOC_ALIGN_VARIANT": "carry"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_every_route(ctx, monkeypatch, env):
    """Version 1 (forced, fat arena), version 2 on every tile, and IOC_ALIGN_VARIANT=carry, which an emitting call does not honour."""
    seqs, pairs = _route_pairs()
    row_base, n_rows = _by_ref(seqs, pairs)
    ctx.align_set_pool(seqs)
    unforced = ctx.align_pairs_pileup(pairs, 11, row_base, n_rows)[3]
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    cols = _check(ctx, seqs, pairs, 11, row_base, n_rows, set_pool=False, stats=True)[3]
    assert np.array_equal(cols, unforced)
    if "IOC_ALIGN_V1" in env or "IOC_ALIGN_ARENA" in env:
        assert ctx.timings()["align_version"] == 1


def test_v2_refusals_come_back_through_version_1(ctx, monkeypatch):
    """The re-runs through version 1: pairs the 16-bit window refuses, and the whole batch after a wait that "ran out".  The table
    is the unforced call's: the run that answers a pair adds it, once."""
    seqs, pairs = _route_pairs()
    pairs = [p for p in pairs if len(seqs[p[0]]) and len(seqs[p[1]])]
    row_base, n_rows = _by_ref(seqs, pairs)
    ctx.align_set_pool(seqs)
    plain = ctx.align_pairs(pairs, 11)
    unforced = ctx.align_pairs_pileup(pairs, 11, row_base, n_rows)[3]
    monkeypatch.setenv("IOC_ALIGN_V2_GUARD", "40")
    t0 = ctx.timings()["n_align_refused"]
    guarded = ctx.align_pairs_pileup(pairs, 11, row_base, n_rows)[3]
    assert ctx.timings()["n_align_refused"] - t0 >= 5, "the guard did not refuse the pairs: the case no longer does what it claims"
    assert np.array_equal(guarded, unforced)
    _check(ctx, seqs, pairs, 11, row_base, n_rows, plain=plain, set_pool=False, stats=True)
    monkeypatch.delenv("IOC_ALIGN_V2_GUARD")
    monkeypatch.setenv("IOC_ALIGN_V2_FAKE_TIMEOUT", "1")
    t1 = ctx.timings()["n_align_refused"]
    timed_out = ctx.align_pairs_pileup(pairs, 11, row_base, n_rows)[3]
    assert ctx.timings()["n_align_refused"] - t1 == len(pairs) and ctx.timings()["align_version"] == 1
    assert np.array_equal(timed_out, unforced)
    _check(ctx, seqs, pairs, 11, row_base, n_rows, plain=plain, set_pool=False)


def test_pair_the_corridor_cannot_vouch_for(ctx, monkeypatch, capfd):
    """Pairs that come back from version 2 without an answer and are run again on every tile: the re-run adds them."""
    seqs, pairs = refuted_pairs()
    row_base, n_rows = _by_ref(seqs, pairs)
    ctx.align_set_pool(seqs)
    plain = ctx.align_pairs(pairs, 11)
    unforced = ctx.align_pairs_pileup(pairs, 11, row_base, n_rows)[3]
    monkeypatch.setenv("IOC_ALIGN_CORRIDOR", "0.15")
    monkeypatch.setenv("IOC_TRACE", "1")
    capfd.readouterr()
    score, _, _, cols = ctx.align_pairs_pileup(pairs, 11, row_base, n_rows)
    err = capfd.readouterr().err
    assert "2 of 3 pairs run again without a corridor" in err, err[-2000:]
    assert "pileup:" in err and "k_ops_pileup" in err and f"{n_rows} rows" in err and "operation bytes:" not in err
    monkeypatch.delenv("IOC_TRACE")
    assert np.array_equal(cols, unforced) and list(score) == [9470, 17022, 9470]
    assert np.array_equal(_check(ctx, seqs, pairs, 11, row_base, n_rows, plain=plain, set_pool=False)[3], unforced)


@pytest.mark.parametrize("arena", ["lean", "fat"])
def test_bound_above_the_budget_runs_in_slices(ctx, monkeypatch, arena):
    """192 pairs of 3 kb, piled by reference (16 on every set of rows), under a budget of 1 MB: the call runs in slices, the table
    stays on the device across them and equals the unsliced call's."""
    rng = random.Random(23)
    base = bytes(rng.choice(b"ACGT") for _ in range(3000))
    seqs = [_mutate(rng, base, 0.1) for _ in range(12)]
    pairs = [(i, (i + 1) % 12, i % 2, 0.2) for i in range(12)] * 16
    row_base, n_rows = _by_ref(seqs, pairs)
    ref = _check(ctx, seqs, pairs, 11, row_base, n_rows)
    monkeypatch.setenv("IOC_ALIGN_CK_BUDGET_MB", "1")
    monkeypatch.setenv("IOC_ALIGN_ARENA", arena)
    score, win, ratio, cols, stats = ctx.align_pairs_pileup(pairs, 11, row_base, n_rows, stats=True)
    tm = ctx.timings()
    assert tm["align_version"] == (2 if arena == "lean" else 1) and tm["align_slices"] > 1
    assert np.array_equal(cols, ref[3]) and np.array_equal(score, ref[0]) and np.array_equal(win, ref[1]) and np.array_equal(ratio, ref[2])
    monkeypatch.delenv("IOC_ALIGN_CK_BUDGET_MB")
    monkeypatch.delenv("IOC_ALIGN_ARENA")
    assert np.array_equal(stats, ctx.align_pairs_stats(pairs, 11)[3])


def test_verdict_threshold_is_not_applied_and_survives(ctx):
    """A verdict threshold set beforehand: the pileup call is exact all the same, and a plain call after it is still in verdict
    mode (and does stop walks early)."""
    rng = random.Random(43)
    base = bytes(rng.choice(b"ACGT") for _ in range(5000))
    other = bytes(rng.choice(b"ACGT") for _ in range(4800))
    seqs = [base, _mutate(rng, base, 0.06), _mutate(rng, base, 0.15), _mutate(rng, base, 0.3), other, _mutate(rng, other, 0.1),
            base[:700] + other[700:3000], base[:40], b"ACGT" * 3, b""]
    n = len(seqs)
    pairs = [(i, j, (i + j) % 2, 0.12) for i in range(n) for j in range(n) if i != j and (i + 2 * j) % 3 == 1]
    row_base, n_rows, _ = _own_rows(seqs, pairs, start=0)
    ctx.align_set_pool(seqs)
    ctx.align_set_verdict_threshold(0.0)
    exact = ctx.align_pairs(pairs, 11)
    try:
        ctx.align_set_verdict_threshold(0.6)
        _check(ctx, seqs, pairs, 11, row_base, n_rows, plain=exact, set_pool=False)
        s1, w1, r1 = ctx.align_pairs(pairs, 11)
        assert np.array_equal(exact[0], s1) and np.array_equal(exact[2] >= 0.6, r1 >= 0.6) and np.all(w1 <= exact[1])
        assert np.count_nonzero(w1 < exact[1]) > 0
    finally:
        ctx.align_set_verdict_threshold(0.0)


def test_errors_and_empty_call(ctx):
    seqs, pairs = _small_pairs(29, 30)
    ctx.align_set_pool(seqs)
    m0 = len(seqs[pairs[0][1]])
    with pytest.raises(api.IocError):
        ctx.align_pairs_pileup([(0, len(seqs), 0, 0.1)], 11, [0], 1000)  # a pair outside the pool
    with pytest.raises(api.IocError):
        ctx.align_pairs_pileup(pairs[:1], 11, [-1], 1000)                # a negative row_base
    with pytest.raises(api.IocError):
        ctx.align_pairs_pileup(pairs[:1], 11, [5], 5 + m0)               # one row short
    assert ctx.align_pairs_pileup(pairs[:1], 11, [5], 5 + m0 + 1)[3].shape == (5 + m0 + 1,)
    score, win, ratio, cols = ctx.align_pairs_pileup([], 11, [], 7)
    assert len(score) == len(win) == len(ratio) == 0 and cols.shape == (7,) and cols.dtype == api.PILEUP_DTYPE
    assert not any(cols[f].any() for f in api.PILEUP_FIELDS)
    # the raw call: NULL out_cols / row_base / a negative n_rows are refused, and a refused call writes nothing
    L = _lib.load()
    arr = ctx._aln_pairs(pairs[:3])
    row_base, n_rows, _ = _own_rows(seqs, pairs[:3], start=0)
    rb = np.asarray(row_base, np.int64)
    prb = rb.ctypes.data_as(L.ioc_align_pairs_pileup.argtypes[11])
    out = np.full(n_rows, 0xA5A5A5A5, np.uint32).repeat(8).view(api.PILEUP_DTYPE)
    before = out.copy()
    assert L.ioc_align_pairs_pileup(ctx.h, 3, arr, 11, 2, -2, 1, None, None, None, None, prb, n_rows, None) == -1
    assert L.ioc_align_pairs_pileup(ctx.h, 3, arr, 11, 2, -2, 1, None, None, None, None, None, n_rows, out.ctypes.data) == -1
    assert L.ioc_align_pairs_pileup(ctx.h, 3, arr, 11, 2, -2, 1, None, None, None, None, prb, -1, out.ctypes.data) == -1
    assert L.ioc_align_pairs_pileup(ctx.h, 3, arr, 11, 2, -2, 1, None, None, None, None, prb, n_rows - 1, out.ctypes.data) == -1
    assert np.array_equal(out, before)
    assert L.ioc_align_pairs_pileup(ctx.h, 3, arr, 11, 2, -2, 1, None, None, None, None, prb, n_rows, out.ctypes.data) == 0  # the others may be NULL
    assert np.array_equal(out, ctx.align_pairs_pileup(pairs[:3], 11, row_base, n_rows)[3])
