"""ioc_align_pairs_polish_weighted: the batched GPU aligner piling every alignment by count and by base quality on the device (the
weighted variant of k_ops_pileup) and calling every segment by weight there (the weighted mode of ioc_pile_call.hip).  On the
generators of tests/test_gpu_align_polish.py: the table of counts must equal ioc_align_pairs_pileup's, the tables of weights the
sum of ioc_host_ops_pileup_weighted over the strings ioc_align_pairs_ops returns in the same context, the sequences, qualities,
offsets and records ioc_host_pileup_call_weighted of those tables, and score / windows / ratio a plain ioc_align_pairs.  Forced
down another route — version 1, re-runs, slices — the output must equal the unforced call's.  Bytes and integers only, no
tolerance; refusals are made on the host."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import polish_common as pc
from tests import polish_weight_common as pw
from tests.align_ops_checks import revcomp
from tests.test_gpu_align import _mutate
from tests.test_gpu_align_ops import _route_pairs, _small_pairs, refuted_pairs
from tests.test_gpu_align_polish import _segments
from tests.test_gpu_align_stats import block_gap_pairs

pytestmark = pytest.mark.gpu

KEYS = ("cols", "wcols", "wins", "score", "windows", "ratio", "polish")


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _same(a, b):
    return a["seq"] == b["seq"] and a["qual"] == b["qual"] and all(np.array_equal(a[k], b[k]) for k in KEYS)


def _set(ctx, seqs, quals=None, seed=5):
    """The pool and its qualities: random bytes 33 .. 126 unless given."""
    if quals is None:
        quals = pw.random_quals(np.random.default_rng(seed), seqs)
    ctx.align_set_pool(seqs)
    ctx.align_set_pool_qual(quals)
    return quals


def _check(ctx, seqs, quals, pairs, k, min_depth=3, plain=None, segs=None, sop=None, stats=False):
    if segs is None:
        segs, sop = _segments(pairs)
    got = ctx.align_pairs_polish_weighted(pairs, k, segs, sop, min_depth, tables=True, stats=stats)
    row0 = [int(x) for x in got["row0"]]
    n_rows = sum(len(seqs[r]) + 1 for r, _ in segs)
    assert got["cols"].shape == got["wcols"].shape == got["wins"].shape == (n_rows,)
    if plain is None:
        plain = ctx.align_pairs(pairs, k)
    assert np.array_equal(got["score"], plain[0]) and np.array_equal(got["windows"], plain[1]) and np.array_equal(got["ratio"], plain[2])
    row_base = [row0[g] for g in sop]
    assert np.array_equal(got["cols"], ctx.align_pairs_pileup(pairs, k, row_base, n_rows)[3])
    dev_ops = ctx.align_pairs_ops(pairs, k)[3]
    want_c, want_i = np.zeros(n_rows, api.PILEUP_DTYPE), np.zeros(n_rows, api.PILEUP_INS_DTYPE)
    for pr, ops, rb in zip(pairs, dev_ops, row_base):
        m = len(seqs[pr[1]])
        api.ops_pileup_weighted(ops, seqs[pr[0]], quals[pr[0]], m, wcols=want_c[rb:rb + m + 1], wins=want_i[rb:rb + m + 1])
    bad = np.flatnonzero(got["wcols"] != want_c)
    assert bad.size == 0, (len(bad), int(bad[0]), got["wcols"][bad[0]], want_c[bad[0]])
    bad = np.flatnonzero(got["wins"] != want_i)
    assert bad.size == 0, (len(bad), int(bad[0]), got["wins"][bad[0]], want_i[bad[0]])
    for g, (ref, rc) in enumerate(segs):
        frame = revcomp(seqs[ref]) if rc else seqs[ref]
        rows = slice(row0[g], row0[g] + len(frame) + 1)
        want = api.pileup_call_weighted(got["cols"][rows], got["wcols"][rows], got["wins"][rows], frame, min_depth)
        assert (got["seq"][g], got["qual"][g]) == want[:2], g
        assert {f: int(got["polish"][f][g]) for f in api.POLISH_STATS_FIELDS} == want[2], g
    if stats:
        assert np.array_equal(got["stats"], ctx.align_pairs_stats(pairs, k)[3])
    # without the tables the same sequences come back
    lean = ctx.align_pairs_polish_weighted(pairs, k, segs, sop, min_depth)
    assert lean["seq"] == got["seq"] and lean["qual"] == got["qual"] and np.array_equal(lean["polish"], got["polish"]) and "wcols" not in lean
    return got


def test_small_random_pairs(ctx):
    """Lengths 0 .. 200 incl. empty sequences, every gap-open class, half against the reverse complement, at both depths."""
    seqs, pairs = _small_pairs(13)
    quals = _set(ctx, seqs)
    a = _check(ctx, seqs, quals, pairs, 11, min_depth=1, stats=True)
    b = _check(ctx, seqs, quals, pairs, 11, min_depth=3)
    assert a["polish"]["n_sub"].sum() > 0 and a["polish"]["n_ins"].sum() > 0 and a["polish"]["n_del"].sum() > 0
    assert b["polish"]["n_low"].sum() > a["polish"]["n_low"].sum()
    assert a["wcols"]["del"].sum() > a["cols"]["del"].sum() > 0


def test_block_gaps(ctx):
    """block_gap_pairs(): insertions far beyond the six slots (`longer`), long runs of 'D', and 480 pairs piled on one set of
    rows in two frames — the contention case."""
    seqs, pairs, what = block_gap_pairs()
    quals = _set(ctx, seqs, seed=6)
    got = _check(ctx, seqs, quals, pairs, 11)
    assert got["wins"]["longer"].sum() > 1000


def test_letters_other_than_acgt(ctx):
    rng = random.Random(3)
    base = bytes(rng.choice(b"ACGT") for _ in range(700))
    def spoil(s, letters, every):
        s = bytearray(s)
        for p in range(rng.randint(0, every), len(s), every):
            s[p] = rng.choice(letters)
        return bytes(s)
    seqs = [spoil(_mutate(rng, base, 0.08), b"NRYacgt", 23), spoil(base, b"NnK", 31), _mutate(rng, base, 0.05), spoil(base[:150], b"N", 7),
            revcomp(spoil(base, b"NnKy", 29))]
    pairs = [(0, 1, 0, 0.12), (2, 1, 0, 0.12), (0, 2, 0, 0.12), (3, 1, 0, 0.3), (1, 0, 0, 0.12), (0, 4, 1, 0.12), (2, 4, 1, 0.12), (1, 4, 1, 0.12)]
    quals = _set(ctx, seqs, seed=7)
    got = _check(ctx, seqs, quals, pairs, 11, min_depth=1, stats=True)
    assert got["wcols"]["other"].sum() > got["cols"]["other"].sum() > 40


def test_closed_form_the_weights_decide(ctx):
    """The case of tests/test_pile_weight_host.py on the device, in both frames: the weighted call gives T, the majority call on
    the same pool the three reads' sequence."""
    T, edited, reads, quals = pw.closed_form()
    seqs = [T, revcomp(T)] + reads
    _set(ctx, seqs, [b"I" * 300] * 2 + quals)
    for ref, rc in ((0, 0), (1, 1)):
        pairs = [(2 + i, ref, rc, 0.1) for i in range(5)]
        got = ctx.align_pairs_polish_weighted(pairs, 11, [(ref, rc)], [0] * 5, 3)
        assert got["seq"] == [T]
        assert [int(got["polish"][f][0]) for f in ("out_len", "n_sub", "n_del", "n_ins", "n_low")] == [300, 0, 0, 0, 0]
        plain = ctx.align_pairs_polish(pairs, 11, [(ref, rc)], [0] * 5, 3)
        assert plain["seq"] == [edited] and [int(plain["polish"][f][0]) for f in ("n_sub", "n_del", "n_ins")] == [1, 1, 1]


def test_constant_low_qualities_give_the_majority_call(ctx):
    """All qualities '"' (weight 1): seq / qual / polish of align_pairs_polish, wins == ins, the six channels of wcols == cols."""
    seqs, pairs = _small_pairs(13)
    _set(ctx, seqs, [b'"' * len(s) for s in seqs])
    segs, sop = _segments(pairs)
    for md in (1, 3):
        got = ctx.align_pairs_polish_weighted(pairs, 11, segs, sop, md, tables=True)
        plain = ctx.align_pairs_polish(pairs, 11, segs, sop, md, tables=True)
        assert got["seq"] == plain["seq"] and got["qual"] == plain["qual"] and np.array_equal(got["polish"], plain["polish"])
        assert np.array_equal(got["wins"], plain["ins"]) and np.array_equal(got["cols"], plain["cols"])
        assert all(np.array_equal(got["wcols"][f], plain["cols"][f]) for f in pc.COL_FIELDS)
        assert not got["wcols"]["ins_runs"].any() and not got["wcols"]["ins_bases"].any() and plain["cols"]["ins_bases"].any()


@pytest.mark.parametrize("env", [{"IOC_ALIGN_V1": "1"}, {"IOC_ALIGN_ARENA": "fat"}, {"IOC_ALIGN_CORRIDOR": "0"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_every_route(ctx, monkeypatch, env):
    seqs, pairs = _route_pairs()
    segs, sop = _segments(pairs)
    quals = _set(ctx, seqs, seed=8)
    unforced = ctx.align_pairs_polish_weighted(pairs, 11, segs, sop, 1, tables=True)
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    assert _same(_check(ctx, seqs, quals, pairs, 11, min_depth=1), unforced)
    if "IOC_ALIGN_V1" in env or "IOC_ALIGN_ARENA" in env:
        assert ctx.timings()["align_version"] == 1


def test_v2_refusals_come_back_through_version_1(ctx, monkeypatch):
    """Pairs the 16-bit window refuses, and the whole batch after a wait that "ran out": the run that answers a pair adds it to
    all three tables, once."""
    seqs, pairs = _route_pairs()
    pairs = [p for p in pairs if len(seqs[p[0]]) and len(seqs[p[1]])]
    segs, sop = _segments(pairs)
    quals = _set(ctx, seqs, seed=9)
    plain = ctx.align_pairs(pairs, 11)
    unforced = ctx.align_pairs_polish_weighted(pairs, 11, segs, sop, 1, tables=True)
    monkeypatch.setenv("IOC_ALIGN_V2_GUARD", "40")
    t0 = ctx.timings()["n_align_refused"]
    guarded = ctx.align_pairs_polish_weighted(pairs, 11, segs, sop, 1, tables=True)
    assert ctx.timings()["n_align_refused"] - t0 >= 5, "the guard did not refuse the pairs: the case no longer does what it claims"
    assert _same(guarded, unforced)
    monkeypatch.delenv("IOC_ALIGN_V2_GUARD")
    monkeypatch.setenv("IOC_ALIGN_V2_FAKE_TIMEOUT", "1")
    t1 = ctx.timings()["n_align_refused"]
    timed_out = ctx.align_pairs_polish_weighted(pairs, 11, segs, sop, 1, tables=True)
    assert ctx.timings()["n_align_refused"] - t1 == len(pairs) and ctx.timings()["align_version"] == 1
    assert _same(timed_out, unforced)
    monkeypatch.delenv("IOC_ALIGN_V2_FAKE_TIMEOUT")
    _check(ctx, seqs, quals, pairs, 11, min_depth=1, plain=plain)


def test_pair_the_corridor_cannot_vouch_for(ctx, monkeypatch, capfd):
    """Pairs that come back from version 2 without an answer and are run again: the re-run adds them; and the trace line."""
    seqs, pairs = refuted_pairs()
    segs, sop = _segments(pairs)
    quals = _set(ctx, seqs, seed=10)
    unforced = ctx.align_pairs_polish_weighted(pairs, 11, segs, sop, 1, tables=True)
    monkeypatch.setenv("IOC_ALIGN_CORRIDOR", "0.15")
    monkeypatch.setenv("IOC_TRACE", "1")
    capfd.readouterr()
    got = ctx.align_pairs_polish_weighted(pairs, 11, segs, sop, 1, tables=True)
    err = capfd.readouterr().err
    assert "2 of 3 pairs run again without a corridor" in err, err[-2000:]
    assert "polish:" in err and "k_ops_pileup<weighted>" in err and "k_pile_call<weighted>" in err and "operation bytes:" not in err
    monkeypatch.delenv("IOC_TRACE")
    assert _same(got, unforced)
    _check(ctx, seqs, quals, pairs, 11, min_depth=1)


def test_bound_above_the_budget_runs_in_slices(ctx, monkeypatch):
    """192 pairs of 3 kb on 12 segments under a budget of 1 MB: the call runs in slices, all three tables stay on the device
    across them, and the output equals the unsliced call's."""
    rng = random.Random(23)
    base = bytes(rng.choice(b"ACGT") for _ in range(3000))
    seqs = [_mutate(rng, base, 0.1) for _ in range(12)]
    pairs = [(i, (i + 1) % 12, i % 2, 0.2) for i in range(12)] * 16
    quals = _set(ctx, seqs, seed=11)
    ref = _check(ctx, seqs, quals, pairs, 11)
    segs, sop = _segments(pairs)
    monkeypatch.setenv("IOC_ALIGN_CK_BUDGET_MB", "1")
    got = ctx.align_pairs_polish_weighted(pairs, 11, segs, sop, 3, tables=True)
    assert ctx.timings()["align_slices"] > 1
    assert _same(got, ref)


def test_a_segment_without_pairs_and_the_empty_call(ctx):
    rng = random.Random(31)
    seqs = [bytes(rng.choice(b"ACGTN") for _ in range(n)) for n in (120, 300, 0, 90)]
    seqs.append(_mutate(rng, seqs[1], 0.05))
    _set(ctx, seqs, seed=12)
    segs = [(0, 1), (1, 0), (2, 0), (3, 0)]
    got = ctx.align_pairs_polish_weighted([(4, 1, 0, 0.1)] * 3, 11, segs, [1, 1, 1], 3, tables=True)
    assert got["seq"][0] == revcomp(seqs[0]) and got["seq"][2] == b"" and got["seq"][3] == seqs[3]
    assert got["qual"][0] == b"!" * 120 and got["qual"][3] == b"!" * 90 and got["polish"]["n_low"][1] < 30
    none = ctx.align_pairs_polish_weighted([], 11, segs, [], 3)
    assert none["seq"] == [revcomp(seqs[0]), seqs[1], b"", seqs[3]] and none["qual"] == [b"!" * len(s) for s in none["seq"]]
    empty = ctx.align_pairs_polish_weighted([], 11, [], [], 3, tables=True)
    assert empty["seq"] == [] and empty["polish"].shape == (0,) and empty["wcols"].shape == (0,) and len(empty["score"]) == 0


def test_refusals_write_nothing(ctx):
    L = _lib.load()
    seqs, pairs = _small_pairs(29, 30)
    pairs = pairs[:6]
    segs, sop = _segments(pairs)
    quals = pw.random_quals(np.random.default_rng(14), seqs)
    total = sum(len(s) for s in seqs)
    bound = sum(api.pileup_call_bound(len(seqs[r])) for r, _ in segs)
    arr = ctx._aln_pairs(pairs)
    sarr = (_lib.PolishSeg * len(segs))(*[_lib.PolishSeg(r, rc) for r, rc in segs])
    out_s, out_q = np.full(bound, 0xA5, np.uint8), np.full(bound, 0xA5, np.uint8)
    off, rec, score = np.full(len(segs) + 1, -9, np.int64), np.full(len(segs) * 8, -9, np.int32), np.full(len(pairs), -9, np.int32)
    def call(sop_, md=1, cap=bound):
        s = np.asarray(sop_, np.int32)
        return L.ioc_align_pairs_polish_weighted(ctx.h, len(pairs), arr, 11, 2, -2, 1, score.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None,
                                                 len(segs), sarr, s.ctypes.data_as(C.POINTER(C.c_int32)), md, out_s.ctypes.data, out_q.ctypes.data,
                                                 cap, off.ctypes.data_as(C.POINTER(C.c_int64)), rec.ctypes.data, None, None, None)
    ctx.align_set_pool(seqs)
    assert call(sop) == -1                                    # no qualities set
    assert b"qualities" in L.ioc_last_error(ctx.h)
    assert L.ioc_align_set_pool_qual(ctx.h, b"I" * (total + 1), total + 1) == -1 and call(sop) == -1   # wrong n_bytes: still none
    assert L.ioc_align_set_pool_qual(ctx.h, b"I" * total, total - 1) == -1
    ctx.align_set_pool_qual(quals)
    good = ctx.align_pairs_polish_weighted(pairs, 11, segs, sop, 1)
    ctx.align_set_pool(seqs)
    assert call(sop) == -1                                    # dropped by a new align_set_pool
    ctx.align_set_pool_qual(quals)
    ctx.align_set_pool_qual(None)
    assert call(sop) == -1                                    # dropped by hand
    with pytest.raises(api.IocError):
        ctx.align_pairs_polish_weighted(pairs, 11, segs, sop, 1)
    ctx.align_set_pool_qual(quals)
    other = next(g for g, (r, _) in enumerate(segs) if len(seqs[r]) != len(seqs[segs[sop[0]][0]]))
    assert call([other] + sop[1:]) == -1                      # a pair whose reference is not as long as its segment's frame
    assert call(sop, md=0) == -1
    assert call(sop, cap=bound - 1) == -4
    assert (out_s == 0xA5).all() and (out_q == 0xA5).all() and (off == -9).all() and (rec == -9).all() and (score == -9).all()
    assert call(sop) == 0
    assert [out_s[off[g]:off[g + 1]].tobytes() for g in range(len(segs))] == good["seq"] and np.array_equal(rec.view(api.POLISH_STATS_DTYPE), good["polish"])
