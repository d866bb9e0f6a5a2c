"""ioc_align_pairs_polish: the batched GPU aligner piling every alignment into both tables on the device (the ins variant of
k_ops_pileup) and calling every segment's consensus there (ioc_pile_call.hip).  On the generators of tests/
test_gpu_align_pileup.py: the first table must equal ioc_align_pairs_pileup's, the second the sum of ioc_host_ops_pileup_ins over
the strings ioc_align_pairs_ops returns in the same context, the sequences, qualities, offsets and records ioc_host_pileup_call
of those tables, and score / windows / ratio a plain ioc_align_pairs.  Forced down another route — version 1, re-runs, slices —
the output must equal the unforced call's.  Bytes and integers only, no tolerance; refusals are made on the host."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import polish_common as pc
from tests.align_ops_checks import revcomp
from tests.test_gpu_align import _mutate
from tests.test_gpu_align_ops import _route_pairs, _small_pairs, refuted_pairs
from tests.test_gpu_align_stats import block_gap_pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _segments(pairs):
    """One segment per (reference, frame) the pairs use, in order of first use: (segs, seg_of_pair)."""
    index, segs, sop = {}, [], []
    for pr in pairs:
        key = (pr[1], int(bool(pr[2])))
        if key not in index:
            index[key] = len(segs)
            segs.append(key)
        sop.append(index[key])
    return segs, sop


def _same(a, b):
    return (a["seq"] == b["seq"] and a["qual"] == b["qual"] and np.array_equal(a["polish"], b["polish"]) and np.array_equal(a["cols"], b["cols"]) and
            np.array_equal(a["ins"], b["ins"]) and np.array_equal(a["score"], b["score"]) and np.array_equal(a["windows"], b["windows"]) and
            np.array_equal(a["ratio"], b["ratio"]))


def _check(ctx, seqs, pairs, k, min_depth=3, set_pool=True, plain=None, segs=None, sop=None, stats=False):
    if set_pool:
        ctx.align_set_pool(seqs)
    if segs is None:
        segs, sop = _segments(pairs)
    got = ctx.align_pairs_polish(pairs, k, segs, sop, min_depth, tables=True, stats=stats)
    row0 = [int(x) for x in got["row0"]]
    n_rows = sum(len(seqs[r]) + 1 for r, _ in segs)
    assert got["cols"].shape == got["ins"].shape == (n_rows,)
    if plain is None:
        plain = ctx.align_pairs(pairs, k)
    assert np.array_equal(got["score"], plain[0]) and np.array_equal(got["windows"], plain[1]) and np.array_equal(got["ratio"], plain[2])
    row_base = [row0[g] for g in sop]
    assert np.array_equal(got["cols"], ctx.align_pairs_pileup(pairs, k, row_base, n_rows)[3])
    dev_ops = ctx.align_pairs_ops(pairs, k)[3]
    want_ins = np.zeros(n_rows, api.PILEUP_INS_DTYPE)
    for pr, ops, rb in zip(pairs, dev_ops, row_base):
        m = len(seqs[pr[1]])
        api.ops_pileup_ins(ops, seqs[pr[0]], m, ins=want_ins[rb:rb + m + 1])
    bad = np.flatnonzero(got["ins"] != want_ins)
    assert bad.size == 0, (len(bad), int(bad[0]), got["ins"][bad[0]], want_ins[bad[0]])
    for g, (ref, rc) in enumerate(segs):
        frame = revcomp(seqs[ref]) if rc else seqs[ref]
        rows = slice(row0[g], row0[g] + len(frame) + 1)
        want = api.pileup_call(got["cols"][rows], got["ins"][rows], frame, min_depth)
        assert (got["seq"][g], got["qual"][g]) == want[:2], g
        assert {f: int(got["polish"][f][g]) for f in api.POLISH_STATS_FIELDS} == want[2], g
    if stats:
        assert np.array_equal(got["stats"], ctx.align_pairs_stats(pairs, k)[3])
    # without the tables the same sequences come back
    lean = ctx.align_pairs_polish(pairs, k, segs, sop, min_depth)
    assert lean["seq"] == got["seq"] and lean["qual"] == got["qual"] and np.array_equal(lean["polish"], got["polish"]) and "cols" not in lean
    return got


def test_small_random_pairs(ctx):
    """Lengths 0 .. 200 incl. empty sequences, every gap-open class, half against the reverse complement: one segment per
    (reference, frame), most with one or two pairs — so depth 1 calls and depth 3 keeps."""
    seqs, pairs = _small_pairs(13)
    a = _check(ctx, seqs, pairs, 11, min_depth=1, stats=True)
    b = _check(ctx, seqs, pairs, 11, min_depth=3, set_pool=False)
    assert a["polish"]["n_sub"].sum() > 0 and a["polish"]["n_ins"].sum() > 0 and a["polish"]["n_del"].sum() > 0
    assert b["polish"]["n_low"].sum() > a["polish"]["n_low"].sum()


def test_block_gaps(ctx):
    """block_gap_pairs(): gaps of 1 .. 200 bases in one block — insertions far beyond the six slots (`longer`), and 480 pairs
    piled on one set of rows in two frames."""
    seqs, pairs, what = block_gap_pairs()
    got = _check(ctx, seqs, pairs, 11)
    assert got["ins"]["longer"].sum() > 1000


def test_many_reads_on_one_segment(ctx):
    """Contention: 300 reads at 10 % divergence of one 300-base reference, all adding into one segment's rows; the call then
    returns the reference itself (every column has a large majority for it)."""
    rng = random.Random(17)
    ref = bytes(rng.choice(b"ACGT") for _ in range(300))
    reads = [_mutate(rng, ref, 0.1) for _ in range(300)]
    seqs = [ref, revcomp(ref)] + reads
    got = _check(ctx, seqs, [(2 + i, 0, 0, 0.2) for i in range(300)], 11)
    assert got["seq"] == [ref]
    mixed = [(2 + i, i % 2, i % 2, 0.2) for i in range(300)]   # the same frame through the stored reverse complement
    got2 = _check(ctx, seqs, mixed, 11, set_pool=False, segs=[(0, 0)], sop=[0] * 300)
    assert got2["seq"] == [ref] and np.array_equal(got2["ins"], got["ins"])


def test_identical_reads_closed_form(ctx):
    """The anchor of tests/test_pile_call_host.py on the device, in both frames: five reads equal to T bring the representative
    back to exactly T, every quality 40."""
    T, rep = pc.anchor()
    seqs = [rep, revcomp(rep)] + [T] * 5
    ctx.align_set_pool(seqs)
    for ref, rc in ((0, 0), (1, 1)):
        got = ctx.align_pairs_polish([(2 + i, ref, rc, 0.1) for i in range(5)], 11, [(ref, rc)], [0] * 5, 3)
        assert got["seq"] == [T] and got["qual"] == [bytes([73]) * 300]
        assert [int(got["polish"][f][0]) for f in ("out_len", "n_sub", "n_del", "n_ins", "n_low")] == [300, 1, 1, 2, 0]


def test_letters_other_than_acgt_and_a_reverse_complemented_frame(ctx):
    """Other letters in reads and frames, frames taken reverse-complemented on the fly (only A C G T are complemented)."""
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
    got = _check(ctx, seqs, pairs, 11, min_depth=1, stats=True)
    assert got["cols"]["other"].sum() > 40 and got["polish"]["n_sub"][-1] > 0
    # above every depth the frames come back as they are: the last one the reverse complement of the stored sequence, its other
    # letters where the reversal puts them and unchanged
    segs, sop = _segments(pairs)
    kept = ctx.align_pairs_polish(pairs, 11, segs, sop, 4)
    assert kept["seq"] == [revcomp(seqs[r]) if rc else seqs[r] for r, rc in segs] and any(b in kept["seq"][-1] for b in b"nKy")
    assert all(set(q) == {33} for q in kept["qual"])


@pytest.mark.parametrize("env", [{"IOC_ALIGN_V1": "1"}, {"IOC_ALIGN_ARENA": "fat"}, {"IOC_ALIGN_CORRIDOR": "0"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_every_route(ctx, monkeypatch, env):
    seqs, pairs = _route_pairs()
    segs, sop = _segments(pairs)
    ctx.align_set_pool(seqs)
    unforced = ctx.align_pairs_polish(pairs, 11, segs, sop, 1, tables=True)
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    assert _same(_check(ctx, seqs, pairs, 11, min_depth=1, set_pool=False), unforced)
    if "IOC_ALIGN_V1" in env or "IOC_ALIGN_ARENA" in env:
        assert ctx.timings()["align_version"] == 1


def test_v2_refusals_come_back_through_version_1(ctx, monkeypatch):
    """Pairs the 16-bit window refuses, and the whole batch after a wait that "ran out": the run that answers a pair adds it to
    both tables, once."""
    seqs, pairs = _route_pairs()
    pairs = [p for p in pairs if len(seqs[p[0]]) and len(seqs[p[1]])]
    segs, sop = _segments(pairs)
    ctx.align_set_pool(seqs)
    plain = ctx.align_pairs(pairs, 11)
    unforced = ctx.align_pairs_polish(pairs, 11, segs, sop, 1, tables=True)
    monkeypatch.setenv("IOC_ALIGN_V2_GUARD", "40")
    t0 = ctx.timings()["n_align_refused"]
    guarded = ctx.align_pairs_polish(pairs, 11, segs, sop, 1, tables=True)
    assert ctx.timings()["n_align_refused"] - t0 >= 5, "the guard did not refuse the pairs: the case no longer does what it claims"
    assert _same(guarded, unforced)
    monkeypatch.delenv("IOC_ALIGN_V2_GUARD")
    monkeypatch.setenv("IOC_ALIGN_V2_FAKE_TIMEOUT", "1")
    t1 = ctx.timings()["n_align_refused"]
    timed_out = ctx.align_pairs_polish(pairs, 11, segs, sop, 1, tables=True)
    assert ctx.timings()["n_align_refused"] - t1 == len(pairs) and ctx.timings()["align_version"] == 1
    assert _same(timed_out, unforced)
    monkeypatch.delenv("IOC_ALIGN_V2_FAKE_TIMEOUT")
    _check(ctx, seqs, pairs, 11, min_depth=1, set_pool=False, plain=plain)


def test_pair_the_corridor_cannot_vouch_for(ctx, monkeypatch, capfd):
    """Pairs that come back from version 2 without an answer and are run again: the re-run adds them; and the trace line."""
    seqs, pairs = refuted_pairs()
    segs, sop = _segments(pairs)
    ctx.align_set_pool(seqs)
    unforced = ctx.align_pairs_polish(pairs, 11, segs, sop, 1, tables=True)
    monkeypatch.setenv("IOC_ALIGN_CORRIDOR", "0.15")
    monkeypatch.setenv("IOC_TRACE", "1")
    capfd.readouterr()
    got = ctx.align_pairs_polish(pairs, 11, segs, sop, 1, tables=True)
    err = capfd.readouterr().err
    assert "2 of 3 pairs run again without a corridor" in err, err[-2000:]
    assert "polish:" in err and "k_ops_pileup<ins>" in err and "k_pile_call" in err and "operation bytes:" not in err
    monkeypatch.delenv("IOC_TRACE")
    assert _same(got, unforced)
    _check(ctx, seqs, pairs, 11, min_depth=1, set_pool=False)


def test_bound_above_the_budget_runs_in_slices(ctx, monkeypatch):
    """192 pairs of 3 kb on 12 segments under a budget of 1 MB: the call runs in slices, both tables stay on the device across
    them, and the output equals the unsliced call's."""
    rng = random.Random(23)
    base = bytes(rng.choice(b"ACGT") for _ in range(3000))
    seqs = [_mutate(rng, base, 0.1) for _ in range(12)]
    pairs = [(i, (i + 1) % 12, i % 2, 0.2) for i in range(12)] * 16
    ref = _check(ctx, seqs, pairs, 11)
    segs, sop = _segments(pairs)
    monkeypatch.setenv("IOC_ALIGN_CK_BUDGET_MB", "1")
    got = ctx.align_pairs_polish(pairs, 11, segs, sop, 3, tables=True)
    assert ctx.timings()["align_slices"] > 1
    assert _same(got, ref)


def test_a_segment_without_pairs(ctx):
    """Its frame comes back as it is, quality 0 throughout — also reverse-complemented, also of length 0, also with no pair at all."""
    rng = random.Random(31)
    seqs = [bytes(rng.choice(b"ACGTN") for _ in range(n)) for n in (120, 300, 0, 90)]
    seqs.append(_mutate(rng, seqs[1], 0.05))
    ctx.align_set_pool(seqs)
    segs = [(0, 1), (1, 0), (2, 0), (3, 0)]
    got = ctx.align_pairs_polish([(4, 1, 0, 0.1)] * 3, 11, segs, [1, 1, 1], 3, tables=True)
    assert got["seq"][0] == revcomp(seqs[0]) and got["seq"][2] == b"" and got["seq"][3] == seqs[3]
    assert got["qual"][0] == b"!" * 120 and got["qual"][3] == b"!" * 90
    assert list(got["polish"]["n_low"]) == [120, int(got["polish"]["n_low"][1]), 0, 90] and got["polish"]["n_low"][1] < 30
    none = ctx.align_pairs_polish([], 11, segs, [], 3)
    assert none["seq"] == [revcomp(seqs[0]), seqs[1], b"", seqs[3]] and none["qual"] == [b"!" * len(s) for s in none["seq"]]


def test_refusals_and_the_empty_call(ctx):
    L = _lib.load()
    seqs, pairs = _small_pairs(29, 30)
    pairs = pairs[:6]
    segs, sop = _segments(pairs)
    ctx.align_set_pool(seqs)
    empty = ctx.align_pairs_polish([], 11, [], [], 3, tables=True)
    assert empty["seq"] == [] and empty["polish"].shape == (0,) and empty["cols"].shape == (0,) and len(empty["score"]) == 0
    good = ctx.align_pairs_polish(pairs, 11, segs, sop, 1)
    bound = sum(api.pileup_call_bound(len(seqs[r])) for r, _ in segs)
    with pytest.raises(api.IocError):
        ctx.align_pairs_polish(pairs, 11, segs, sop, 0)
    with pytest.raises(api.IocError) as e:
        ctx.align_pairs_polish(pairs, 11, segs, sop, 1, cap=bound - 1)
    assert e.value.code == -4
    # the raw call: every refusal writes nothing
    arr = ctx._aln_pairs(pairs)
    sarr = (_lib.PolishSeg * len(segs))(*[_lib.PolishSeg(r, rc) for r, rc in segs])
    out_s, out_q = np.full(bound, 0xA5, np.uint8), np.full(bound, 0xA5, np.uint8)
    off, rec, score = np.full(len(segs) + 1, -9, np.int64), np.full(len(segs) * 8, -9, np.int32), np.full(len(pairs), -9, np.int32)
    def call(sop_, md=1, cap=bound, sarr_=sarr):
        s = np.asarray(sop_, np.int32)
        return L.ioc_align_pairs_polish(ctx.h, len(pairs), arr, 11, 2, -2, 1, score.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, len(segs),
                                        sarr_, s.ctypes.data_as(C.POINTER(C.c_int32)), md, out_s.ctypes.data, out_q.ctypes.data, cap,
                                        off.ctypes.data_as(C.POINTER(C.c_int64)), rec.ctypes.data, None, None)
    other = next(g for g, (r, _) in enumerate(segs) if len(seqs[r]) != len(seqs[segs[sop[0]][0]]))
    assert call([other] + sop[1:]) == -1                      # a pair whose reference is not as long as its segment's frame
    assert call([len(segs)] + sop[1:]) == -1 and call([-1] + sop[1:]) == -1
    assert call(sop, md=0) == -1
    assert call(sop, cap=bound - 1) == -4
    outside = (_lib.PolishSeg * len(segs))(*[_lib.PolishSeg(len(seqs), 0) for _ in segs])
    assert call(sop, sarr_=outside) == -1
    assert (out_s == 0xA5).all() and (out_q == 0xA5).all() and (off == -9).all() and (rec == -9).all() and (score == -9).all()
    assert call(sop) == 0
    assert [out_s[off[g]:off[g + 1]].tobytes() for g in range(len(segs))] == good["seq"] and np.array_equal(rec.view(api.POLISH_STATS_DTYPE), good["polish"])
