"""ioc_pileup_call_weighted: the weighted mode of the call kernels (ioc_pile_call.hip) from host tables that are uploaded — the
table of counts for the depth gates, the two tables of weights for everything else.  Every segment's sequence, qualities and
record must equal ioc_host_pileup_call_weighted of its rows (which tests/test_pile_weight_host.py holds against a restatement in
Python): the tables written out by hand, tables no aligner would produce, segment lengths around the kernels' chunk of rows, many
short segments.  Bytes and integers only, no tolerance; every refusal is made on the host before a launch."""
import ctypes as C

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import polish_common as pc
from tests import polish_weight_common as pw
from tests.test_gpu_pile_call import _aligner_like, _frames

pytestmark = pytest.mark.gpu

CHUNK = api.PILE_CALL_CHUNK


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _check(ctx, frames, cols, wcols, wins, min_depth):
    """One device call against the host definition, segment by segment; returns the records."""
    seqs, quals, st = ctx.pileup_call_weighted(frames, cols, wcols, wins, min_depth)
    assert len(seqs) == len(quals) == len(frames) and st.dtype == api.POLISH_STATS_DTYPE and st.shape == (len(frames),)
    at = 0
    for g, f in enumerate(frames):
        n = len(f) + 1
        want = api.pileup_call_weighted(cols[at:at + n], wcols[at:at + n], wins[at:at + n], f, min_depth)
        assert (seqs[g], quals[g]) == want[:2], (g, len(f))
        assert {k: int(st[k][g]) for k in api.POLISH_STATS_FIELDS} == want[2], (g, len(f))
        assert not st["reserved"][g].any()
        at += n
    return st


def _weights_like(rng, cols, ins):
    """Weights an aligner could leave beside these counts: every event between 1 and 93."""
    wcols, wins = cols.copy(), ins.copy()
    for f in pc.COL_FIELDS:
        wcols[f] = cols[f] * rng.integers(1, 94, len(cols)).astype(np.uint32)
    wins["slot"] = ins["slot"] * rng.integers(1, 94, ins["slot"].shape).astype(np.uint32)
    return wcols, wins


def test_hand_written_tables(ctx):
    """The tables of tests/polish_weight_common.py and, with the counts as their own weights, those of tests/polish_common.py: one
    segment each, one call per depth; the expected bytes are written out there."""
    mine = [pw.hand_case_w(c) for c in pw.HAND_CALLS_W]
    theirs = [(f, cols, cols, ins, md, seq, qual, st) for f, cols, ins, md, seq, qual, st in map(pc.hand_case, pc.HAND_CALLS)]
    for md in (1, 3):
        cases = [c for c in mine + theirs if c[4] == md]
        assert len(cases) > 5
        frames = [c[0] for c in cases]
        seqs, quals, st = ctx.pileup_call_weighted(frames, *(np.concatenate([c[x] for c in cases]) for x in (1, 2, 3)), md)
        for g, c in enumerate(cases):
            assert (seqs[g], quals[g]) == (c[5], c[6]), (md, g)
            assert {k: int(st[k][g]) for k in api.POLISH_STATS_FIELDS} == c[7], (md, g)


@pytest.mark.parametrize("min_depth", [1, 3])
def test_tables_no_aligner_would_produce(ctx, min_depth):
    """Every counter of all three tables drawn at random, up to 2^32 - 1: sums beyond 32 bits, both gates, qualities clamped."""
    rng = np.random.default_rng(13)
    frames = _frames(rng, [0, 5, 70, 300, 1, 257], b"ACGTNacgtRY")
    n_rows = sum(len(f) + 1 for f in frames)
    cols, wcols, wins = pw.random_tables_w(rng, n_rows)
    st = _check(ctx, frames, cols, wcols, wins, min_depth)
    assert st["n_ins"].sum() > 50
    # shallow counts under light and heavy weights, a fifth of the rows without any weight: both gates close on some rows
    cols, _ = pc.random_tables(rng, n_rows, values=(0, 0, 0, 1))
    _, wcols, wins = pw.random_tables_w(rng, n_rows, values=(0, 1, 2, 40, 93))
    for f in pc.COL_FIELDS:
        wcols[f][::5] = 0
    st = _check(ctx, frames, cols, wcols, wins, min_depth)
    assert st["n_low"].sum() >= 100 and st["n_ins"].sum() > 0


@pytest.mark.parametrize("min_depth", [1, 3])
def test_segment_lengths_around_a_chunk(ctx, min_depth):
    """255, 256, 257, 513 and 0 bases: the carry down a segment's chunks, the last partial step, the empty segment."""
    rng = np.random.default_rng(11)
    frames = _frames(rng, [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 0])
    cols, ins = _aligner_like(rng, frames)
    wcols, wins = _weights_like(rng, cols, ins)
    st = _check(ctx, frames, cols, wcols, wins, min_depth)
    assert st["n_ins"].sum() > 10 and st["n_sub"].sum() > 5 and st["n_low"].sum() > 5


def test_many_short_segments(ctx):
    """300 segments of 0 .. 40 rows: the scan over the segments and the packed offsets."""
    rng = np.random.default_rng(12)
    frames = _frames(rng, [max(int(n) - 1, 0) for n in rng.integers(0, 41, 300)])
    cols, ins = _aligner_like(rng, frames)
    wcols, wins = _weights_like(rng, cols, ins)
    for md in (1, 3):
        _check(ctx, frames, cols, wcols, wins, md)


def test_refusals_and_the_empty_call(ctx):
    L = _lib.load()
    rng = np.random.default_rng(15)
    frames = _frames(rng, [10, 0, 3])
    cols, ins = _aligner_like(rng, frames)
    wcols, wins = _weights_like(rng, cols, ins)
    seqs, quals, st = ctx.pileup_call_weighted([], *(np.zeros(0, t) for t in (api.PILEUP_DTYPE, api.PILEUP_DTYPE, api.PILEUP_INS_DTYPE)))
    assert seqs == [] and quals == [] and st.shape == (0,)
    bound = sum(api.pileup_call_bound(len(f)) for f in frames)
    with pytest.raises(api.IocError) as e:
        ctx.pileup_call_weighted(frames, cols, wcols, wins, 3, cap=bound - 1)
    assert e.value.code == -4
    rlen = np.array([len(f) for f in frames], np.int32)
    foff = np.array([0, 10, 10], np.int64)
    out_s, out_q = np.full(bound, 0xA5, np.uint8), np.full(bound, 0xA5, np.uint8)
    off, rec = np.full(4, -9, np.int64), np.full(3 * 8, -9, np.int32)
    def call(n, rl, md, cap, wc=wcols.ctypes.data):
        return L.ioc_pileup_call_weighted(ctx.h, n, rl.ctypes.data_as(C.POINTER(C.c_int32)), b"".join(frames), foff.ctypes.data_as(C.POINTER(C.c_int64)),
                                          cols.ctypes.data, wc, wins.ctypes.data, md, out_s.ctypes.data, out_q.ctypes.data, cap,
                                          off.ctypes.data_as(C.POINTER(C.c_int64)), rec.ctypes.data)
    assert call(3, rlen, 0, bound) == -1
    assert call(3, np.array([10, -1, 3], np.int32), 3, bound) == -1
    assert call(3, rlen, 3, bound, wc=None) == -1
    assert call(3, rlen, 3, bound - 1) == -4
    assert (out_s == 0xA5).all() and (out_q == 0xA5).all() and (off == -9).all() and (rec == -9).all()
    assert call(3, rlen, 3, bound) == 0
    want = ctx.pileup_call_weighted(frames, cols, wcols, wins, 3)
    assert off[0] == 0 and [out_s[off[g]:off[g + 1]].tobytes() for g in range(3)] == want[0] and (out_s[off[3]:] == 0xA5).all()
    assert np.array_equal(rec.view(api.POLISH_STATS_DTYPE), want[2])
