"""ioc_pileup_call: the consensus call of many references at once on the device (ioc_pile_call.hip), from host tables that are
uploaded.  Every segment's sequence, qualities and record must equal ioc_host_pileup_call of its rows (which tests/
test_pile_call_host.py holds against a restatement in Python): segment lengths around a wave and around the call kernels' chunk
of rows, many small segments beside a long one (the packed offsets), tables no aligner would produce with counts up to 2^32 - 1,
the tables written out by hand, frames with other letters, both depths.  Bytes and integers only, no tolerance; every refusal is
made on the host before a launch."""
import ctypes as C

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import polish_common as pc

pytestmark = pytest.mark.gpu

CHUNK = api.PILE_CALL_CHUNK


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _frames(rng, lens, letters=b"ACGT"):
    return [bytes(rng.choice(list(letters), n).astype(np.uint8)) for n in lens]


def _check(ctx, frames, cols, ins, min_depth):
    """One device call against the host definition, segment by segment; returns the records."""
    seqs, quals, st = ctx.pileup_call(frames, cols, ins, min_depth)
    assert len(seqs) == len(quals) == len(frames) and st.dtype == api.POLISH_STATS_DTYPE and st.shape == (len(frames),)
    at = 0
    for g, f in enumerate(frames):
        n = len(f) + 1
        want = api.pileup_call(cols[at:at + n], ins[at:at + n], f, min_depth)
        assert (seqs[g], quals[g]) == want[:2], (g, len(f))
        assert {k: int(st[k][g]) for k in api.POLISH_STATS_FIELDS} == want[2], (g, len(f))
        assert not st["reserved"][g].any()
        at += n
    return st


def _aligner_like(rng, frames, depth=9):
    """Tables as an aligner would leave them: the frame's base in the majority, some rows with another majority, a deletion or an
    insertion of 1 .. 7 bases, some rows below any depth."""
    n_rows = sum(len(f) + 1 for f in frames)
    cols, ins = np.zeros(n_rows, api.PILEUP_DTYPE), np.zeros(n_rows, api.PILEUP_INS_DTYPE)
    at = 0
    for f in frames:
        for p, b in enumerate(f):
            u, row = rng.random(), at + p
            d = depth if rng.random() > 0.1 else int(rng.integers(0, 4))
            ch = pc.COL_FIELDS[pc.CH.get(b, 4)]
            cols[ch][row] = d
            if u < 0.1 and d:
                cols[ch][row], cols[pc.COL_FIELDS[int(rng.integers(0, 6))]][row] = d // 3, d - d // 3
            if u > 0.85:
                for s in range(int(rng.integers(1, 8))):
                    if s < 6:
                        ins["slot"][row, s, int(rng.integers(0, 5))] = int(rng.integers(depth // 2, depth + 1))
                    else:
                        ins["longer"][row] = depth
        if rng.random() < 0.5:
            ins["slot"][at + len(f), 0, 1] = depth
        at += len(f) + 1
    return cols, ins


LENS = [0, 1, 63, 64, 65, CHUNK - 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 2, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1]


@pytest.mark.parametrize("min_depth", [1, 3])
def test_segment_lengths_around_a_wave_and_a_chunk(ctx, min_depth):
    """rlen + 1 rows at and next to 64, the chunk and twice the chunk: the carry down a segment's chunks, the last partial step."""
    rng = np.random.default_rng(1)
    frames = _frames(rng, LENS)
    cols, ins = _aligner_like(rng, frames)
    st = _check(ctx, frames, cols, ins, min_depth)
    assert st["n_ins"].sum() > 50 and st["n_del"].sum() > 5 and st["n_sub"].sum() > 20 and st["n_low"].sum() > 20
    cols, ins = pc.random_tables(rng, len(cols), values=(0, 1, 2, 3, 4, 5))
    _check(ctx, frames, cols, ins, min_depth)


def test_many_small_segments_beside_a_long_one(ctx):
    """300 segments of 0 .. 40 rows and one of 3000 in their midst: the scan over the segments, offsets behind a long output."""
    rng = np.random.default_rng(2)
    lens = [max(int(n) - 1, 0) for n in rng.integers(0, 41, 300)]
    lens.insert(150, 2999)
    frames = _frames(rng, lens)
    cols, ins = _aligner_like(rng, frames)
    for md in (1, 3):
        _check(ctx, frames, cols, ins, md)


@pytest.mark.parametrize("min_depth", [1, 3])
def test_tables_no_aligner_would_produce(ctx, min_depth):
    """Every counter drawn from {0, 1, 2, 3, 2^31, 2^32 - 1}: depths and insertion sums beyond 32 bits, qualities clamped."""
    rng = np.random.default_rng(3)
    frames = _frames(rng, [0, 5, 70, 300, 1, 257], b"ACGTNacgtRY")
    n_rows = sum(len(f) + 1 for f in frames)
    cols, ins = pc.random_tables(rng, n_rows, p_zero_ins=0.3)
    st = _check(ctx, frames, cols, ins, min_depth)
    assert st["n_ins"].sum() > 100


def test_hand_written_tables(ctx):
    """The tables of tests/polish_common.py, one segment each, in one call per depth; the expected bytes are written out there."""
    for md in (1, 3):
        names = [c[0] for c in pc.HAND_CALLS if c[4] == md]
        cases = [pc.hand_case(c) for c in pc.HAND_CALLS if c[4] == md]
        frames = [c[0] for c in cases]
        cols, ins = np.concatenate([c[1] for c in cases]), np.concatenate([c[2] for c in cases])
        seqs, quals, st = ctx.pileup_call(frames, cols, ins, md)
        for g, c in enumerate(cases):
            assert (seqs[g], quals[g]) == (c[4], c[5]), names[g]
            assert {k: int(st[k][g]) for k in api.POLISH_STATS_FIELDS} == c[6]


def test_frames_with_other_letters(ctx):
    """Letters other than A C G T in the frame: their channel is `other`, and where it wins the frame's byte goes out as it is."""
    rng = np.random.default_rng(4)
    frames = _frames(rng, [200, 77], b"ACGTNnacgtRYK-")
    cols, ins = _aligner_like(rng, frames)
    cols["other"] += ((rng.random(len(cols)) < 0.3) * 7).astype(np.uint32)
    st = _check(ctx, frames, cols, ins, 3)
    seqs = ctx.pileup_call(frames, cols, ins, 3)[0]
    assert any(b in seqs[0] for b in b"nacgtRYK-") and st["n_sub"].sum() > 0


def test_refusals_and_the_empty_call(ctx):
    L = _lib.load()
    rng = np.random.default_rng(5)
    frames = _frames(rng, [10, 0, 3])
    cols, ins = _aligner_like(rng, frames)
    seqs, quals, st = ctx.pileup_call([], np.zeros(0, api.PILEUP_DTYPE), np.zeros(0, api.PILEUP_INS_DTYPE))
    assert seqs == [] and quals == [] and st.shape == (0,)
    with pytest.raises(api.IocError):
        ctx.pileup_call(frames, cols, ins, 0)
    bound = sum(api.pileup_call_bound(len(f)) for f in frames)
    with pytest.raises(api.IocError) as e:
        ctx.pileup_call(frames, cols, ins, 3, cap=bound - 1)
    assert e.value.code == -4
    # the raw call: a refused call writes nothing
    rlen = np.array([len(f) for f in frames], np.int32)
    foff = np.array([0, 10, 10], np.int64)
    out_s, out_q = np.full(bound, 0xA5, np.uint8), np.full(bound, 0xA5, np.uint8)
    off, rec = np.full(4, -9, np.int64), np.full(3 * 8, -9, np.int32)
    def call(n, rl, md, cap):
        return L.ioc_pileup_call(ctx.h, n, rl.ctypes.data_as(C.POINTER(C.c_int32)), b"".join(frames), foff.ctypes.data_as(C.POINTER(C.c_int64)),
                                 cols.ctypes.data, ins.ctypes.data, md, out_s.ctypes.data, out_q.ctypes.data, cap,
                                 off.ctypes.data_as(C.POINTER(C.c_int64)), rec.ctypes.data)
    assert call(3, rlen, 0, bound) == -1
    assert call(3, np.array([10, -1, 3], np.int32), 3, bound) == -1
    assert call(-1, rlen, 3, bound) == -1
    assert call(3, rlen, 3, bound - 1) == -4
    assert (out_s == 0xA5).all() and (out_q == 0xA5).all() and (off == -9).all() and (rec == -9).all()
    assert call(3, rlen, 3, bound) == 0
    want = ctx.pileup_call(frames, cols, ins, 3)
    assert off[0] == 0 and [out_s[off[g]:off[g + 1]].tobytes() for g in range(3)] == want[0] and (out_s[off[3]:] == 0xA5).all()
    assert np.array_equal(rec.view(api.POLISH_STATS_DTYPE), want[2])
