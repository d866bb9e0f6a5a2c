"""ioc_pileup_sites: the site kernels (ioc_pile_sites.hip) over uploaded tables against the host definition, ioc_host_pileup_sites,
segment by segment — at the sizes where the scans can go wrong: around a wave and around a workgroup's chunk of
PILE_CALL_CHUNK rows, rows that yield two records each, more kept sites than a wave and than two, more segments than one step
of the segment scan, and max_sites cutting inside a chunk and at its edge.  Records and integers only, no tolerance."""
import ctypes as C

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import polish_common as pc
from tests import sites_common as sc

pytestmark = pytest.mark.gpu

CHUNK = api.PILE_CALL_CHUNK


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _check(ctx, rlen, cols, md=3, ma=3, mp=25, mx=4096):
    got, found = ctx.pileup_sites(rlen, cols, md, ma, mp, mx)
    assert len(got) == len(rlen) and found.shape == (len(rlen),)
    row = 0
    for g, r in enumerate(rlen):
        want, n = api.pileup_sites(cols[row:row + r + 1], md, ma, mp, mx)
        assert int(found[g]) == n, (g, r)
        assert got[g].tobytes() == want.tobytes(), (g, r, len(got[g]), len(want))
        row += r + 1
    return got, found


def test_hand_tables_on_the_device(ctx):
    for name, rows, (md, ma, mp, mx), want, n_found in sc.HAND_SITES:
        got, found = ctx.pileup_sites([len(rows) - 1], sc.table(rows), md, ma, mp, mx)
        assert (sc.as_tuples(got[0]), int(found[0])) == (want, n_found), name
    # ... and all of them as the segments of one call, under one rule
    rlen = [len(rows) - 1 for _, rows, *_ in sc.HAND_SITES]
    _check(ctx, rlen, np.concatenate([sc.table(rows) for _, rows, *_ in sc.HAND_SITES]), 3, 3, 25, 2)


def test_lengths_around_a_wave_and_a_chunk(ctx):
    rng = np.random.default_rng(41)
    rlen = [0, 1, 63, 64, CHUNK - 1, CHUNK, CHUNK + 1, 600]
    cols, _ = pc.random_tables(rng, sum(rlen) + len(rlen), values=(0, 3, 10, 11, 40))
    got, found = _check(ctx, rlen, cols)
    assert found[-1] > 128 and found[2] > 0
    for r in rlen:   # each alone: a call of one segment
        one, _ = pc.random_tables(rng, r + 1, values=(0, 1, 2, 3, 2**31, sc.M32))
        _check(ctx, [r], one, 1, 1, 10)
    _check(ctx, rlen, cols, 11, 4, 50, 7)


def test_every_row_yields_two_records(ctx):
    """rlen 600: rows 0 .. 599 an insertion site and a base site each, row 600 an insertion site — 1201 records, placed by the
    wave scan, the workgroup scan and the carry down three chunks; and max_sites cutting inside a chunk and at its edge."""
    rlen = 600
    cols = sc.table([(6, 4, 0, 0, 0, 0, 5)] * rlen + [(0, 0, 0, 0, 0, 0, 4)])
    got, found = _check(ctx, [rlen], cols)
    assert int(found[0]) == 2 * rlen + 1 == len(got[0])
    assert got[0]["row"].tolist() == [p // 2 for p in range(2 * rlen + 1)] and got[0]["kind"].tolist() == ([1, 0] * rlen + [1])
    for mx in (1, 63, 64, 65, 129, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 4 * CHUNK, 1200, 1201, 1202):
        kept, n = _check(ctx, [rlen], cols, mx=mx)
        assert len(kept[0]) == min(mx, 1201) and int(n[0]) == 1201
    # among other segments: the offsets of the ones behind it move with what it keeps
    cols3 = np.concatenate([sc.table([(7, 3, 0, 0, 0, 0, 0), sc.Z]), cols, sc.table([(5, 5, 0, 0, 0, 0, 5)] * 70 + [sc.Z])])
    for mx in (1, 100, 2 * CHUNK, 4096):
        _check(ctx, [1, rlen, 70], cols3, mx=mx)


def test_many_tiny_segments(ctx):
    """130 segments of 0 .. 3 bases: the segment scan takes three steps, its carry runs over two of them."""
    rng = np.random.default_rng(43)
    rlen = [int(x) for x in rng.integers(0, 4, 130)]
    cols, _ = pc.random_tables(rng, sum(rlen) + len(rlen), values=(0, 3, 4, 10))
    got, found = _check(ctx, rlen, cols, 3, 3, 25)
    assert found.sum() > 64 and (found[70:] > 0).any() and (found == 0).any()
    _check(ctx, rlen, cols, 3, 3, 25, mx=1)
    empty, none = ctx.pileup_sites([], np.zeros(0, api.PILEUP_DTYPE))
    assert empty == [] and none.shape == (0,)


def test_refusals_write_nothing(ctx):
    L = _lib.load()
    rlen = np.array([5, 0, 2], np.int32)
    cols = sc.table([(6, 4, 0, 0, 0, 0, 5)] * 10)
    bound = sum(api.pileup_sites_bound(r, 4) for r in rlen)
    assert bound == 4 + 1 + 4
    out, off, found = np.full(bound * 8, -9, np.int32), np.full(4, -9, np.int64), np.full(3, -9, np.int64)
    def call(md=3, ma=3, mp=25, mx=4, cap=bound, n=3, r=rlen):
        return L.ioc_pileup_sites(ctx.h, n, r.ctypes.data_as(C.POINTER(C.c_int32)), cols.ctypes.data, md, ma, mp, mx, out.ctypes.data, cap,
                                  off.ctypes.data_as(C.POINTER(C.c_int64)), found.ctypes.data_as(C.POINTER(C.c_int64)))
    assert call(cap=bound - 1) == -4
    assert call(md=0) == -1 and call(ma=0) == -1 and call(mp=0) == -1 and call(mp=51) == -1 and call(mx=0) == -1 and call(n=-1) == -1
    assert call(r=np.array([5, -1, 2], np.int32)) == -1
    assert (out == -9).all() and (off == -9).all() and (found == -9).all()
    assert call() == 0
    assert off.tolist() == [0, 4, 4, 8] and found.tolist() == [11, 0, 5]
    with pytest.raises(api.IocError) as e:
        ctx.pileup_sites(rlen, cols, max_sites=4, cap=bound - 1)
    assert e.value.code == -4
