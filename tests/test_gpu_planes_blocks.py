"""ioc_planes_blocks: the kernels of ioc_read_blocks.hip over host base planes, against the host definition segment by segment, as
bytes — one call over the planted segments of blocks_common.planted_case with their pairs interleaved (tests/test_planes_blocks_host.py
measures what each planted shape is there for), the same call at max_blocks 1 and under a second rule, a small call after the large
one on the same context, the empty call and the refusals."""
import ctypes as C

import numpy as np
import pytest

from isonclust2_amd import api
from tests import blocks_common as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


@pytest.fixture(scope="module")
def planted():
    case = bc.planted_case()
    return case, bc.interleaved(case)


@pytest.mark.parametrize("rule", [{}, dict(max_blocks=1), bc.SECOND], ids=["default", "one_block", "second"])
def test_planted_segments_interleaved(ctx, planted, rule):
    case, (rlen, sop, planes, mine) = planted
    assert sorted({len(p) for _, p in case}) == [0, 1, 2, 3, 5, 64, 65, 130] and sop[:4] == [0, 1, 2, 3]
    want = bc.host_segments(case, **rule)
    got = ctx.planes_blocks(rlen, sop, planes, **rule)
    bc.same_as_host(got, want, mine)
    lean = ctx.planes_blocks(rlen, sop, planes, rows=False, **rule)
    assert "rows" not in lean and lean["reads"].tobytes() == got["reads"].tobytes() and lean["seg"].tobytes() == got["seg"].tobytes()
    if not rule:
        assert set(got["reads"]["how"].tolist()) == {0, 1, 2, 3}
        assert {s for g, w in enumerate(want) for row in bc.states(got["reads"][mine[g]], len(w["blocks"])) for s in row} == {0, 1, 2, 3}
        assert tuple(got["seg"][12][["n_blocks", "n_found", "n_groups"]]) == (32, 35, 3) and int(got["reads"]["key"].max()) >= 2**63
        assert [(int(b["first"]), int(b["end"])) for b in got["blocks"][11]] == [(50, 4150)]
    if rule.get("max_blocks") == 1:
        assert tuple(got["seg"][12][["n_blocks", "n_found"]]) == (1, 35)
    # a small call after the large one on the same context
    small = [c for c in case if c[0] in (64, 20)]
    r2, s2, p2, m2 = bc.interleaved(small)
    bc.same_as_host(ctx.planes_blocks(r2, s2, p2, **rule), bc.host_segments(small, **rule), m2)


def test_random_planes(ctx):
    rng = np.random.default_rng(3)
    case = [(rlen, bc.random_planes(rng, n, rlen)) for rlen, n in ((300, 40), (70, 7), (1000, 33), (5, 3))]
    rlen, sop, planes, mine = bc.interleaved(case)
    for rule in (dict(min_gap=3, min_depth=2, min_alt=2, min_pct=5, min_block=2), dict(min_gap=1, min_depth=1, min_alt=1, min_pct=1, min_block=1, max_blocks=7)):
        bc.same_as_host(ctx.planes_blocks(rlen, sop, planes, **rule), bc.host_segments(case, **rule), mine)


def test_the_empty_call_and_a_segment_without_pairs(ctx):
    got = ctx.planes_blocks([], [], [])
    assert got["blocks"] == [] and got["reads"].shape == (0,) and got["seg"].shape == (0,) and got["block_off"].tolist() == [0]
    got = ctx.planes_blocks([30, 0], [], [])
    assert got["block_off"].tolist() == [0, 0, 0] and not got["seg"].tobytes().strip(b"\0") and not got["rows"][0].tobytes().strip(b"\0")


def test_refusals_leave_the_outputs_untouched(ctx):
    rlen, n = 64, 64
    p = np.ascontiguousarray(dict(bc.planted_case())[64])
    rl, sop = np.array([rlen], np.int32), np.zeros(n, np.int32)
    good = [20, 3, 3, 25, 10, 32]
    fill = lambda dt, k: np.frombuffer(bytes([0xA5]) * (dt.itemsize * k), dt).copy()

    def call(rule, n_segs=1, n_pairs=n, sop=sop, base=p.ctypes.data, cap=32, boff=True, reads=True, seg=True, blocks=True):
        out = fill(api.BLOCK_ROW_DTYPE, rlen + 1), fill(api.PILE_BLOCK_DTYPE, 32), fill(np.dtype(np.int64), 2), fill(api.READ_BLOCKS_DTYPE, n), fill(api.BLOCKS_SEG_DTYPE, 1)
        before = [o.tobytes() for o in out]
        ptr = lambda o, on=True: o.ctypes.data if on else None
        rc = ctx.L.ioc_planes_blocks(ctx.h, n_segs, rl.ctypes.data_as(C.POINTER(C.c_int32)), n_pairs, sop.ctypes.data_as(C.POINTER(C.c_int32)), base, *rule, ptr(out[0]),
                                     ptr(out[1], blocks), cap, out[2].ctypes.data_as(C.POINTER(C.c_int64)) if boff else None, ptr(out[3], reads), ptr(out[4], seg))
        return rc, [o.tobytes() for o in out] == before

    assert call(good) == (0, False)
    for at, bad in ((0, 0), (1, 0), (2, 0), (3, 0), (3, 51), (4, 0), (5, 0), (5, 33)):
        rule = list(good)
        rule[at] = bad
        assert call(rule) == (-1, True), (at, bad)
    outside = sop.copy()
    outside[7] = 1
    negative = sop.copy()
    negative[0] = -1
    for kw in (dict(n_segs=-1), dict(n_pairs=-1), dict(sop=outside), dict(sop=negative), dict(base=None), dict(boff=False), dict(reads=False), dict(seg=False),
               dict(blocks=False), dict(cap=-1)):
        assert call(good, **kw) == (-1, True), kw
    assert call(good, cap=31) == (-4, True)
    with pytest.raises(api.IocError) as e:
        ctx.planes_blocks([rlen], sop, list(p), cap=31)
    assert e.value.code == -4
