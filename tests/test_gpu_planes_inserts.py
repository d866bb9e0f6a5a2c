"""ioc_planes_inserts: the kernels of ioc_read_inserts.hip over host planes, against the host definition segment by segment, as bytes
— one call over the planted segments of inserts_common.planted_case with their pairs interleaved (tests/test_planes_inserts_host.py
measures what each planted shape is there for), at slack 8, 0 and 32, each a call of its own rule, at max_sites 1 and without block
words; a small call after the large one on the same context, random planes, the empty call and the refusals."""
import ctypes as C

import numpy as np
import pytest

from isonclust2_amd import api
from tests import inserts_common as ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


@pytest.fixture(scope="module")
def planted():
    case = ic.planted_case()
    return case, ic.interleaved(case)


@pytest.mark.parametrize("rule", [{}, dict(slack=0), dict(slack=32), dict(max_sites=1)], ids=["slack8", "slack0", "slack32", "one_site"])
def test_planted_segments_interleaved(ctx, planted, rule):
    case, (rlen, sop, planes, lens, pk, pm, pf, mine) = planted
    assert sorted({len(b) for _, b, _, _ in case}) == [0, 1, 3, 6, 64, 65, 130] and sop[:4] == [0, 1, 2, 3]
    want = ic.host_segments(case, **rule)
    got = ctx.planes_inserts(rlen, sop, planes, lens, pre_key=pk, pre_mask=pm, pre_full=pf, **rule)
    ic.same_as_host(got, want, mine)
    lean = ctx.planes_inserts(rlen, sop, planes, lens, pre_key=pk, pre_mask=pm, pre_full=pf, rows=False, **rule)
    assert "rows" not in lean and lean["reads"].tobytes() == got["reads"].tobytes() and lean["seg"].tobytes() == got["seg"].tobytes()
    if not rule:
        assert set(got["reads"]["how"].tolist()) == {0, 1, 2, 3}
        assert tuple(got["seg"][11][["n_sites", "n_found", "n_groups"]]) == (32, 35, 3) and int(got["reads"]["key"].max()) >= 2**63
        assert [(int(s["first"]), int(s["end"])) for s in got["sites"][10]] == [(1992, 2009), (4092, 4099)]
        assert int(got["seg"][9]["n_groups"]) == 6
    if rule.get("slack") == 32:
        assert int(got["sites"][4][0]["len_max"]) == 65 * 255
    if rule.get("max_sites") == 1:
        assert tuple(got["seg"][11][["n_sites", "n_found"]]) == (1, 35)
    # the stage on its own: no block words
    ic.same_as_host(ctx.planes_inserts(rlen, sop, planes, lens, **rule), ic.host_segments(case, with_pre=False, **rule), mine)
    # a small call after the large one on the same context
    small = [c for c in case if c[0] in (64, 2)]
    r2, s2, p2, l2, k2, m2, f2, mine2 = ic.interleaved(small)
    ic.same_as_host(ctx.planes_inserts(r2, s2, p2, l2, pre_key=k2, pre_mask=m2, pre_full=f2, **rule), ic.host_segments(small, **rule), mine2)


def test_random_planes(ctx):
    rng = np.random.default_rng(3)
    case = []
    for rlen, n in ((300, 40), (70, 7), (1000, 33), (5, 3)):
        b, l = ic.random_planes(rng, n, rlen)
        case.append((rlen, b, l, ic.random_pre(rng, n)))
    rlen, sop, planes, lens, pk, pm, pf, mine = ic.interleaved(case)
    for rule in (dict(min_ins=3, slack=1, min_depth=2, min_alt=2, min_pct=5), dict(min_ins=1, slack=31, min_depth=1, min_alt=1, min_pct=1, max_sites=7),
                 dict(min_ins=20, slack=8, min_depth=1, min_alt=1, min_pct=1)):
        ic.same_as_host(ctx.planes_inserts(rlen, sop, planes, lens, pre_key=pk, pre_mask=pm, pre_full=pf, **rule), ic.host_segments(case, **rule), mine)


def test_the_empty_call_and_a_segment_without_pairs(ctx):
    got = ctx.planes_inserts([], [], [], [])
    assert got["sites"] == [] and got["reads"].shape == (0,) and got["seg"].shape == (0,) and got["site_off"].tolist() == [0]
    got = ctx.planes_inserts([30, 0], [], [], [])
    assert got["site_off"].tolist() == [0, 0, 0] and not got["seg"].tobytes().strip(b"\0") and not got["rows"][0].tobytes().strip(b"\0")


def test_refusals_leave_the_outputs_untouched(ctx):
    _, b, l, _ = ic.planted_case()[4]
    b, l = np.ascontiguousarray(b), np.ascontiguousarray(l)
    n, rlen = b.shape[0], b.shape[1] - 1
    rl, sop = np.array([rlen], np.int32), np.zeros(n, np.int32)
    pk, pm, pf = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(1, np.uint64)
    good = [20, 8, 3, 3, 25, 32]
    fill = lambda dt, k: np.frombuffer(bytes([0xA5]) * (dt.itemsize * k), dt).copy()

    def call(rule, n_segs=1, n_pairs=n, sop=sop, base=b.ctypes.data, ilen=l.ctypes.data, pre=(None, None, None), cap=32, soff=True, reads=True, seg=True, sites=True):
        out = fill(api.INSERT_ROW_DTYPE, rlen + 1), fill(api.PILE_INSERT_DTYPE, 32), fill(np.dtype(np.int64), 2), fill(api.READ_INSERTS_DTYPE, n), fill(api.INSERTS_SEG_DTYPE, 1)
        before = [o.tobytes() for o in out]
        ptr = lambda o, on=True: o.ctypes.data if on else None
        rc = ctx.L.ioc_planes_inserts(ctx.h, n_segs, rl.ctypes.data_as(C.POINTER(C.c_int32)), n_pairs, sop.ctypes.data_as(C.POINTER(C.c_int32)), base, ilen, *rule, *pre,
                                      ptr(out[0]), ptr(out[1], sites), cap, out[2].ctypes.data_as(C.POINTER(C.c_int64)) if soff else None, ptr(out[3], reads),
                                      ptr(out[4], seg))
        return rc, [o.tobytes() for o in out] == before

    assert call(good) == (0, False) and call(good, pre=(pk.ctypes.data, pm.ctypes.data, pf.ctypes.data)) == (0, False)
    for at, bad in ((0, 0), (0, 256), (1, -1), (1, 33), (2, 0), (3, 0), (4, 0), (4, 51), (5, 0), (5, 33)):
        rule = list(good)
        rule[at] = bad
        assert call(rule) == (-1, True), (at, bad)
    outside = sop.copy()
    outside[7] = 1
    negative = sop.copy()
    negative[0] = -1
    for kw in (dict(n_segs=-1), dict(n_pairs=-1), dict(sop=outside), dict(sop=negative), dict(base=None), dict(ilen=None), dict(soff=False), dict(reads=False),
               dict(seg=False), dict(sites=False), dict(cap=-1), dict(pre=(pk.ctypes.data, None, None)), dict(pre=(pk.ctypes.data, pm.ctypes.data, None)),
               dict(pre=(None, None, pf.ctypes.data))):
        assert call(good, **kw) == (-1, True), kw
    assert call(good, cap=31) == (-4, True)
    with pytest.raises(api.IocError) as e:
        ctx.planes_inserts([rlen], sop, list(b), list(l), cap=31)
    assert e.value.code == -4
