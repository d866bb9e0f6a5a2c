"""ioc_reads_ends: the kernels of ioc_read_ends.hip over host extents, against the host definition segment by segment, as bytes — one
call over the planted segments of ends_common.planted_case with their pairs interleaved (tests/test_reads_ends_host.py measures what
each planted shape is there for), at slack 10, 0, 1 and 32, at max_sites 1, max_variants 2 and min_pct 100, each with and without
pre_group and the row table; a small call after the large one on the same context, random extents, the empty call and the refusals."""
import ctypes as C

import numpy as np
import pytest

from isonclust2_amd import api
from tests import ends_common as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


@pytest.fixture(scope="module")
def planted():
    case = ec.planted_case()
    return case, ec.interleaved(case)


@pytest.mark.parametrize("rule", [{}, dict(slack=0), dict(slack=1), dict(slack=32), dict(max_sites=1), dict(max_variants=2), dict(min_pct=100)],
                         ids=["slack10", "slack0", "slack1", "slack32", "one_site", "two_variants", "pct100"])
def test_planted_segments_interleaved(ctx, planted, rule):
    case, (rlen, sop, ext, pre, mine) = planted
    rule = {**ec.PLANTED, **rule}
    assert sorted({len(e) for _, e, _ in case}) == [0, 1, 3, 6, 64, 65, 130] and sop[:4] == [0, 1, 2, 3]
    want = ec.host_segments(case, **rule)
    got = ctx.reads_ends(rlen, sop, ext, pre_group=pre, **rule)
    ec.same_as_host(got, want, mine)
    lean = ctx.reads_ends(rlen, sop, ext, pre_group=pre, rows=False, **rule)
    assert "rows" not in lean
    ec.same_as_host(lean, want, mine)
    if rule == ec.PLANTED:
        assert tuple(got["seg"][11][["n_starts", "n_starts_found", "n_variants"]]) == (32, 35, 32)
        assert [(int(s["first"]), int(s["end"])) for s in got["starts"][10]] == [(0, 11), (4086, 4106)]
        assert got["variants"][6]["pre_group"].tolist() == [0, 0, ec.TOP - 1, ec.TOP]
    if rule.get("slack") == 1:
        assert [(int(s["first"]), int(s["end"])) for s in got["starts"][10]][-1] == (4095, 4097)
    # the stage on its own: no pre_group
    ec.same_as_host(ctx.reads_ends(rlen, sop, ext, **rule), ec.host_segments(case, with_pre=False, **rule), mine)
    # a small call after the large one on the same context
    small = [c for c in case if c[0] in (64, 2)]
    r2, s2, e2, p2, mine2 = ec.interleaved(small)
    ec.same_as_host(ctx.reads_ends(r2, s2, e2, pre_group=p2, **rule), ec.host_segments(small, **rule), mine2)


def test_random_extents(ctx):
    rng = np.random.default_rng(3)
    case = []
    for rlen, n in ((300, 40), (70, 7), (1000, 133), (5, 3), (4100, 70)):
        e, p = ec.random_extents(rng, n, rlen)
        case.append((rlen, e, p))
    rlen, sop, ext, pre, mine = ec.interleaved(case)
    for rule in (dict(slack=1, min_over=1, min_depth=2, min_alt=2, min_pct=5), dict(slack=31, min_depth=1, min_alt=1, min_pct=1, max_sites=7, max_variants=3),
                 dict(slack=12, min_depth=1, min_alt=1, min_pct=100)):
        ec.same_as_host(ctx.reads_ends(rlen, sop, ext, pre_group=pre, **rule), ec.host_segments(case, **rule), mine)


def test_the_empty_call_and_a_segment_without_pairs(ctx):
    got = ctx.reads_ends([], [], [])
    assert got["starts"] == [] and got["reads"].shape == (0,) and got["seg"].shape == (0,) and got["site_off"].tolist() == [0] and got["var_off"].tolist() == [0]
    got = ctx.reads_ends([30, 0], [], [])
    assert got["site_off"].tolist() == [0] * 5 and got["var_off"].tolist() == [0] * 3 and not got["seg"].tobytes().strip(b"\0")
    assert not got["rows"][0].tobytes().strip(b"\0") and len(got["rows"][0]) == 31


def test_refusals_leave_the_outputs_untouched(ctx):
    rlen, e, p = ec.planted_case()[4]
    e, p = np.ascontiguousarray(e), np.ascontiguousarray(p)
    n = len(e)
    rl, sop = np.array([rlen], np.int32), np.zeros(n, np.int32)
    good = [10, 20, 3, 3, 10, 32, 64]
    sites_bound, var_bound = api.reads_ends_bound(rlen, n)
    assert (sites_bound, var_bound) == (64, 64)
    fill = lambda dt, k: np.frombuffer(bytes([0xA5]) * (dt.itemsize * k), dt).copy()

    def call(rule, n_segs=1, n_pairs=n, sop=sop, ext=e, pre=p, cap=64, vcap=64, soff=True, voff=True, reads=True, seg=True, sites=True, variants=True):
        out = (fill(api.END_ROW_DTYPE, rlen + 1), fill(api.END_SITE_DTYPE, 64), fill(np.dtype(np.int64), 3), fill(api.END_VARIANT_DTYPE, 64), fill(np.dtype(np.int64), 2),
               fill(api.READ_ENDS_DTYPE, n), fill(api.ENDS_SEG_DTYPE, 1))
        before = [o.tobytes() for o in out]
        ptr = lambda o, on=True: o.ctypes.data if on else None
        p64 = lambda o, on: o.ctypes.data_as(C.POINTER(C.c_int64)) if on else None
        rc = ctx.L.ioc_reads_ends(ctx.h, n_segs, rl.ctypes.data_as(C.POINTER(C.c_int32)), n_pairs, sop.ctypes.data_as(C.POINTER(C.c_int32)),
                                  ext.ctypes.data if ext is not None else None, pre.ctypes.data if pre is not None else None, *rule, ptr(out[0]), ptr(out[1], sites),
                                  cap, p64(out[2], soff), ptr(out[3], variants), vcap, p64(out[4], voff), ptr(out[5], reads), ptr(out[6], seg))
        return rc, [o.tobytes() for o in out] == before

    assert call(good) == (0, False) and call(good, pre=None) == (0, False)
    for at, bad in ((0, -1), (0, 33), (1, 0), (2, 0), (3, 0), (4, 0), (4, 101), (5, 0), (5, 33), (6, 0)):
        rule = list(good)
        rule[at] = bad
        assert call(rule) == (-1, True), (at, bad)
    outside, negative, low = sop.copy(), sop.copy(), p.copy()
    outside[7], negative[0], low[5] = 1, -1, -2
    bad_ext = []
    for row in ((-1, 30, 0, 0), (0, rlen + 1, 0, 0), (20, 10, 0, 0), (0, 30, -1, 0), (0, 30, 0, -1)):
        x = e.copy()
        x[3] = row
        bad_ext.append(dict(ext=x))
    for kw in [dict(n_segs=-1), dict(n_pairs=-1), dict(sop=outside), dict(sop=negative), dict(pre=low), dict(ext=None), dict(soff=False), dict(voff=False),
               dict(reads=False), dict(seg=False), dict(sites=False), dict(variants=False), dict(cap=-1), dict(vcap=-1)] + bad_ext:
        assert call(good, **kw) == (-1, True), kw
    assert call(good, cap=63) == (-4, True) and call(good, vcap=63) == (-4, True)
    with pytest.raises(api.IocError) as err:
        ctx.reads_ends([rlen], sop, e, sites_cap=63)
    assert err.value.code == -4
    with pytest.raises(api.IocError) as err:
        ctx.reads_ends([rlen], sop, e, variants_cap=63)
    assert err.value.code == -4
