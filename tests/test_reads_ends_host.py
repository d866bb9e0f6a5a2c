"""ioc_host_reads_ends and ioc_host_ops_extent, the definitions of the ends stage: against py_ends (tests/ends_common.py) on the
planted extents of the GPU test — with what each planted shape is there for — and on random extents, as bytes; the extent of
hand-written and of random operation strings against the block stage's read record and the statistics; the refusals; and the two
property cases through the host aligner."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import api
from tests import ends_common as ec
from tests import iso_polish_common as ipc

RULES = [{}, dict(slack=0), dict(slack=1), dict(slack=32), dict(max_sites=1), dict(max_variants=2), dict(min_pct=100)]


@pytest.fixture(scope="module")
def planted():
    case = ec.planted_case()
    return case, {r: w for (r, _, _), w in zip(case, ec.host_segments(case, **ec.PLANTED))}


def spans(sites):
    return [(int(s["first"]), int(s["end"])) for s in sites]


@pytest.mark.parametrize("rule", RULES, ids=lambda r: "-".join(f"{k}{v}" for k, v in r.items()) or "planted")
def test_the_definition_equals_py_ends_on_the_planted_case(rule):
    rule = {**ec.PLANTED, **rule}
    case = ec.planted_case()
    for (rlen, e, p), w in zip(case, ec.host_segments(case, **rule)):
        ec.same(w, ec.py_ends(e, rlen, p, **{**ec.DEFAULT, **rule}), rlen)
    for (rlen, e, _), w in zip(case, ec.host_segments(case, with_pre=False, **rule)):
        ec.same(w, ec.py_ends(e, rlen, None, **{**ec.DEFAULT, **rule}), rlen)
        lean = api.host_reads_ends(e, rlen, rows=False, **{**ec.DEFAULT, **rule})
        assert "rows" not in lean and lean["reads"].tobytes() == w["reads"].tobytes()


def test_what_the_planted_shapes_are_there_for(planted):
    case, at10 = planted
    by = {r: (e, p) for r, e, p in case}
    run = lambda r, **rule: api.host_reads_ends(by[r][0], r, pre_group=by[r][1], **{**ec.DEFAULT, **ec.PLANTED, **rule})
    # no rows, no pairs, N below min_depth, reads that take no part
    assert int(at10[0]["seg"]["n_reads"]) == 0 and at10[0]["reads"].tolist() == [(-1, -1, -1, 0)]
    assert not at10[65]["seg"].tobytes().strip(b"\0") and len(at10[65]["reads"]) == 0
    assert int(at10[2]["seg"]["n_reads"]) == 2 and len(at10[2]["starts"]) == len(at10[2]["stops"]) == 0 and set(at10[2]["reads"]["start_site"].tolist()) == {-1}
    assert tuple(at10[63]["reads"][33:43]["start_site"]) == (-1,) * 10 and int(at10[63]["seg"]["n_reads"]) == 55
    # a start site that holds row 0 and a stop site that holds row rlen
    assert spans(at10[1]["starts"]) == [(0, 2)] and spans(at10[1]["stops"]) == [(0, 2)] and int(at10[1]["stops"][0]["peak_row"]) == 1
    assert spans(at10[128]["stops"]) == [(118, 129)] and int(at10[128]["stops"][0]["peak_row"]) == 128
    # rows 0-and-2 of step 6: at slack 1 row 21 is the only start row there, its peak has no read, and all three reads land in it
    s1 = run(63, slack=1)
    assert spans(s1["starts"]) == [(0, 2), (21, 22)] and tuple(s1["starts"][1][["n_reads", "peak_row", "peak_reads"]]) == (3, 21, 0)
    assert s1["reads"][30:33]["start_site"].tolist() == [1, 1, 1]
    # windows across 63 | 64 and across 4095 | 4096
    assert spans(run(127, slack=1)["starts"]) == [(0, 2), (63, 65)] and spans(run(127, slack=0)["starts"]) == [(0, 1)]
    assert spans(run(4200, slack=1)["starts"])[-1] == (4095, 4097) and spans(at10[4200]["starts"])[-1] == (4086, 4106)
    # equally far from two sites: the lower; exactly slack and slack + 1 from a site
    w = at10[64]
    assert spans(w["starts"]) == [(0, 16), (35, 56)] and int(w["reads"][10]["start_site"]) == 0
    assert spans(w["stops"]) == [(20, 41), (54, 65)] and w["reads"][11:13]["stop_site"].tolist() == [0, -1]
    assert int(w["reads"][12]["variant"]) == -1 and int(w["seg"]["n_placed"]) == 63
    # 35 start sites found, 32 kept: the reads of the last three have none; max_sites 1
    w = at10[2000]
    assert tuple(w["seg"][["n_starts", "n_starts_found", "n_variants"]]) == (32, 35, 32)
    assert set(w["reads"][96:105]["start_site"].tolist()) == {-1} and w["reads"][93:96]["start_site"].tolist() == [31] * 3
    assert tuple(run(2000, max_sites=1)["seg"][["n_starts", "n_starts_found", "n_placed"]]) == (1, 35, 3)
    assert tuple(run(2000, slack=32)["seg"][["n_starts", "n_starts_found"]]) == (1, 1)   # ends closer than 2 slack: one site
    # min_pct 100: a site only where every read starts within slack of the row
    assert spans(run(128, min_pct=100)["starts"]) == [(0, 11)] and len(run(129, min_pct=100)["starts"]) == 0 and len(run(129, min_pct=100)["stops"]) == 1
    # pre_group -1 is never placed, 2^31 - 1 is the last variant
    w = at10[127]
    assert w["variants"]["pre_group"].tolist() == [0, 0, ec.TOP - 1, ec.TOP] and w["variants"]["n_reads"].tolist() == [20, 4, 3, 20]
    assert set(w["reads"][44:61]["variant"].tolist()) == {-1} and int(w["seg"]["n_placed"]) == 47
    # pre_group is the major word of the order; two placed reads of pre_group 2 are unsupported; max_variants cuts the list
    w = at10[129]
    assert [tuple(v)[:3] for v in w["variants"].tolist()] == [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0)]
    assert w["reads"][128:]["variant"].tolist() == [-1, -1] and int(w["seg"]["n_placed"]) == 130
    cut = run(129, max_variants=2)
    assert tuple(cut["seg"][["n_variants", "n_variants_found"]]) == (2, 4) and set(cut["reads"][70:128]["variant"].tolist()) == {1, -1}
    # head / tail at min_over - 1 and at min_over
    assert tuple(at10[128]["starts"][0][["n_reads", "n_over"]]) == (65, 10) and tuple(at10[128]["stops"][0][["n_reads", "n_over"]]) == (65, 7)


def test_random_extents():
    rng = np.random.default_rng(1)
    for t in range(80):
        rlen, n = int(rng.integers(0, 400)), int(rng.integers(0, 90))
        e, p = ec.random_extents(rng, n, rlen)
        rule = dict(slack=int(rng.integers(0, 33)), min_over=int(rng.choice([1, 20, 21])), min_depth=int(rng.integers(1, 5)), min_alt=int(rng.integers(1, 4)),
                    min_pct=int(rng.choice([1, 10, 50, 100])), max_sites=int(rng.choice([1, 3, 32])), max_variants=int(rng.choice([1, 2, 64])))
        ec.same(api.host_reads_ends(e, rlen, pre_group=p, **rule), ec.py_ends(e, rlen, p, **rule), (t, rule))


def test_the_extent_of_hand_strings():
    ext = lambda ops, rlen: tuple(api.host_ops_extent(ops, rlen))
    assert ext(b"", 0) == (0, 0, 0, 0)
    assert ext(b"iiiddd", 3) == (0, 0, 3, 0)            # no walk byte: all leading, nothing covered
    assert ext(b"iiI==D=ii", 4) == (0, 4, 2, 2)         # a walk that begins with 'I': the row behind it is the first
    assert ext(b"ddiDD==Iidd", 8) == (2, 6, 1, 1)       # ... with 'D': a deleted row is covered; 'd' rows are not
    assert ext(b"dd=d", 4) == (2, 3, 0, 0)
    for ops, rlen in ((b"==", 3), (b"=Y", 2), (b"=\0", 2)):
        with pytest.raises(ValueError):
            api.host_ops_extent(ops, rlen)


def test_the_extent_of_random_strings_is_the_block_record_and_the_statistics():
    rng = random.Random(0)
    for _ in range(200):
        walk = "".join(rng.choice("==XID") for _ in range(rng.randrange(0, 60)))
        lead = "i" * rng.randrange(0, 4) + "d" * rng.randrange(0, 4)
        trail = "i" * rng.randrange(0, 4) + "d" * rng.randrange(0, 4)
        ops = (lead + walk + trail).encode()
        rlen, qlen = sum(c in b"=XDd" for c in ops), sum(c in b"=XIi" for c in ops)
        query = bytes(rng.choice(b"ACGTN") for _ in range(qlen))
        base = api.ops_project(ops, query, rlen)[0]
        rec, st, e = api.planes_blocks(base[None, :])["reads"][0], api.ops_stats(ops), api.host_ops_extent(ops, rlen)
        assert tuple(e) == (int(rec["first_row"]), int(rec["end_row"]), st["lead_i"], st["trail_i"]), ops


def test_refusals_leave_the_outputs_untouched():
    L = api._lib.load()
    e = ec.extents([(0, 30, 1, 2)] * 5)
    pre = np.zeros(5, np.int32)
    good = [10, 20, 3, 3, 10, 32, 64]
    fill = lambda dt, k: np.frombuffer(bytes([0xA5]) * (dt.itemsize * k), dt).copy()

    def call(rule, ext=e, pre=pre, n=5, rlen=30, drop=()):
        out = [fill(api.END_ROW_DTYPE, 31), fill(api.END_SITE_DTYPE, 31), fill(api.END_SITE_DTYPE, 31), fill(api.END_VARIANT_DTYPE, 5), fill(api.READ_ENDS_DTYPE, 5),
               fill(api.ENDS_SEG_DTYPE, 1)]
        before = [o.tobytes() for o in out]
        rc = L.ioc_host_reads_ends(ext.ctypes.data if ext is not None else None, pre.ctypes.data if pre is not None else None, n, rlen, *rule,
                                   *(None if x in drop else o.ctypes.data for x, o in enumerate(out)))
        return rc, [o.tobytes() for o in out] == before

    assert call(good) == (0, False) and call(good, pre=None) == (0, False) and call(good, drop=(0,))[0] == 0
    for at, bad in ((0, -1), (0, 33), (1, 0), (2, 0), (3, 0), (4, 0), (4, 101), (5, 0), (5, 33), (6, 0)):
        rule = list(good)
        rule[at] = bad
        assert call(rule) == (-1, True), (at, bad)
    for row in ((-1, 30, 0, 0), (0, 31, 0, 0), (20, 10, 0, 0), (0, 30, -1, 0), (0, 30, 0, -1)):
        bad = e.copy()
        bad[3] = row
        assert call(good, ext=bad) == (-1, True), row
    low = pre.copy()
    low[2] = -2
    for kw in (dict(pre=low), dict(n=-1), dict(rlen=-1), dict(ext=None), dict(drop=(1,)), dict(drop=(2,)), dict(drop=(3,)), dict(drop=(4,)), dict(drop=(5,))):
        assert call(good, **kw) == (-1, True), kw
    x = api._lib.ReadExtent(7, 7, 7, 7)
    assert L.ioc_host_ops_extent(b"==", 2, 3, C.byref(x)) == -1 and L.ioc_host_ops_extent(b"==", -1, 2, C.byref(x)) == -1 and x.first_row == 7
    assert L.ioc_host_ops_extent(b"==", 2, 2, None) == -1


# ---- the property cases, seed 0, measured on the host aligner and pinned ----
def holding(sites, row):
    return [b for b, s in enumerate(sites) if int(s["first"]) <= row < int(s["end"])]


def test_property_case_a():
    """Measured at seed 0 (profiles/read_ends.txt): start sites [0, 11) with 80 reads, 78 of them at row 0, and [240, 261) with 41, 39
    at row 250; stop sites [1190, 1211) with 40 reads and [1490, 1501) with 92; the three variants carry 40 + 40 + 41 reads, none of
    a whole class lands in another class's site, and no whole read is unplaced; of the 12 reads that start anywhere, one starts
    inside the site at row 250 and joins that variant, the other 11 have no start site: 121 of 132 reads are placed."""
    frame, reads, ops, ext = ec.property_case("A")
    got = api.host_reads_ends(ext, len(frame))
    ec.same(got, ec.py_ends(ext, len(frame)))
    assert len(got["starts"]) == 2 == int(got["seg"]["n_starts_found"]) and [holding(got["starts"], r) for r in ec.STARTS_A] == [[0], [1]]
    assert len(got["stops"]) == 2 == int(got["seg"]["n_stops_found"]) and [holding(got["stops"], r) for r in ec.STOPS_A] == [[0], [1]]
    assert [tuple(v)[:3] for v in got["variants"].tolist()] == [(0, 0, 0), (0, 0, 1), (0, 1, 1)]
    true = [(0, 1)] * ec.CLASS + [(0, 0)] * ec.CLASS + [(1, 1)] * ec.CLASS   # (start site, stop site) of the whole classes
    mine = [(int(r["start_site"]), int(r["stop_site"])) for r in got["reads"][:3 * ec.CLASS]]
    wrong = sum(m != t and -1 not in m for m, t in zip(mine, true))
    unplaced = sum(-1 in m for m in mine)
    print("case A: starts", [tuple(s) for s in got["starts"].tolist()], "stops", [tuple(s) for s in got["stops"].tolist()], "variants", got["variants"].tolist(),
          "wrong", wrong, "unplaced whole reads", unplaced, "seg", got["seg"])
    assert wrong == 0
    assert unplaced == 0 and got["variants"]["n_reads"].tolist() == [40, 40, 41] and int(got["seg"]["n_placed"]) == 121   # (recorded, no condition)
    # every variant's consensus from its own reads: rows below min_depth keep the representative's base, so nothing is trimmed
    for v in range(3):
        cols, ins = None, None
        for i in np.flatnonzero(got["reads"]["variant"] == v):
            cols, ins = api.planes_pile(api.ops_project(ops[i], reads[i], len(frame))[0], api.ops_project_ins(ops[i], reads[i], len(frame)), cols, ins)
        seq, _, _ = api.pileup_call(cols, ins, frame, min_depth=3)
        assert ipc.edit_distance(seq, frame) == 0, v


def test_property_case_b():
    """The same reads against R[100:]: most reads carry 100 bases in front of the representative's row 0.  Measured at seed 0: the
    start site at row 0 has 82 reads — the 80 whole reads that reach it and two of those that start anywhere, before R[100] — and
    all 82 have a head of at least min_over."""
    frame, _, _, ext = ec.property_case("B")
    got = api.host_reads_ends(ext, len(frame))
    at0 = got["starts"][holding(got["starts"], 0)[0]]
    print("case B: starts", [tuple(s) for s in got["starts"].tolist()], "stops", [tuple(s) for s in got["stops"].tolist()], "variants", got["variants"].tolist())
    assert 2 * int(at0["n_over"]) > int(at0["n_reads"])
    assert tuple(at0[["n_reads", "n_over"]]) == (82, 82)   # (recorded)
