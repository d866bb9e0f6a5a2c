"""What ioc_resolve returns besides the assignments — the cuts (ioc_get_cuts), the tie sets (ioc_get_ties) and the flag byte of
ioc_get_decisions — against the sequential restatement of the greedy loop (tests/resolve_common.greedy_resolve, itself checked
against the oracle in tests/test_resolve_host.py).  Integers throughout, no tolerance; tie keys are unordered, and where the
order-dependent tie (bit 0) is flagged the decision is one of the passing candidates of the winning Size.

The crafted inputs go through queries_upload / left_load directly and are resolved through the staged calls with sahlin-mode
parameters (no list is cut by `need`, no alignment is started); whether a candidate passes depends on `need` alone (0: every
candidate, 1 << 30: none), so the reference owes nothing to the device.  Every test first asserts, from the restatement, that
its inputs reach the kernel path it is named for: the 8 x 256 candidates k_decide_scan holds in registers, the 32 walk slots,
the 16 tie slots, the 256 staged evaluations."""
import functools

import numpy as np
import pytest

from isonclust2_amd import api, synth
from tests import resolve_common as rc
from tests import structured_reads as sr
from tests.helpers import oracle_sorted_batch

pytestmark = pytest.mark.gpu

UNEVALUATED, REJECTED = 0xFFFFFFFF, 0xFFFFFFFE


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def sahlin(min_shared=5, min_fraction=0.8):
    p = api.default_params(rc.K, 15, "sahlin")
    p.min_shared, p.min_fraction = min_shared, min_fraction
    return p


@functools.lru_cache(maxsize=None)
def crafted(name):
    """a crafted case, its upload arrays and its left MinDB (shared by the tests of this module; read only)"""
    case = {"pool": rc.pool_case, "edges": rc.edges_case, "mixed": rc.mixed_case}[name]()
    left = rc.left_csr(case["left_sets"]) if case["L"] else None
    return case, rc.records(case["fwd"], case["rev"]), left


@functools.lru_cache(maxsize=None)
def mixed_restated(min_shared, min_fraction):
    return rc.restate(crafted("mixed")[0], min_shared, min_fraction)


def stage(ctx, name, p, need=None):
    """upload, left state, index, scores, forced decisions and verdicts of a crafted case: everything up to ioc_resolve"""
    case, rec, left = crafted(name)
    ctx.set_params(p)
    ctx.queries_upload(rec["off_fwd"], rec["off_rev"], rec["min_val"], rec["min_pos"], rec["hpc_len"], rec["err_cell"],
                       case["need"] if need is None else need)
    if left is None:
        ctx.left_load(0, None, None, None, None)
    else:
        ctx.left_load(case["L"], (1 + np.arange(case["L"]) % 15).astype(np.uint8), *left)
    ctx.index_build()
    ctx.score()
    for j, f in case.get("forced", {}).items():
        if isinstance(f, tuple):
            ctx.force_decision(j, f[0], f[1])
        else:
            ctx.force_decision(j, f)
    n = case["n"]
    ctx.set_aln_verdicts(case.get("verdict_t", np.full(n, rc.NO_VERDICT, np.int32)), case.get("verdict_s", np.zeros(n, np.int8)))
    return case


def outputs(ctx):
    ctx.resolve()
    return ctx.decisions(), ctx.cuts(), ctx.ties()


def test_bindings_and_constants(ctx):
    assert api.TIE_SLOTS == rc.TIE_SLOTS == 16 and api.CUT_NONE == rc.INT32_MAX and api.NO_VERDICT == rc.NO_VERDICT
    case = stage(ctx, "edges", sahlin())
    ctx.set_aln_verdicts(None)                          # verdicts off: no tie sets
    ctx.resolve()
    assert ctx.cuts().dtype == np.int32 and ctx.cuts().shape == (case["n"],)
    with pytest.raises(api.IocError):
        ctx.ties()
    ctx.force_decision(3, -1)
    ctx.resolve()
    assert ctx.decisions()[0][3] == -1 and ctx.cuts()[3] == api.CUT_NONE
    ctx.clear_forced()
    ctx.resolve()
    assert ctx.decisions()[0][3] >= 0 and ctx.cuts()[3] == 8


def test_over_2048_candidates_long_ties_and_walk_overflow(ctx):
    """1100 queries over a pool of 12 values, nothing passes: every query opens a cluster and is a candidate of every later
    one.  Reached: lists beyond the 2048 register slots whose top Size lies only behind them, tie sets of hundreds, walks and
    unevaluated items far beyond their slots."""
    case = crafted("pool")[0]
    R = rc.restate(case)
    pc = rc.path_counts(R)
    n = case["n"]
    late = np.flatnonzero(R.n_cand > rc.SCAN_REGS)
    assert pc["max_cand"] == 2 * (n - 1) > rc.SCAN_REGS and len(late) >= 50
    assert np.array_equal(R.n_cand, 2 * np.arange(n))                       # every pair is in the lists: entry = 2t + s or s * j + t
    tail_only = [j for j in late if all(k >= rc.SCAN_REGS and (k & 1) * j + (k >> 1) >= rc.SCAN_REGS for k in R.ties[j])]
    assert len(tail_only) >= 20
    assert int((R.n_ties[late] >= 300).sum()) >= 20 and pc["max_ties"] >= 800
    assert pc["walk_over_slots"] >= 1000 and pc["items_over_stage"] >= 900 and pc["max_walk"] > 2000
    assert R.flags[0] == 0 and set(R.flags[1:].tolist()) == {2} and set(R.target.tolist()) == {-1}
    stage(ctx, "pool", sahlin())
    dec, cuts, ties = outputs(ctx)
    assert dec[2][0] == 0 and np.all(dec[2][1:] == 2)                       # (query 0 has no candidate at all)
    rc.compare(R, dec, cuts, ties)


@pytest.mark.parametrize("need", [rc.NEED_ALL, rc.NEED_NONE])
def test_edges_of_the_slots(ctx, need):
    """300 left clusters; per query exactly 1, 15, 16, 17, 31, 32, 33, 255, 256, 257 and 300 candidates tied at the top, and
    one query with reverse-strand candidates only.  need 0: every tied candidate passes (bit 0, the staged-items edge at 256);
    need large: none does (bit 1)."""
    case = crafted("edges")[0]
    nd = np.full(case["n"], need, np.uint32)
    R = rc.restate(case, need=nd)
    want = list(rc.EDGE_TIES) + [5]
    assert R.n_ties.tolist() == want and R.walk.tolist() == want and R.items.tolist() == want
    assert {c - s for c in want for s in (rc.TIE_SLOTS, rc.WALK_SLOTS, rc.SCAN_ITEMS)} >= {-1, 0, 1}
    assert all(k & 1 for k in R.ties[-1]) and not any(k & 1 for t in R.ties[:-1] for k in t)
    assert np.all(R.n_cand >= 300) and set(R.cut.tolist()) == {8}
    if need == rc.NEED_ALL:
        assert R.flags.tolist() == [0] + [1] * (len(want) - 1) and R.strand[-1] == -1
    else:
        assert set(R.flags.tolist()) == {2}
    stage(ctx, "edges", sahlin(), need=nd)
    rc.compare(R, *outputs(ctx))


def _float_parts(R, f):
    w = np.flatnonzero(R.cut != rc.INT32_MAX)
    return (sum(rc.cut_of_f32(int(R.top[j]), f) != R.cut[j] for j in w),
            sum(int(float(R.top[j]) * float(np.float32(f))) != R.cut[j] for j in w))


@pytest.mark.parametrize("min_shared,min_fraction", rc.MIXED_PARAMS)
def test_mixed_with_left_clusters(ctx, min_shared, min_fraction):
    """400 queries against 50 left clusters, pools of 6, 12 and 40 values, need drawn per query, forced decisions and verdicts:
    which targets are clusters depends on the earlier decisions."""
    case = crafted("mixed")[0]
    R = mixed_restated(min_shared, min_fraction)
    pc = rc.path_counts(R)
    forced = case["forced"]
    assert {(-3 if isinstance(f, tuple) else f) for f in forced.values()} == {-1, -2, -3} and len(forced) >= 10
    assert pc["walks"] >= 80 and pc["flag2"] >= 40
    taken = np.flatnonzero((R.flags == 2) & (case["verdict_t"] != rc.NO_VERDICT))
    assert (case["verdict_t"][taken] >= 0).sum() >= 5 and (case["verdict_t"][taken] < 0).sum() >= 5
    # a -2 entry is never a cluster; queries that opened one do show up in later tie sets
    gated = {case["L"] + j for j, f in forced.items() if f == -2}
    assert not any((k >> 1) in gated for t in R.ties for k in t)
    assert sum(any((k >> 1) >= case["L"] for k in t) for t in R.ties) >= 5
    if (min_shared, min_fraction) == (5, 0.8):
        assert pc["walk_over_slots"] >= 10 and pc["ties_over_slots"] >= 3 and pc["flag1"] >= 50
    if (min_shared, min_fraction) == (5, 0.7):
        assert _float_parts(R, min_fraction)[0] >= 2 and _float_parts(R, min_fraction)[1] >= 1      # tops 90 and 170; top 10
    if min_fraction > 1:
        assert pc["max_items"] == 0 and pc["flag2"] == pc["walks"] and np.all(R.cut[R.top > 0] > R.top[R.top > 0])
    if min_shared == 0:
        assert int(((R.top > 0) & (R.top < 5)).sum()) >= 10                   # walks a MinShared of 5 would not start
    if min_fraction == 0.0:
        assert set(R.cut[R.top > 0].tolist()) == {0} and pc["walk_over_slots"] >= 300
    stage(ctx, "mixed", sahlin(min_shared, min_fraction))
    rc.compare(R, *outputs(ctx))


@pytest.mark.parametrize("env", ["IOC_RESOLVE_LAZY=0", "IOC_RESOLVE_SKIP_P1=0", "IOC_QUEUE_CAP=64", "IOC_RESOLVE_BOUND=0"])
def test_same_outputs_on_every_route(ctx, monkeypatch, env):
    """The mixed case without the lazy sweeps, with the first half of the first exact sweep, with a work queue that overflows
    and without the upper bound of totalMapped."""
    name, value = env.split("=")
    monkeypatch.setenv(name, value)
    R = mixed_restated(5, 0.8)
    if name == "IOC_QUEUE_CAP":
        assert int(R.items.sum()) > 4 * int(value) and int(R.items.max()) > int(value)
    stage(ctx, "mixed", sahlin())
    rc.compare(R, *outputs(ctx))


def _keys(ties, upto):
    """the tie sets as sorted lists; of a set beyond the slots any 16 members are reported (compare() checks them): None"""
    count, keys = ties
    return [sorted(keys[j, :int(count[j])].tolist()) if count[j] <= rc.TIE_SLOTS else None for j in range(upto)]


def test_warm_restart_after_changed_verdicts(ctx, monkeypatch):
    """resolve, change the verdicts of a few queries of the second half, resolve again: the restatement of the new verdicts, the
    same as the sequence without the warm restart, and cuts and ties in front of the first change as they were."""
    case = crafted("mixed")[0]
    n, L = case["n"], case["L"]
    R0 = mixed_restated(5, 0.8)
    use = np.flatnonzero((R0.flags == 2) & (np.arange(n) >= n // 2))
    change = use[::max(1, len(use) // 5)][:5]
    assert len(change) >= 3 and change[0] >= n // 2
    vt, vs = case["verdict_t"].copy(), case["verdict_s"].copy()
    for j in change.tolist():
        if vt[j] >= 0 or vt[j] == rc.NO_VERDICT:
            vt[j], vs[j] = -1, 0
        else:
            vt[j], vs[j] = j % L, -1
    R1 = rc.restate(case, verdict_t=vt, verdict_s=vs)
    first = int(change[0])
    assert not np.array_equal(R1.target, R0.target)                      # the change is seen, and by later queries too
    assert any(R1.ties[j] != R0.ties[j] for j in range(first + 1, n))
    runs = {}
    for warm in ("1", "0"):
        monkeypatch.setenv("IOC_RESOLVE_WARM", warm)
        stage(ctx, "mixed", sahlin())
        before = outputs(ctx)
        rc.compare(R0, *before)
        ctx.set_aln_verdicts(vt, vs)
        after = outputs(ctx)
        rc.compare(R1, *after)
        assert np.array_equal(after[1][:first], before[1][:first])
        assert np.array_equal(after[2][0][:first], before[2][0][:first]) and _keys(after[2], first) == _keys(before[2], first)
        runs[warm] = after
    a, b = runs["1"], runs["0"]
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2][0], b[2][0]) and _keys(a[2], n) == _keys(b[2], n)


@pytest.mark.parametrize("name", ["short_dup", "family_ties"])
def test_real_reads(ctx, name):
    """Real minimizer lists (short_dup; the structured set family_ties), staged with sahlin parameters, the true `need` and no
    verdict.  Here `passes` is read from the device's own candidate tables (ctx.query_candidates under the final decisions: a
    total that was evaluated, not rejected, and reaches `need`) — those tables are pinned to the oracle elsewhere
    (helpers.compare_candidate_tables) and serve here as the reference for k_decide_pick only: given the totals, the pick, the
    flags, the cuts and the tie sets.  On top of the comparison: every cluster candidate in reach of the walk and above the
    winner's Size (all of the walk where nothing passes) carries an evaluated and failing total or a rejection."""
    rs = synth.generate_config("short_dup", seed=1) if name == "short_dup" else sr.case(name)
    _, view = oracle_sorted_batch(rs)
    p = sahlin()
    n = len(view["hpc_len"])
    ctx.set_params(p)
    cell = np.array([api.host_err_cell(e) for e in view["hpc_err"]], np.uint8)
    need = np.array([api.host_min_total(int(h), p.mapped_threshold) for h in view["hpc_len"]], np.uint32)
    ctx.queries_upload(view["off_fwd"], view["off_rev"], view["min_val"], view["min_pos"], view["hpc_len"], cell, need)
    ctx.left_load(0, None, None, None, None)
    ctx.index_build()
    ctx.score()
    ctx.set_aln_verdicts(np.full(n, rc.NO_VERDICT, np.int32), np.zeros(n, np.int8))
    dec, cuts, ties = outputs(ctx)
    tables = {}

    def table(q):
        if q not in tables:
            t, s, sz, _, tm = ctx.query_candidates(q, 2 * n + 2)
            tables[q] = {(int(a), int(b)): (int(z), int(x)) for a, b, z, x in zip(t, s, sz, tm)}
        return tables[q]

    def passes(q, t, s, z):
        tm = table(q).get((t, s), (0, UNEVALUATED))[1]
        return tm not in (UNEVALUATED, REJECTED) and tm >= need[q]

    fwd, rev = rc.lists_of_view(view)
    R = rc.greedy_resolve(n, 0, fwd, rev, [], need, p.min_shared, p.min_fraction, passes=passes, tables=True)
    pc = rc.path_counts(R)
    assert pc["walks"] >= n // 4 and pc["flag1"] >= 3, pc
    if name == "family_ties":
        assert pc["walk_over_slots"] >= 10 and pc["ties_over_slots"] >= 1, pc
    rc.compare(R, dec, cuts, ties)
    checked = 0
    for j in np.flatnonzero(R.cut != rc.INT32_MAX).tolist():
        tab = table(j)
        t, s, z = R.cands[j]
        assert sorted(tab) == sorted(zip(t.tolist(), s.tolist())) and all(tab[(a, b)][0] == c for a, b, c in zip(t.tolist(), s.tolist(), z.tolist())), j
        floor = min(int(R.cut[j]), int(R.top[j])) if R.flags[j] & 2 else max(int(R.cut[j]), int(R.win_size[j]) + 1)
        for (a, b), (size, tm) in tab.items():
            if size >= floor:
                assert tm == REJECTED or (tm != UNEVALUATED and tm < need[j]), (j, a, b, size, tm, int(need[j]))
                checked += 1
    assert checked >= 20
