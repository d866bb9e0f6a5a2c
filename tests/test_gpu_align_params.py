"""The batched GPU aligner at scoring parameters other than 2 / -2 / 1 (tests/align_params_common.py has the sets and why each is
there; tests/test_align_params_host.py pins the host aligner, the definition, at the same sets).  For every pair of every case:
the operation string of ioc_align_pairs_ops is ioc_host_align_ops' byte for byte, score / windows / ratio are the host's and the
plain ioc_align_pairs' in the same context, and the string passes check_ops.  Integers and bytes, no tolerance.

Every test says which kernel family it means to reach — the comparing kernel, the query-profile kernel with 32-bit cells, version
2 (ioc_host_align_route decides, by parameters and the pair's gap_open) — and asserts that it did: the routes its pairs take by
the rule, and ioc_timings' align_version / n_align_refused / align_slices / n_align_cells_computed of the run."""
import ctypes as C

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests.align_ops_checks import check_ops, revcomp
from tests.align_params_common import DEFAULT, PARAM_IDS, PARAM_SETS, ROUTE_COMPARE, ROUTE_PROFILE, ROUTE_V2, route
from tests.polish_common import gap_open
from tests.test_gpu_align import tile_sequences, verdict_pairs
from tests.test_gpu_align_ops import _long_pairs, _route_pairs, _small_pairs
from tests.test_gpu_align_polish import _segments

pytestmark = pytest.mark.gpu

_host_cache = {}


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _host_ops(q, r, rc, go, p):
    """(operation string, score) of ioc_host_align_ops, cached per (query, reference, revcomp, gap_open, parameter set)."""
    key = (q, r, bool(rc), go, p)
    if key not in _host_cache:
        _host_cache[key] = api.host_align_ops(q, revcomp(r) if rc else r, match=p[0], mismatch=p[1], gap_open=go, gap_extend=p[2])
    return _host_cache[key]


def _routes(seqs, pairs, p):
    """The kernel families the pairs take by the rule, those with an empty sequence (answered without a kernel) left out."""
    assert all(set(s) <= set(b"ACGT") for s in seqs)  # (another letter would send its pairs to the comparing kernel whatever the rule)
    return {route(p, gap_open(pr[3])) for pr in pairs if len(seqs[pr[0]]) and len(seqs[pr[1]])}


def _check(ctx, seqs, pairs, k, p, plain=None, set_pool=True):
    """One emitting call against the host aligner, a plain ioc_align_pairs (`plain`: its result, taken here if None) and the
    string's own invariants.  Returns (score, windows, ratio, ops, align_version of the emitting call, pairs it had refused)."""
    if set_pool:
        ctx.align_set_pool(seqs)
    refused = ctx.timings()["n_align_refused"]
    score, win, ratio, ops = ctx.align_pairs_ops(pairs, k, *p)
    tm = ctx.timings()
    if plain is None:
        plain = ctx.align_pairs(pairs, k, *p)
    assert np.array_equal(score, plain[0]) and np.array_equal(win, plain[1]) and np.array_equal(ratio, plain[2])
    L = _lib.load()
    for i, pr in enumerate(pairs):
        qi, ri, rcomp, e = pr[:4]
        q, r, go = seqs[qi], seqs[ri], gap_open(e)
        tag = (i, len(q), len(r), rcomp, e, p)
        hops, hscore = _host_ops(q, r, rcomp, go, p)
        if ops[i] != hops:
            d = next((x for x in range(min(len(hops), len(ops[i]))) if hops[x] != ops[i][x]), min(len(hops), len(ops[i])))
            raise AssertionError(f"pair {tag}: device string (len {len(ops[i])}, score {score[i]}) leaves the host's (len {len(hops)}, score "
                                 f"{hscore}) at column {d}: {ops[i][max(0, d - 10):d + 10]!r} / {hops[max(0, d - 10):d + 10]!r}")
        assert score[i] == hscore, tag
        check_ops(ops[i], q, revcomp(r) if rcomp else r, int(score[i]), go, match=p[0], mismatch=p[1], gap_extend=p[2], tag=tag, any_gap_costs=True)
        comp = api.ops_to_comp(ops[i])
        assert win[i] == round(L.ioc_host_aln_ratio(comp, len(comp), e, 1, k)), tag            # (slen 1: the count itself)
        assert ratio[i] == (L.ioc_host_aln_ratio(comp, len(comp), e, len(q), k) if len(q) else 0.0), tag
    return score, win, ratio, ops, tm["align_version"], tm["n_align_refused"] - refused


def _version_for(routes_):
    """align_version of a run whose pairs take these families: version 1 runs last whenever a pair is not version 2's."""
    return 2 if routes_ == {ROUTE_V2} else 1


@pytest.mark.parametrize("p", PARAM_SETS, ids=PARAM_IDS)
def test_small_pairs(ctx, p):
    """Lengths 0 .. 200, empty and one-base sequences, two-letter and identical sequences, every gap-open class — so every
    family the rule gives the set in one call, a couple of version 2 with two different gd among them."""
    seqs, pairs = _small_pairs(13, 60)
    assert {gap_open(pr[3]) for pr in pairs} == {2, 3, 4, 5}
    want = {route(p, go) for go in (2, 3, 4, 5)}
    assert _routes(seqs, pairs, p) == want
    for k in (1, 11, 32) if p in ((1, -1, 1), (2, -2, 3)) else (11,):
        got = _check(ctx, seqs, pairs, k, p)
        assert got[4] == _version_for(want) and got[5] == 0, (got[4], got[5], want)
    if want != {ROUTE_V2} and ROUTE_V2 in want:
        # the pairs the rule gives version 2, alone: version 2 did take them (and none came back refused)
        sub = [pr for pr in pairs if route(p, gap_open(pr[3])) == ROUTE_V2]
        got = _check(ctx, seqs, sub, 11, p, set_pool=False)
        assert got[4] == 2 and got[5] == 0


def _tile_pairs():
    """test_tile_boundaries' sequences at the lengths where a rebase group (64 rows), a checkpoint pitch (256 / 512) and a strip
    (1024 columns) end, each paired with itself, its successor and the one five on; e cycles through the four gap-open classes."""
    lens = [255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1537, 2049]
    seqs = tile_sequences(lens)[0][:len(lens)]
    es = (0.0, 0.02, 0.05, 0.3)
    pairs = []
    for a in range(len(lens)):
        for b in (a, (a + 1) % len(lens), (a + 5) % len(lens)):
            pairs.append((a, b, (a + b) % 2, es[len(pairs) % 4]))
    return seqs, pairs


@pytest.mark.parametrize("p", PARAM_SETS, ids=PARAM_IDS)
def test_tile_edges(ctx, p):
    """All four gap-open classes, and with them both sides of the set's cx / cm / gd boundaries, in one call."""
    seqs, pairs = _tile_pairs()
    assert [gap_open(e) for e in (0.0, 0.02, 0.05, 0.3)] == [5, 4, 3, 2]
    want = {route(p, go) for go in (2, 3, 4, 5)}
    assert _routes(seqs, pairs, p) == want
    got = _check(ctx, seqs, pairs, 11, p)
    assert got[4] == _version_for(want), (got[4], want)
    if want == {ROUTE_V2}:
        # 16-bit halves: a pair may leave the window and come back through version 1 (still the host's bytes, above) — but a set
        # that loses most of its pairs that way no longer tests version 2
        assert got[5] <= len(pairs) // 4, got[5]


ROUTE_ENVS = [{"IOC_ALIGN_V1": "1"}, {"IOC_ALIGN_ARENA": "fat"}, {"IOC_ALIGN_VARIANT": "carry"}, {"IOC_ALIGN_CORRIDOR": "0"},
              {"IOC_ALIGN_NO_PROFILE": "1"}, {"IOC_ALIGN_FORCE_CROSS": "1"}, {}]
# the routes set has gap_open 2 throughout (e 0.12 .. 0.3): one family per parameter set
ROUTE_SETS = {(1, -1, 1): ROUTE_V2, (5, -4, 2): ROUTE_V2, (2, -6, 1): ROUTE_COMPARE, (250, -2, 1): ROUTE_PROFILE, (2, -2, 3): ROUTE_PROFILE}


@pytest.mark.parametrize("p", list(ROUTE_SETS), ids=["%d_%d_%d" % p for p in ROUTE_SETS])
@pytest.mark.parametrize("env", ROUTE_ENVS, ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_every_route(ctx, monkeypatch, env, p):
    """The switches test_gpu_align_ops.py chooses its routes with, at parameters of every family (2.6 kb family, an unrelated
    pair, a 4.6 kb pair, a repeat, an empty sequence).  Under IOC_ALIGN_VARIANT=carry the plain call runs the carry kernel and
    the emitting call the traced one: two formulations agree."""
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    seqs, pairs = _route_pairs()
    assert _routes(seqs, pairs, p) == {ROUTE_SETS[p]}
    got = _check(ctx, seqs, pairs, 11, p)
    v1_forced = "IOC_ALIGN_V1" in env or "IOC_ALIGN_ARENA" in env or "IOC_ALIGN_NO_PROFILE" in env
    assert got[4] == (1 if v1_forced or ROUTE_SETS[p] != ROUTE_V2 else 2), got[4]
    if ROUTE_SETS[p] != ROUTE_V2 or v1_forced:
        assert got[5] == 0          # (nothing passes through version 2, so nothing comes back from it)


def test_long_pairs_corridor_and_its_fit_between_parameter_sets(ctx, monkeypatch):
    """9 kb pairs, the only size with a corridor, its certificate and the probe launch: (1, -1, 1) and (5, -4, 2), all version 2's.
    Every tile (IOC_ALIGN_CORRIDOR=0), the default corridor, and the default corridor once more — the call before has fed the
    learned width model at these parameters — return the host's strings.  2 / -2 / 1 runs between the two sets: the model is
    per parameter signature and must not leak (ioc_ctx::aln_fit_sig).  Ten related pairs and two unrelated ones; the host side
    is most of the test's time (0.2 - 0.3 s a pair and set)."""
    seqs, pairs = _long_pairs()
    ctx.align_set_pool(seqs)

    def computed(fn):
        before = ctx.timings()["n_align_cells_computed"]
        out = fn()
        return out, ctx.timings()["n_align_cells_computed"] - before

    for p in ((1, -1, 1), DEFAULT, (5, -4, 2)):
        assert _routes(seqs, pairs, p) == {ROUTE_V2}
        monkeypatch.setenv("IOC_ALIGN_CORRIDOR", "0")
        ref, every_tile = computed(lambda: _check(ctx, seqs, pairs, 11, p, set_pool=False))
        assert ref[4] == 2 and ref[5] <= len(pairs) // 4, (p, ref[4], ref[5])
        monkeypatch.delenv("IOC_ALIGN_CORRIDOR")
        for turn in range(2):
            got, done = computed(lambda: _check(ctx, seqs, pairs, 11, p, plain=ref[:3], set_pool=False))
            assert got[3] == ref[3] and got[4] == 2 and got[5] <= len(pairs) // 4, (p, turn, got[4], got[5])
            assert done < every_tile, (p, turn, done, every_tile)  # (tiles were left out: there was a corridor)


@pytest.mark.parametrize("p", [(1, -1, 1), (5, -4, 2)], ids=["1_-1_1", "5_-4_2"])
def test_verdict_mode(ctx, p):
    """test_verdict_mode_decides_every_comparison_like_the_full_count's pairs: scores exact, every `ratio >= threshold` as with
    the full count, never more windows than it — and walks did stop early.  gap_open 2 throughout: version 2."""
    seqs, pairs = verdict_pairs()
    assert _routes(seqs, pairs, p) == {ROUTE_V2}
    ctx.align_set_pool(seqs)
    ctx.align_set_verdict_threshold(0.0)
    s0, w0, r0 = ctx.align_pairs(pairs, 11, *p)
    assert ctx.timings()["align_version"] == 2
    stopped = 0
    try:
        for thr in (0.2, 0.6):
            ctx.align_set_verdict_threshold(thr)
            s1, w1, r1 = ctx.align_pairs(pairs, 11, *p)
            assert np.array_equal(s0, s1)
            assert np.array_equal(r0 >= thr, r1 >= thr), thr
            assert np.all(w1 <= w0)
            stopped += int(np.count_nonzero(w1 < w0))
    finally:
        ctx.align_set_verdict_threshold(0.0)
    assert stopped > 0
    # the full count is the host's where the host is cheap (the pairs under 1000 x 1000 cells)
    cheap = [i for i, pr in enumerate(pairs) if len(seqs[pr[0]]) * len(seqs[pr[1]]) < 10**6]
    assert len(cheap) >= 8
    L = _lib.load()
    for i in cheap:
        qi, ri, rc, e = pairs[i]
        hops, hs = _host_ops(seqs[qi], seqs[ri], rc, gap_open(e), p)
        comp = api.ops_to_comp(hops)
        assert s0[i] == hs and r0[i] == (L.ioc_host_aln_ratio(comp, len(comp), e, len(seqs[qi]), 11) if len(seqs[qi]) else 0.0), i


def test_sinks_carry_the_parameters(ctx):
    """ioc_align_pairs_stats / _pileup / _polish at (5, -4, 2) on the routes set (version 2): the records, the table and the
    consensus are ioc_host_ops_stats / ioc_host_ops_pileup / ioc_host_pileup_call of the HOST's strings at these parameters —
    which differ from the strings at 2 / -2 / 1, so a sink that dropped the three integers on its way to the walk would show."""
    p = (5, -4, 2)
    seqs, pairs = _route_pairs()
    assert _routes(seqs, pairs, p) == {ROUTE_V2}
    ctx.align_set_pool(seqs)
    host = [_host_ops(seqs[pr[0]], seqs[pr[1]], pr[2], gap_open(pr[3]), p) for pr in pairs]
    other = [_host_ops(seqs[pr[0]], seqs[pr[1]], pr[2], gap_open(pr[3]), DEFAULT) for pr in pairs[:3]]
    assert any(a[0] != b[0] for a, b in zip(host, other))
    # stats
    score, _, _, st = ctx.align_pairs_stats(pairs, 11, *p)
    assert ctx.timings()["align_version"] == 2
    assert list(score) == [h[1] for h in host]
    for i, (ops, _) in enumerate(host):
        assert {f: int(st[f][i]) for f in api.ALN_STATS_FIELDS} == api.ops_stats(ops), i
    # pileup and polish: one segment per (reference, frame)
    segs, sop = _segments(pairs)
    row0 = np.concatenate([[0], np.cumsum([len(seqs[r]) + 1 for r, _ in segs])])
    n_rows, row_base = int(row0[-1]), [int(row0[g]) for g in sop]
    want_cols, want_ins = np.zeros(n_rows, api.PILEUP_DTYPE), np.zeros(n_rows, api.PILEUP_INS_DTYPE)
    for pr, (ops, _), rb in zip(pairs, host, row_base):
        m = len(seqs[pr[1]])
        api.ops_pileup(ops, seqs[pr[0]], m, cols=want_cols[rb:rb + m + 1])
        api.ops_pileup_ins(ops, seqs[pr[0]], m, ins=want_ins[rb:rb + m + 1])
    got = ctx.align_pairs_pileup(pairs, 11, row_base, n_rows, match=p[0], mismatch=p[1], gap_extend=p[2])
    assert list(got[0]) == [h[1] for h in host] and np.array_equal(got[3], want_cols)
    pol = ctx.align_pairs_polish(pairs, 11, segs, sop, 1, tables=True, match=p[0], mismatch=p[1], gap_extend=p[2])
    assert list(pol["score"]) == [h[1] for h in host]
    assert np.array_equal(pol["cols"], want_cols) and np.array_equal(pol["ins"], want_ins)
    for g, (ref, rc) in enumerate(segs):
        frame = revcomp(seqs[ref]) if rc else seqs[ref]
        rows = slice(int(row0[g]), int(row0[g]) + len(frame) + 1)
        want = api.pileup_call(want_cols[rows], want_ins[rows], frame, 1)
        assert (pol["seq"][g], pol["qual"][g]) == want[:2], g
        assert {f: int(pol["polish"][f][g]) for f in api.POLISH_STATS_FIELDS} == want[2], g


def _raw(ctx, pairs, k, p):
    """ioc_align_pairs itself, the outputs prefilled: (return code, score, windows, ratio)."""
    n = len(pairs)
    score, win, ratio = np.full(n, -77, np.int32), np.full(n, -77, np.int64), np.full(n, -77.0, np.float64)
    rc = _lib.load().ioc_align_pairs(ctx.h, n, ctx._aln_pairs(pairs), k, p[0], p[1], p[2], score.ctypes.data_as(C.POINTER(C.c_int32)),
                                     win.ctypes.data_as(C.POINTER(C.c_int64)), ratio.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, score, win, ratio


def test_parameters_outside_the_accepted_range_are_refused(ctx):
    """include/isonclust2_hip.h, next to ioc_align_pairs: gap_extend >= 0, w = max(|match|, |mismatch|) + 2 gap_extend + 5 at most
    2^24, w x (query + reference length) at most 2^30 for every pair.  IOC_ERR_ARG and no output written — not even the answer of
    the pair with an empty sequence in front of the pair that is too long —; the emitting form refuses alike."""
    seqs, pairs = _small_pairs(29, 30)
    seqs = seqs + [b""]
    pairs = [(len(seqs) - 1, 0, 0, 0.1)] + pairs
    span = max(len(seqs[pr[0]]) + len(seqs[pr[1]]) for pr in pairs if len(seqs[pr[0]]) and len(seqs[pr[1]]))
    assert span > 200
    ctx.align_set_pool(seqs)
    w_most = (1 << 30) // span                               # the largest w the longest pair accepts
    for p in ((2, -2, -1), ((1 << 24) - 4, -2, 0), (2, -(1 << 24), 1), (w_most - 5 + 1, -2, 0), (2, -2, (w_most - 5) // 2 + 1)):
        rc, score, win, ratio = _raw(ctx, pairs, 11, p)
        assert rc == -1, (p, rc)
        assert np.all(score == -77) and np.all(win == -77) and np.all(ratio == -77.0), p
        with pytest.raises(api.IocError):
            ctx.align_pairs_ops(pairs, 11, *p)
    # just inside: scores of millions in the comparing kernel's 32-bit cells, the host's all the same
    p = (w_most - 5, -(w_most - 5), 0)
    assert _routes(seqs, pairs, p) == {ROUTE_COMPARE}
    got = _check(ctx, seqs, pairs, 11, p, set_pool=False)
    assert got[4] == 1 and max(got[0]) > 10**6
