"""The host aligner (ioc_host_align, ioc_host_align_ops) at the scoring parameters of tests/align_params_common.py — the
definition the GPU aligner is held to in tests/test_gpu_align_params.py.  Three statements written independently of each other
agree on every pair of every set: the host aligner, the oracle's aligner (oracle.cpp `sg_trace`: score and comparison string) and
a plain Gotoh score loop below (score only, no traceback).  And the rule that says which kernel family a pair takes
(ioc_host_align_route) is pinned to a table worked out by hand.  No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from oracle import pyoracle as po
from tests.align_ops_checks import check_ops, ops_to_comp
from tests.align_params_common import DEFAULT, GAP_OPENS, PARAM_IDS, PARAM_SETS, PARAM_TABLE, ROUTE_COMPARE, ROUTE_PROFILE, ROUTE_V2, route, routes
from tests.test_oracle_align import aligner_pairs

N_PAIRS = 150


@functools.lru_cache(maxsize=None)
def _pairs():
    return [(q, r, go) for _, q, r, go in aligner_pairs(N_PAIRS)]


def gotoh_scores(q, r, gap_open, params):
    """The semi-global affine score of q against r for every (match, mismatch, gap_extend) of `params` at once: H, E, F filled
    anti-diagonal by anti-diagonal (the cells of one depend on the two before it only), first row and column 0 (free leading
    gaps), a gap of length L costing gap_open + (L - 1) gap_extend, the score the best cell of the last row and the last column
    (free trailing gaps).  int64 throughout."""
    n, m = len(q), len(r)
    P = np.array(params, np.int64)
    mt, mm, ge = P[:, 0], P[:, 1], P[:, 2]
    none = -10**12
    H = np.zeros((n + 1, m + 1, len(P)), np.int64)
    E, F = np.full_like(H, none), np.full_like(H, none)
    eq = np.frombuffer(q, np.uint8)[:, None] == np.frombuffer(r, np.uint8)[None, :]
    sub = np.where(eq[:, :, None], mt, mm)
    for d in range(2, n + m + 1):
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        E[i, j] = np.maximum(H[i, j - 1] - gap_open, E[i, j - 1] - ge)
        F[i, j] = np.maximum(H[i - 1, j] - gap_open, F[i - 1, j] - ge)
        H[i, j] = np.maximum(np.maximum(H[i - 1, j - 1] + sub[i - 1, j - 1], E[i, j]), F[i, j])
    return np.maximum(H[:, m].max(axis=0), H[n].max(axis=0))


@functools.lru_cache(maxsize=None)
def _gotoh():
    """[pair][parameter set] -> score, computed once for every test of the module."""
    return np.array([gotoh_scores(q, r, go, PARAM_SETS) for q, r, go in _pairs()])


def _host(q, r, go, p):
    cap = len(q) + len(r) + 2
    comp, sc = C.create_string_buffer(cap), C.c_int32()
    n = _lib.load().ioc_host_align(q, len(q), r, len(r), p[0], p[1], go, p[2], comp, cap, C.byref(sc))
    assert n >= 0
    return sc.value, comp.raw[:n]


def _oracle(q, r, go, p):
    cap = len(q) + len(r) + 2
    comp, sc = C.create_string_buffer(cap), C.c_int32()
    n = po.lib().orc_align(q, len(q), r, len(r), p[0], p[1], go, p[2], comp, cap, C.byref(sc))
    assert n >= 0
    return sc.value, comp.raw[:n]


def test_the_pairs_are_what_the_sets_need():
    pairs = _pairs()
    assert len(pairs) == N_PAIRS and {go for _, _, go in pairs} == set(GAP_OPENS)
    assert any(b"N" in q for q, _, _ in pairs) and min(len(q) * len(r) for q, r, _ in pairs) < 400 < 40000 < max(len(q) * len(r) for q, r, _ in pairs)
    assert len(PARAM_SETS) == 11 and DEFAULT in PARAM_TABLE


@pytest.mark.parametrize("p", PARAM_SETS, ids=PARAM_IDS)
def test_three_aligners_agree_on_the_score(p):
    gs = _gotoh()[:, PARAM_SETS.index(p)]
    for t, (q, r, go) in enumerate(_pairs()):
        hs, _ = _host(q, r, go, p)
        os_, _ = _oracle(q, r, go, p)
        assert hs == os_ == gs[t], (t, len(q), len(r), go, p, hs, os_, int(gs[t]))


@pytest.mark.parametrize("p", PARAM_SETS, ids=PARAM_IDS)
def test_comparison_and_operation_strings(p):
    """The comparison string is the oracle's byte for byte; the operation string is that comparison string under '=' -> '|',
    carries the same score and passes check_ops (with the re-scoring of runs where gap_open <= gap_extend)."""
    for t, (q, r, go) in enumerate(_pairs()):
        tag = (t, len(q), len(r), go, p)
        hs, hc = _host(q, r, go, p)
        _, oc = _oracle(q, r, go, p)
        assert hc == oc, tag
        ops, score = api.host_align_ops(q, r, match=p[0], mismatch=p[1], gap_open=go, gap_extend=p[2])
        assert score == hs and ops_to_comp(ops) == hc, tag
        check_ops(ops, q, r, score, go, match=p[0], mismatch=p[1], gap_extend=p[2], tag=tag, any_gap_costs=True)


def test_check_ops_rescoring_of_runs():
    """A run of L gap columns: gap_open + (L - 1) gap_extend where opening costs more than extending (and the caller need not
    say anything), gap_open + (L - 1) min(gap_open, gap_extend) where it does not — and then only for a caller that asks."""
    q, r, ops = b"ACGTAC", b"ACAC", b"==II=="
    check_ops(ops, q, r, 8 - (3 + 1), 3)                                               # 3 + 1
    check_ops(ops, q, r, 8 - (2 + 2), 2, gap_extend=2, any_gap_costs=True)             # open == extend
    check_ops(ops, q, r, 8 - (2 + 2), 2, gap_extend=3, any_gap_costs=True)             # two gaps of one column: 2 + 2, not 2 + 3
    check_ops(ops, q, r, 8 - (5 + 0), 5, gap_extend=0)
    with pytest.raises(AssertionError):
        check_ops(ops, q, r, 8 - (2 + 3), 2, gap_extend=3, any_gap_costs=True)         # (what one gap of two columns would cost)
    with pytest.raises(AssertionError):
        check_ops(ops, q, r, 8 - (2 + 2), 2, gap_extend=3)                             # the callers of before keep their assert
    with pytest.raises(AssertionError):
        check_ops(ops, q, r, 8 - (2 + 2), 2, gap_extend=2)


# {parameter set: routes at gap_open 2, 3, 4, 5}, by hand from cm = match + gap_extend + gap_open, cx = mismatch + gap_extend +
# gap_open, gd = gap_open - gap_extend: profile needs 0 <= cm, cx <= 255; version 2 also gd >= 0 and max(cm, cx) <= 31
C_, P_, V_ = ROUTE_COMPARE, ROUTE_PROFILE, ROUTE_V2
ROUTES_BY_HAND = {
    (2, -2, 1): (V_, V_, V_, V_),
    (1, -1, 1): (V_, V_, V_, V_),
    (5, -4, 2): (V_, V_, V_, V_),        # cx = 0 at gap_open 2, gd = 0 there
    (2, -2, 0): (V_, V_, V_, V_),        # cx = 0 at gap_open 2
    (2, -6, 1): (C_, C_, C_, V_),        # cx = -3, -2, -1, 0
    (250, -2, 1): (P_, P_, P_, C_),      # cm = 253, 254, 255, 256, far above 31
    (2, -2, 3): (P_, V_, V_, V_),        # gd = -1, 0, 1, 2
    (2, -2, 6): (P_, P_, P_, P_),        # gd = -4 .. -1
    (0, -1, 1): (V_, V_, V_, V_),
    (3, -1, 2): (V_, V_, V_, V_),
    (1, -3, 5): (P_, P_, P_, V_),        # gd = -3 .. 0
}


def test_route_table():
    assert set(ROUTES_BY_HAND) == set(PARAM_SETS)
    for p, want in ROUTES_BY_HAND.items():
        assert tuple(routes(p)[go] for go in GAP_OPENS) == want, p


def test_route_edges():
    """Each bound of the rule from both sides, everything else held inside."""
    assert route((2, -6, 1), 5) == V_ and route((2, -6, 1), 4) == C_            # cx 0 / -1
    assert route((2, -7, 1), 5) == C_
    assert route((250, -2, 1), 4) == P_ and route((250, -2, 1), 5) == C_        # cm 255 / 256
    assert route((2, 250, 1), 4) == P_ and route((2, 251, 1), 4) == C_          # cx 255 / 256 (a "mismatch" that pays)
    assert route((-7, -8, 1), 5) == C_ and route((-6, -6, 1), 5) == V_          # cm -1 / 0
    assert route((2, -2, 2), 2) == V_ and route((2, -2, 3), 2) == P_            # gd 0 / -1
    assert route((2, -2, 5), 5) == V_ and route((2, -2, 6), 5) == P_
    # version 2's 16-bit halves: a tile's top row, 1024 columns, is cut to 16 bits around its first column, and a lane runs 64
    # rows between two looks of the guard with 65535 - (32768 + 28000) = 4767 above it: max(cm, cx) 31 / 32
    assert 1024 * 31 <= 32767 < 1024 * 32 and 64 * 31 <= 4767
    assert route((28, -2, 1), 2) == V_ and route((29, -2, 1), 2) == P_
    assert route((25, -2, 1), 5) == V_ and route((26, -2, 1), 5) == P_
    assert route((2, 28, 1), 2) == V_ and route((2, 29, 1), 2) == P_            # (the rise of a mismatch that pays more)


def test_default_parameters_route_as_ever():
    """2 / -2 / 1: version 2 may take every pair, whatever its gap_open."""
    assert routes(DEFAULT) == {go: V_ for go in GAP_OPENS}
