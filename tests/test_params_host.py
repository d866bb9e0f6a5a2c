"""CPU checks of the host helpers that turn the clustering thresholds into the integers the kernels work with, away from the
default point (k, w) = (11, 15), MinProbNoHits 0.1, MappedThreshold 0.65:
  ioc_host_gap_limits  the largest gap of missing minimizers getMappedRatio still counts (src/cluster.cpp:333-347), per
                       (target cell, query cell) of the p_shared table, against the oracle's orc_gap_limit
  ioc_host_min_total   the smallest totalMapped that passes `float(totalMapped / hpcLen) >= MappedThreshold`
                       (src/cluster.cpp:390-400), against a brute force over every total
and the shape of the table that k_gap_bounds (ioc_resolve.hip) must not assume: the limits of a query cell do not always
ascend with the target's cell."""
import time

import numpy as np
import pytest

from isonclust2_amd import api
from oracle import pyoracle as po

# the oracle stops counting at 10^6, the product at INT32_MAX - 2 (every gap passes): both mean "unbounded"
UNBOUNDED = 10 ** 6
KW_ALL = [(k, w) for k in range(10, 31) for w in range(k, k + 32)]

# (k, w) -> query cells whose limit at the last target cell (15) is below the column's largest limit, at MinProbNoHits 0.1;
# at 0.05 and below (26, 39 - 43) cell 12 joins them
NON_MONOTONE_01 = {
    **{(21, w): [11] for w in range(49, 53)},
    **{(26, w): [10, 13] for w in range(54, 58)},
    **{(27, w): [12, 15] for w in range(50, 55)},
    **{(28, w): [15] for w in range(56, 60)},
    **{(29, w): [14] for w in range(32, 37)},
    **{(30, w): [15] for w in range(38, 43)},
}
NON_MONOTONE_LOW = {**NON_MONOTONE_01, **{(26, w): [12] for w in range(39, 44)}}


def _norm(x):
    return min(int(x), UNBOUNDED)


@pytest.fixture(scope="module")
def tables():
    out = {}
    for k, w in KW_ALL:
        tab, filled = po.pmin_table(k, w)
        if filled == 225:
            out[(k, w)] = tab
    return out


@pytest.mark.parametrize("prob", [1e-4, 0.01, 0.05, 0.1, 0.3, 0.5, 1.0, 1.5])
def test_gap_limits_equal_oracle_every_kw(tables, prob):
    assert len(tables) == len(KW_ALL)      # every (k, w) of k 10 - 30, w k - k+31 has its 225 cells
    memo = {}                              # (the table repeats its values across neighbouring w)
    n_cells = 0
    for (k, w), tab in tables.items():
        g, p = api.host_gap_limits(k, w, prob)
        assert np.array_equal(p, tab), (k, w)
        for a in range(15):
            for b in range(15):
                x = float(tab[a, b])
                if x not in memo:
                    memo[x] = po.lib().orc_gap_limit(x, prob)
                assert _norm(g[a, b]) == _norm(memo[x]), (k, w, a + 1, b + 1, prob, int(g[a, b]), memo[x])
                n_cells += 1
    assert n_cells == 225 * len(KW_ALL)
    if prob > 1.0:
        assert all(int(api.host_gap_limits(k, w, prob)[0].max()) == -1 for k, w in ((10, 10), (30, 61)))


def test_gap_limits_unbounded_at_zero(tables):
    """MinProbNoHits 0: every gap passes (pow(pError, n) >= 0), the product says so without walking n up to its cap."""
    t0 = time.time()
    for k, w in KW_ALL:
        g, _ = api.host_gap_limits(k, w, 0.0)
        assert int(g.min()) == 2 ** 31 - 3, (k, w)
    assert time.time() - t0 < 10.0
    # the oracle on one table (it walks 10^6 calls of pow per distinct cell value)
    k, w = 11, 15
    g, _ = api.host_gap_limits(k, w, 0.0)
    memo = {}
    for a in range(15):
        for b in range(15):
            x = float(tables[(k, w)][a, b])
            if x not in memo:
                memo[x] = po.lib().orc_gap_limit(x, 0.0)
            assert _norm(g[a, b]) == _norm(memo[x]) == UNBOUNDED


@pytest.mark.parametrize("prob", [0.1, 0.05, 0.01])
def test_gap_limit_columns_are_not_always_ascending(prob):
    """The rows the GPU reproducer of tests/test_gpu_params.py relies on: a query cell whose limit at target cell 15 is not
    the column's largest.  k_gap_bounds takes its head / tail extents and its LDS window from the largest limit of the column;
    this pins that the table really has such columns, and exactly where."""
    want = NON_MONOTONE_01 if prob == 0.1 else NON_MONOTONE_LOW
    got = {}
    for k, w in KW_ALL:
        g, _ = api.host_gap_limits(k, w, prob)
        cells = [c + 1 for c in range(15) if g[14, c] < g[:, c].max()]
        if cells:
            got[(k, w)] = cells
    assert got == want
    g, _ = api.host_gap_limits(21, 50, 0.1)
    assert g[12:, 10].tolist() == [81, 112, 110]
    g, _ = api.host_gap_limits(30, 40, 0.1)
    assert g[13:, 14].tolist() == [1506, 1501]


@pytest.mark.parametrize("thr", [0.0, 0.3, 0.65, 0.9, 0.99, 1.0, 1.1])
def test_min_total_equals_brute_force(thr):
    for hl in (1, 2, 3, 7, 1000, 2 ** 24 + 1):
        T = np.arange(hl + 1, dtype=np.float64)
        # cluster.cpp:390-400: the ratio in double, narrowed to float, compared with the double threshold
        ok = (T / float(hl)).astype(np.float32).astype(np.float64) >= thr
        want = int(np.argmax(ok)) if ok.any() else 0xFFFFFFFE
        assert api.host_min_total(hl, thr) == want, (hl, thr)
