"""The restatement of the greedy loop's bookkeeping (tests/resolve_common.greedy_resolve) checked on the CPU: its Sizes and
decisions against the oracle's traced run, its walk lengths against helpers.walk_lengths, a six-query example worked out by
hand, and int(top * MinFraction) at the tops where a 32-bit product parts from the double one.  The GPU tests
(tests/test_gpu_resolve_outputs.py) compare ioc_resolve's cuts, tie sets and flags with this restatement."""
import functools

import numpy as np
import pytest

from isonclust2_amd import api, synth
from tests import resolve_common as rc
from tests.helpers import oracle_traced_run, walk_lengths


@functools.lru_cache(maxsize=None)
def traced(cfg, seed):
    """the oracle's fast-mode run of a synthetic configuration, every entry traced, and its restatement (shared, read only)"""
    rs = synth.generate_config(cfg, seed=seed)
    run = oracle_traced_run(rs)
    view, rows, ocl = run["view"], run["rows"], run["cls"]
    n = rs.n
    need = np.array([api.host_min_total(int(h), 0.65) for h in view["hpc_len"]], np.int64)
    total = {(int(e), int(c), int(s)): int(x) for e, c, s, x in zip(rows["entry"], rows["cls"], rows["strand"], rows["total_mapped"])}
    gated = {int(j): -2 for j in np.flatnonzero(np.asarray(view["state"]) != 0)}
    # (single batch: target = the entry that opened the cluster, whose cluster id is the oracle's assignment of that entry)
    passes = lambda q, t, s, z: total[(q, int(ocl[t]), s)] >= need[q]      # noqa: E731
    fwd, rev = rc.lists_of_view(view)
    R = rc.greedy_resolve(n, 0, fwd, rev, [], need, 5, 0.8, forced=gated, passes=passes, tables=True)
    return rs, run, R


@pytest.mark.parametrize("cfg,seed", [("tiny", 7), ("short_dup", 1)])
def test_sizes_and_decisions_equal_the_oracles_trace(cfg, seed):
    rs, run, R = traced(cfg, seed)
    rows, ocl, ost = run["rows"], run["cls"], run["strand"]
    assert len(rows["entry"]) > rs.n
    for j in range(rs.n):
        m = rows["entry"] == j
        want = sorted(zip(rows["cls"][m].tolist(), rows["strand"][m].tolist(), rows["size"][m].tolist()))
        t, s, z = R.cands[j]
        assert sorted(zip(ocl[t].tolist(), s.tolist(), z.tolist())) == want, j
    # the decisions: the oracle's cluster of every entry, exact where no order-dependent tie is flagged
    gated = np.asarray(run["view"]["state"]) != 0
    for j in np.flatnonzero(~gated).tolist():
        if R.flags[j] & 1:
            assert any(ocl[k >> 1] == ocl[j] and (-1 if k & 1 else 1) == ost[j] for k in R.pass_keys[j]), j
        elif R.target[j] < 0:
            assert ocl[j] not in ocl[:j][~gated[:j]].tolist(), j            # opens a cluster of its own
        else:
            assert (ocl[R.target[j]], R.strand[j]) == (ocl[j], ost[j]), j
    assert int((R.cut != rc.INT32_MAX).sum()) >= rs.n // 4                   # (walks: most reads of these sets join)


@pytest.mark.parametrize("cfg,seed", [("tiny", 7), ("short_dup", 1)])
def test_walk_lengths_equal_the_restated_candidates_above_the_cut(cfg, seed):
    rs, run, R = traced(cfg, seed)
    assert np.array_equal(walk_lengths(run["rows"], rs.n), R.items)
    assert np.array_equal(R.items, R.walk)                                  # (MinFraction <= 1: the cut never lies above top)


def test_six_queries_by_hand():
    """Two left clusters A = {1..6}, B = {1..5, 7}; MinShared 5, MinFraction 0.8.
      q0  [1 2 3 4 5], passes: A and B tie at Size 5 (cut 4), both pass -> bit 0, one of them
      q1  [1 2 3 200]: top 3 < MinShared -> opens cluster 3 (= L + 1), no walk
      q2  gated (forced -2); its list would make it the best candidate of q3, it never is one
      q3  [1 2 3 4 5 6 300 301], nothing passes: A 6, B 5, q1 3 -> top 6, cut 4, tie set {A}; bit 1, takes its verdict (B, -1)
      q4  reverse list [7 5 4 3 2 1], passes: B 6, A 5 on the reverse strand -> joins B reversed, no flag
      q5  [1 2 3 200 200 600], nothing passes: q1 holds five of the entries (the repeated 200 counts twice) -> top 5, tie set
          {q1}, bit 1, no verdict -> opens a cluster"""
    left = [[1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 7]]
    fwd = [[1, 2, 3, 4, 5], [1, 2, 3, 200], [1, 2, 3, 4, 5, 6, 300, 301], [1, 2, 3, 4, 5, 6, 300, 301], [500], [1, 2, 3, 200, 200, 600]]
    rev = [[100], [201], [401], [400], [7, 5, 4, 3, 2, 1], [601]]
    need = np.array([0, 0, 0, rc.NEED_NONE, 0, rc.NEED_NONE])
    vt = np.array([rc.NO_VERDICT, -1, 0, 1, 0, rc.NO_VERDICT])
    vs = np.array([0, 0, 1, -1, 1, 0])
    R = rc.greedy_resolve(6, 2, fwd, rev, left, need, 5, 0.8, forced={2: -2}, verdict_t=vt, verdict_s=vs)
    M = rc.INT32_MAX
    assert R.target.tolist() == [0, -1, -2, 1, 1, -1]
    assert R.strand.tolist() == [1, 0, 0, -1, -1, 0]
    assert R.flags.tolist() == [1, 0, 0, 2, 0, 2]
    assert R.cut.tolist() == [4, M, M, 4, 4, 4]
    assert [sorted(t) for t in R.ties] == [[0, 2], [], [], [0], [3], [6]]
    assert sorted(R.pass_keys[0]) == [0, 2] and R.top.tolist() == [5, 0, 0, 6, 6, 5]
    assert R.walk.tolist() == [2, 0, 0, 2, 2, 1]
    # the comparison the GPU tests use accepts this result and either winner of q0, and nothing else
    count = np.array([2, 0, 0, 1, 1, 1], np.uint32)
    keys = np.zeros((6, rc.TIE_SLOTS), np.uint32)
    keys[0, :2], keys[3, 0], keys[4, 0], keys[5, 0] = (2, 0), 0, 3, 6
    dec = (R.target.copy(), R.strand.copy(), R.flags.copy())
    rc.compare(R, dec, R.cut.copy(), (count, keys))
    dec[0][0] = 1
    rc.compare(R, dec, R.cut.copy(), (count, keys))
    for spoil in ("winner", "cut", "count", "key", "flag"):
        d, c, k, u = [x.copy() for x in dec], R.cut.copy(), keys.copy(), count.copy()
        if spoil == "winner":
            d[0][4] = 0
        elif spoil == "cut":
            c[3] = 5
        elif spoil == "count":
            u[5] = 2
        elif spoil == "key":
            k[4, 0] = 2
        else:
            d[2][5] = 0
        with pytest.raises(AssertionError):
            rc.compare(R, tuple(d), c, (u, k))


# (top, MinFraction, the cut): found by search over top < 400 — the first three part from a product whose factor was narrowed to
# 32 bits, the last three from a product formed in 32 bits altogether
FLOAT_PARTS = [(10, 0.7, 7), (20, 0.7, 14), (10, 0.9, 9), (90, 0.7, 62), (170, 0.7, 118), (180, 0.7, 125)]


def test_cut_is_the_truncated_double_product():
    for top, f, want in FLOAT_PARTS:
        assert rc.cut_of(top, f) == want
        narrowed = int(float(top) * float(np.float32(f)))
        assert narrowed != want or rc.cut_of_f32(top, f) != want, (top, f)
    assert int(float(10) * float(np.float32(0.7))) == 6 and rc.cut_of_f32(90, 0.7) == 63
    # through the loop: one left cluster that holds every value, one query of `top` entries
    for top, f, want in FLOAT_PARTS:
        R = rc.greedy_resolve(1, 1, [np.arange(top) % 40], [[77]], [np.arange(40)], [0], 5, f)
        assert (R.top[0], R.cut[0], R.target[0]) == (top, want, 0)
    assert rc.cut_of(5, 1.25) == 6 and rc.cut_of(7, 0.0) == 0 and rc.cut_of(3, 0.5) == 1


def test_crafted_cases_reach_their_paths():
    """The builders of the GPU tests, from the restatement alone (the GPU tests assert the same counts before they compare)."""
    e0 = rc.restate(rc.edges_case())
    assert e0.n_ties.tolist() == list(rc.EDGE_TIES) + [5] and e0.items.tolist() == list(rc.EDGE_TIES) + [5]
    assert e0.flags.tolist() == [0] + [1] * (len(rc.EDGE_TIES) - 1) + [1] and e0.strand[-1] == -1
    assert all(k & 1 for k in e0.ties[-1])                                   # the last query: reverse-strand candidates only
    case = rc.edges_case()
    e1 = rc.restate(case, need=np.full(case["n"], rc.NEED_NONE))
    assert set(e1.flags.tolist()) == {2} and set(e1.target.tolist()) == {-1}
