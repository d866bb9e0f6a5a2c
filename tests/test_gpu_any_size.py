"""ioc_cluster_consensus on a batch of more entries than one device pass takes (131 072): the driver's windows stop at the pass
limit, IOC_MERGE_CHUNK bounds them as it bounds the chunks of ioc_cluster_merge, and the result is the one of the unbounded walk.

The large view is built here: 131 072 + 256 entries of which 400 are the entries of a small sorted batch, all others gated
(state 1, score -1, no minimizers, no sequence: the gates skip them, src/cluster.cpp:116-160, so they need no oracle counterpart).
Placement: the first 320 real entries one every 328th position; the last 80 four positions apart around the 131 072nd entry,
40 on each side.  (400 entries spaced 328 apart over all 131 328 positions would leave at most ONE real entry behind the
131 072nd: no consensus event could fall there.)"""
import numpy as np
import pytest

from isonclust2_amd import _lib, api, synth
from tests import adopt_common as ac
from tests.fuzz_cases import oracle_consensus_run
from tests.helpers import ToyGraphs

pytestmark = pytest.mark.gpu

PASS = 131072
N_PAD = PASS + 256
CMAX, CMIN, PERIOD = 6, 2, 500     # (the oracle takes 212 consensus events on this batch, 4 of them at its last 40 entries)
POS = np.concatenate([328 * np.arange(320) + 256, PASS - 160 + 4 * np.arange(80)]).astype(np.int64)


@pytest.fixture(scope="module")
def small():
    """The 400-entry batch, the oracle's consensus run of it, and the product's run of the same (unpadded) batch."""
    rs = synth.generate(400, 10, 700, 12, 21, seed=4)
    B, view, ost, og = oracle_consensus_run(rs, CMAX, CMIN, PERIOD, mode="fast")
    acl, ast = B.assignments(rs.n)
    v = ac.with_sequences(rs, view)
    ctx = api.Context(0)
    got = _run(ctx, v)
    ctx.close()
    return dict(view=v, ocl=acl[view["orig"]], ostr=ast[view["orig"]], ost=ost, og=og, oindex=B.index(), plain=got)


def _run(ctx, view):
    g = ToyGraphs()
    cargs = _lib.ConsensusArgs(cons_min_size=CMIN, cons_max_size=CMAX, cons_period=PERIOD, left_depth=-1, left_sizes=None)
    cls, strand, st = ctx.cluster_consensus(api.default_params(11, 15, "fast"), None, view, cargs, g.ops)
    return dict(cls=cls, strand=strand, st=st, g=g, index=ctx.index_export())


def _same_graph_log(g, og):
    first = next((x for x in range(min(len(g.log), len(og.log))) if g.log[x] != og.log[x]), None)
    assert first is None, (first, g.log[first - 2:first + 2], og.log[first - 2:first + 2])
    assert len(g.log) == len(og.log) and g.calls == og.calls
    assert {kk: [(len(s), wt) for s, wt in vv] for kk, vv in g.g[0].items()} == \
           {kk: [(len(s), wt) for s, wt in vv] for kk, vv in og.g[0].items()}


def _equals_oracle(got, small, at=None):
    cls, strand = (got["cls"], got["strand"]) if at is None else (got["cls"][at], got["strand"][at])
    assert np.array_equal(cls, small["ocl"]) and np.array_equal(strand, small["ostr"])
    assert got["st"]["n_cons_invoked"] == small["ost"]["cons_invoked"]
    _same_graph_log(got["g"], small["og"])
    ac.same_mindb(got["index"], small["oindex"])


def test_unpadded_batch_equals_the_oracle(small):
    assert small["ost"]["cons_invoked"] > 10
    _equals_oracle(small["plain"], small)


def test_consensus_beyond_one_device_pass(small):
    padded = ac.pad_view(small["view"], N_PAD, POS)
    ctx = api.Context(0)
    got = _run(ctx, padded)
    ctx.close()
    real = np.zeros(N_PAD, bool)
    real[POS] = True
    assert np.all(got["cls"][~real] == -1) and np.all(got["strand"][~real] == 0)
    # consensus events (entry that triggered them, in the order they were taken) on both sides of the pass limit
    entries = np.array([e[1] for e in got["g"].rep_events])
    print(f"consensus events: {len(entries)}, in front of entry {PASS}: {int((entries < PASS).sum())}, behind it: {int((entries >= PASS).sum())}")
    assert (entries < PASS).sum() >= 3 and (entries >= PASS).sum() >= 3
    plain = small["plain"]
    assert np.array_equal(got["cls"][POS], plain["cls"]) and np.array_equal(got["strand"][POS], plain["strand"])
    assert got["st"]["n_clusters"] == plain["st"]["n_clusters"] and got["st"]["n_cons_invoked"] == plain["st"]["n_cons_invoked"]
    ac.same_mindb(got["index"], plain["index"])
    assert [(c, int(np.searchsorted(POS, e))) + tuple(r) for c, e, *r in got["g"].rep_events] == [tuple(ev) for ev in plain["g"].rep_events]
    assert got["g"].log == plain["g"].log
    _equals_oracle(got, small, at=POS)


def test_window_bound_honoured(small, monkeypatch):
    """IOC_MERGE_CHUNK=64 bounds the consensus windows: the unbounded run's result."""
    monkeypatch.setenv("IOC_MERGE_CHUNK", "64")
    ctx = api.Context(0)
    got = _run(ctx, small["view"])
    ctx.close()
    plain = small["plain"]
    assert got["st"]["n_cons_restarts"] >= 400 // 64
    assert np.array_equal(got["cls"], plain["cls"]) and np.array_equal(got["strand"], plain["strand"])
    assert got["st"]["n_clusters"] == plain["st"]["n_clusters"] and got["st"]["n_cons_invoked"] == plain["st"]["n_cons_invoked"]
    ac.same_mindb(got["index"], plain["index"])
    assert got["g"].rep_events == plain["g"].rep_events and got["g"].log == plain["g"].log
    _equals_oracle(got, small)
