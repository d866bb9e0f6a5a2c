"""Clustering away from the default point of its parameters, device against oracle.  Every other parity test runs MinShared 5,
MinFraction 0.8, MappedThreshold 0.65, MinProbNoHits 0.1, AlignedThreshold 0.2 and k 10 - 15; the kernels derive shortcuts from
these values (the Size cut and the phase-1 rule of k_decide_scan / k_decide_pick, `need`, the upper bound of totalMapped and the
list cut of k_gap_bounds, the aligner's verdict threshold), each one correct only under assumptions the default point happens to
satisfy.  Here: a covering grid of the thresholds, a sweep of (k, w) over the whole table, reproducers of the faults off the
default point (a gap-limit column that does not ascend, MinFraction > 1), the alignment modes, merge, consensus and the command
line.  Every case compares cluster id and strand per entry and the number of clusters with the oracle on the same reads and the
same parameters (tests/helpers.py: param_pair)."""
import numpy as np
import pytest

from isonclust2_amd import api, synth
from oracle import pyoracle as po
from tests import fuzz_cases as fz
from tests.helpers import compare_candidate_tables, oracle_entry_assignments, oracle_sorted_batch, param_pair

pytestmark = pytest.mark.gpu

MS = [-1, 0, 1, 2, 12]
MF = [0.0, 0.5, 1.0, 1.25]
MT = [0.0, 0.3, 0.9, 0.99, 1.0, 1.2]
PN = [1e-4, 0.01, 0.5, 1.0, 1.5]
# covering set: case i takes (MappedThreshold, MinProbNoHits) pair i of their 30 and (MinShared, MinFraction) pair i % 20 of theirs
GRID = [dict(min_shared=MS[(i % 20) // 4], min_fraction=MF[i % 4], mapped_threshold=MT[i % 6], min_prob_no_hits=PN[i // 6])
        for i in range(30)]
# (k, w) sweep at MinProbNoHits 0.1: every k, w = k and w = k + 31, and every group of (k, w) whose gap-limit columns do not ascend
# to the last target cell (tests/test_params_host.py pins those rows); (26, 41) only at 0.01
KW = [(10, 10), (11, 42), (12, 12), (13, 44), (14, 14), (15, 46), (16, 16), (17, 48), (18, 18), (19, 50), (20, 20), (21, 50),
      (22, 22), (23, 54), (24, 24), (25, 56), (26, 55), (27, 52), (28, 57), (29, 33), (30, 40), (30, 61)]
KW_CASES = [dict(k=k, w=w, min_prob_no_hits=0.1) for k, w in KW] + [dict(k=26, w=41, min_prob_no_hits=0.01)]
NON_MONOTONE = [(21, 50), (26, 55), (27, 52), (28, 57), (29, 33), (30, 40)]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _limits(d):
    g, _ = api.host_gap_limits(int(d.get("k", 11)), int(d.get("w", 15)), float(d.get("min_prob_no_hits", 0.1)))
    return g.astype(np.int64) + 1   # limEx of k_gap_bounds: a gap of n missing minimizers counts iff n < limEx


def _not_ascending(d):
    lim = _limits(d)
    return bool(np.any(lim[14, :] < lim.max(axis=0)))


def test_cases_reach_the_paths_off_the_default_point():
    """What the grid and the sweep are for, asserted from the table and the parameters, so that trimming them cannot quietly
    drop a path."""
    assert any(int(_limits(d).max()) > 64 for d in GRID)                           # k_gap_bounds' global-memory branch
    assert any(int(_limits(d).max()) > 64 for d in KW_CASES)
    assert all(_not_ascending(dict(k=k, w=w)) for k, w in NON_MONOTONE)             # a column that does not ascend
    assert all(any(d["k"] == k and d["w"] == w for d in KW_CASES) for k, w in NON_MONOTONE)
    assert _not_ascending(dict(k=26, w=41, min_prob_no_hits=0.01)) and not _not_ascending(dict(k=26, w=41))
    assert any(d["min_shared"] == 0 for d in GRID)                                  # top == 0 passes the MinShared rule
    assert any(d["min_fraction"] > 1 and 0 <= d["min_shared"] <= 4 for d in GRID)   # cut > top from top = 4 on
    for a, b, vals in (("min_shared", "min_fraction", (MS, MF)), ("mapped_threshold", "min_prob_no_hits", (MT, PN))):
        assert {(d[a], d[b]) for d in GRID} == {(x, y) for x in vals[0] for y in vals[1]}
    assert {d["k"] for d in KW_CASES} == set(range(10, 31))
    assert sum(w == k for k, w in KW) >= 5 and sum(w == k + 31 for k, w in KW) >= 5 and (30, 30 + 31) in KW


def _check(ctx, monkeypatch, rs, d, step=3):
    """One fast-mode case: assignments and cluster count against the oracle, the candidate tables and totalMapped of every
    `step`-th entry against the oracle's trace (a bound-rejected candidate must fail `need` on the oracle's exact total), and the
    device again without the shortcuts (IOC_RESOLVE_BOUND=0 IOC_SCORE_KEEPQ=0): the same result from at least as many
    evaluations.  Returns the oracle's batch and view."""
    a, o = param_pair(d)
    B, view = oracle_sorted_batch(rs, a.k, a.w, params=o)
    entries = list(range(0, rs.n, step))
    po.trace_set(entries, mapped_calls=True)
    try:
        ocl, ost, _ = oracle_entry_assignments(B, view)
        rows, calls = po.trace_rows(), po.trace_mapped_calls()
    finally:
        po.trace_set(())
    cls, strand, st = ctx.cluster_batch(a, view)
    bad = np.nonzero((cls != ocl) | (strand != ost))[0]
    assert not len(bad), (d, bad[:5].tolist(), cls[bad[:5]].tolist(), ocl[bad[:5]].tolist())
    assert st["n_clusters"] == B.n_clusters(), d
    n_eval = int(ctx.timings()["n_mapped_evals"])
    tgt, _, _ = ctx.decisions()
    keep = 1   # (ioc_set_params)
    if 0.0 <= a.min_fraction <= 1.0 and a.min_shared > 0:
        keep = max(1, min(int(a.min_shared * a.min_fraction), a.min_shared))
    n_rows, n_walked, n_dev = compare_candidate_tables(ctx, view, rows, calls, entries, tgt, thr=a.mapped_threshold, size_cut=keep)
    assert n_rows == len(rows["entry"])
    assert n_walked == int(np.isin(calls["entry"], entries).sum())
    assert n_dev >= n_walked
    with monkeypatch.context() as m:
        m.setenv("IOC_RESOLVE_BOUND", "0")
        m.setenv("IOC_SCORE_KEEPQ", "0")
        cls2, strand2, st2 = ctx.cluster_batch(a, view)
        assert np.array_equal(cls2, cls) and np.array_equal(strand2, strand) and st2["n_clusters"] == st["n_clusters"], d
        assert int(ctx.timings()["n_mapped_evals"]) >= n_eval, d
    return B, view


@pytest.mark.parametrize("i", range(len(GRID)))
def test_threshold_grid_fast(ctx, monkeypatch, i):
    rs = synth.generate(150 + 5 * i, 10 + i % 7, 260, 10.0, 20.0, seed=1000 + i, dup_every=2 + i % 2)
    _check(ctx, monkeypatch, rs, GRID[i])


@pytest.mark.parametrize("d", KW_CASES, ids=lambda d: f"k{d['k']}w{d['w']}p{d['min_prob_no_hits']}")
def test_kw_sweep_fast(ctx, monkeypatch, d):
    """Reads long enough that a strand holds more minimizers than the largest gap limit of the table (the head and tail extents of
    k_gap_bounds reach their end), with qualities that put the queries in error cells 11 - 15."""
    k, w = d["k"], d["w"]
    lmax = int(_limits(d).max())
    ln = int(min(16000, max(500, 1.5 * lmax * (w - k + 2) / 2)))
    rs = synth.generate(10, 3, ln, 8.0, 10.5, seed=k * 100 + w, dup_every=2)
    _check(ctx, monkeypatch, rs, dict(d, min_shared=2), step=1)


def test_min_fraction_above_one_opens_every_cluster(ctx, monkeypatch):
    """MinFraction 1.25: the reference's walk returns NEG at its first candidate once int(top * 1.25) > top (cluster.cpp:386-388),
    so on reads that normally join, every read opens a cluster of its own; 1.0 is the boundary (the top candidates pass the cut)."""
    rs = synth.generate(120, 4, 500, 12.0, 20.0, seed=77)
    B, view = oracle_sorted_batch(rs)
    oracle_entry_assignments(B, view)
    live = int((np.asarray(view["state"]) == 0).sum())
    assert live - B.n_clusters() > 50                     # the reads join at the default point
    B, view = _check(ctx, monkeypatch, rs, dict(min_fraction=1.25), step=2)
    assert B.n_clusters() == live
    B, view = _check(ctx, monkeypatch, rs, dict(min_fraction=1.0), step=2)
    assert live - B.n_clusters() > 50


ALN_CASES = ([("sahlin", at, msf) for at in (0.0, 0.05, 0.5, 0.95, 1.0, 1.5) for msf in ((2, 0.5), (5, 1.25))]
             + [("furious", at, msf) for at in (0.05, 1.0) for msf in ((2, 0.5), (5, 1.25))])


@pytest.mark.parametrize("mode,at,msf", ALN_CASES, ids=[f"{m}-a{a}-m{s[0]}f{s[1]}" for m, a, s in ALN_CASES])
def test_alignment_modes_thresholds(ctx, mode, at, msf):
    """The alignment fallback's verdict threshold (AlignedThreshold) and, with MinFraction 1.25, queries whose mapping walk stops
    at once but which still go to the alignment (cluster.cpp:553-566).  Small sets: the oracle aligns with its scalar aligner."""
    d = dict(min_shared=msf[0], min_fraction=msf[1], aligned_threshold=at)
    rs = synth.generate(60, 6, 300, 9.0, 18.0, seed=int(at * 100) + 7 * msf[0], dup_every=2)
    a, o = param_pair(d, mode)
    B, view = oracle_sorted_batch(rs, params=o)
    ocl, ost, _ = oracle_entry_assignments(B, view, mode=mode)
    cls, strand, st = ctx.cluster_batch(a, fz._with_sequences(rs, view))
    bad = np.nonzero((cls != ocl) | (strand != ost))[0]
    assert not len(bad), (d, mode, bad[:5].tolist(), cls[bad[:5]].tolist(), ocl[bad[:5]].tolist())
    assert st["n_clusters"] == B.n_clusters()


MERGE_CASES = [
    dict(n=160, g=8, ln=400, qlo=9.0, qhi=20.0, dup=2, jit=0.0, k=11, w=15, seed=5101, mode="fast",
         params=dict(min_shared=1, min_fraction=0.5, mapped_threshold=0.9, min_prob_no_hits=0.01)),
    dict(n=140, g=6, ln=600, qlo=8.0, qhi=11.0, dup=0, jit=0.3, k=21, w=50, seed=5102, mode="fast",
         params=dict(min_shared=2, min_fraction=1.25, mapped_threshold=0.3)),
    dict(n=120, g=5, ln=500, qlo=10.0, qhi=18.0, dup=3, jit=0.0, k=13, w=44, seed=5103, mode="fast",
         params=dict(min_shared=0, min_fraction=0.0, mapped_threshold=0.99, min_prob_no_hits=1e-4)),
]


@pytest.mark.parametrize("i", range(len(MERGE_CASES)))
def test_merge_off_default(ctx, i):
    ok, why = fz.run_parity(ctx, MERGE_CASES[i], merge=True)
    assert ok, f"{why}  --case \"{MERGE_CASES[i]}\""


def test_consensus_off_default(ctx):
    """ioc_consensus.cpp derives the Size from which an entry can see a changed representative from MinShared and MinFraction."""
    c = dict(n=150, g=6, ln=500, cmax=6, cmin=3, period=25, seed=5201, dup=2, mode="fast", qlo=11, qhi=22,
             params=dict(min_shared=2, min_fraction=0.5))
    ok, why = fz.run_consensus(ctx, c)
    assert ok, f"{why}  {c}"


def test_cli_off_default_matches_oracle(tmp_path):
    from tests.test_cli import sort_cluster_merge_dump_vs_oracle
    rs = synth.generate(200, 20, 900, 9, 16, seed=23)
    sort_cluster_merge_dump_vs_oracle(tmp_path, "fast", rs, dict(k=21, w=50, min_shared=2, min_fraction=0.6,
                                                                 mapped_threshold=0.8, min_prob_no_hits=0.05))


def test_cli_refuses_batches_sorted_with_different_parameters(tmp_path):
    from tests.test_cli import _write_fastq, run
    rs = synth.generate(60, 6, 400, 10, 20, seed=29)
    fq = tmp_path / "reads.fq"
    _write_fastq(rs, fq)
    cl = []
    for i, r in enumerate(("0.65", "0.8")):
        out = tmp_path / f"s{i}"
        res = run("sort", "-r", r, "-o", str(out), str(fq))
        assert res.returncode == 0, res.stderr
        res = run("cluster", "-l", str(out / "batches" / "isONbatch_0.cer"), "-o", str(tmp_path / f"c{i}.cer"), "-x", "fast")
        assert res.returncode == 0, res.stderr
        cl.append(tmp_path / f"c{i}.cer")
    res = run("cluster", "-l", str(cl[0]), "-r", str(cl[1]), "-o", str(tmp_path / "m.cer"), "-x", "fast")
    assert res.returncode == 1
    assert "sorted with different parameters" in res.stderr



def _reads(pairs):
    seq = np.frombuffer(b"".join(a for a, _ in pairs), np.uint8).copy()
    qual = np.frombuffer(b"".join(b for _, b in pairs), np.uint8).copy()
    offs = np.zeros(len(pairs) + 1, np.int64)
    offs[1:] = np.cumsum([len(a) for a, _ in pairs])
    return synth.ReadSet(seq=seq, qual=qual, offs=offs, transcript=np.zeros(len(pairs), np.int32),
                         strand=np.ones(len(pairs), np.int8), tag="hand-built")


def test_bound_reproducer_non_ascending_column(ctx, monkeypatch):
    """Two hand-built reads at (k, w) = (21, 50), MinShared 1, MappedThreshold 0.99: a representative in error cell 14 and a
    query in cell 11 (225 minimizers on its forward strand) that share ONE minimizer, the query's 113th (index 112).  limEx of
    column 11 ends 82, 113, 111: the reference counts the head (112 < 113) and the tail (225 - 113 < 113) of that single hit, so
    totalMapped = hpcLen and the query joins.  A bound whose head and tail extents stop at lim[14] = 111 minimizers is
    p[110] + hpcLen - p[114], below `need`: the candidate would be rejected without an evaluation."""
    rng = np.random.default_rng(5)
    acgt = np.frombuffer(b"ACGT", np.uint8)

    def rnd(n):
        return acgt[rng.integers(0, 4, n)].tobytes()

    q = rnd(4700)
    qq = np.full(len(q), 33 + 10, np.uint8)
    qq[rng.random(len(q)) < 0.386] = 33 + 9
    qq = qq.tobytes()
    d = dict(k=21, w=50, min_shared=1, mapped_threshold=0.99)
    _, view = oracle_sorted_batch(_reads([(q, qq)]), 21, 50, params=param_pair(d)[1])
    pos = view["min_pos"][view["off_fwd"][0]:view["off_fwd"][1]]
    assert len(pos) == 225
    # the raw stretch of the query's minimizer 112 (positions are HPC coordinates: the start of every run of equal bases)
    qa = np.frombuffer(q, np.uint8)
    starts = np.concatenate([[0], np.nonzero(qa[1:] != qa[:-1])[0] + 1])
    P = int(pos[112])
    s, e = int(starts[P]), int(starts[P + 21])
    pad = int(rng.integers(0, 30))
    rep = rnd(2600) + q[s - pad:e + pad] + rnd(2600)
    nl = int(len(rep) * 0.44)   # error cell 14 with the larger score: a clean half and a noisy one
    rq = bytes([33 + 40]) * (len(rep) - nl) + bytes([33 + 5]) * nl
    rs = _reads([(q, qq), (rep, rq)])
    B, view = oracle_sorted_batch(rs, 21, 50, params=param_pair(d)[1])
    assert view["orig"].tolist() == [1, 0]
    assert [api.host_err_cell(x) for x in view["hpc_err"]] == [14, 11]
    lim = _limits(d)
    assert lim[13, 10] == 113 and lim[14, 10] == 111
    po.trace_set([1], mapped_calls=True)
    try:
        ocl, ost, _ = oracle_entry_assignments(B, view)
        rows = po.trace_rows()
    finally:
        po.trace_set(())
    hl = int(view["hpc_len"][1])
    assert rows["size"].tolist() == [1] and rows["first_index"].tolist() == [112] and rows["strand"].tolist() == [1]
    assert rows["total_mapped"].tolist() == [hl] and rows["walked"].tolist() == [1]
    assert ocl.tolist() == [0, 0] and B.n_clusters() == 1
    p = view["min_pos"][view["off_fwd"][1]:view["off_fwd"][2]]
    assert int(p[110]) + hl - int(p[114]) < api.host_min_total(hl, 0.99)
    _check(ctx, monkeypatch, rs, d, step=1)
