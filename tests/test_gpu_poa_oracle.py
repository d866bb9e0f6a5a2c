"""The product's POA engine (isonclust2_amd/csrc/ioc_poa.hip: sequence-to-graph DP and traceback on the GPU, graphs and
heaviest-bundle consensus on the host) against the ORACLE's scalar POA (oracle/poa_oracle.cpp: an independent restatement
of the published algorithm in the shape of spoa 4.0's scalar engine and graph — src/consensus.cpp:15-32, 91, 128-137,
src/main.cpp:285-324).  Both stores are fed the same operations; compared after EVERY addition: the alignment (score and
every (node, position) pair) and, per graph, the nodes' letters, the edges with their weights, the topological order and the
consensus string.  "Parity with the oracle's POA; spoa unpinned" (its source is absent from the reference tree).

All three alignment types of `cluster -A`: the four workloads written for local alignment run under global and
semi-global alignment too (`*_off_local`), and after them the shapes that only matter there: rows 0 and columns 0 longer than a
tile and a wave carry, gaps of 300+ bases that no zero floor cuts, graphs with several sources and sinks, unrelated reads.  The
oracle's types are pinned on the CPU by tests/test_oracle_poa_modes.py."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import api
from oracle import pyoracle as po
from tests.poa_common import mutate, random_addition
from tests.poa_modes_common import GLOBAL, LOCAL, SEMI_GLOBAL
from tests.test_gpu_poa import Poa
from tests.test_gpu_poa_modes import ModePoa

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


OFF_LOCAL = [GLOBAL, SEMI_GLOBAL]


def _stores(ctx, t, **sc):
    """the engine and the oracle under alignment type t (sc: scores other than the reference's, test_gpu_poa_params.py)"""
    return (Poa(ctx, **sc) if t == LOCAL else ModePoa(ctx, t, **sc)), po.OraclePoa(mode=t, **sc)


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _longest_run(a, value):
    best = cur = 0
    for x in a.tolist():
        cur = cur + 1 if x == value else 0
        best = max(best, cur)
    return best


def _copy_engine_graph(src, idx, dst, to_idx, to_side=0):
    """ioc_poa_graph_save -> ioc_poa_graph_load: a graph does not record the type that built it"""
    L = src.L
    n = L.ioc_poa_graph_save(src.h, 0, idx, None, C.c_int64(0))
    assert n > 0
    buf = (C.c_uint8 * n)()
    assert L.ioc_poa_graph_save(src.h, 0, idx, buf, C.c_int64(n)) == n
    assert L.ioc_poa_graph_load(dst.h, to_side, to_idx, buf, C.c_int64(n)) == 0


def _edges(ef, et, ew):
    return sorted(zip(ef.tolist(), et.tolist(), ew.tolist()))


def _same_graph(dev, orc, idx, tag):
    db, dr, def_, det, dew = dev.graph(idx)
    ob, orr, oef, oet, oew = orc.graph(idx)
    assert db == ob, (tag, "letters")
    assert _edges(def_, det, dew) == _edges(oef, oet, oew), (tag, "edges / weights")
    assert dr.tolist() == orr.tolist(), (tag, "topological order")
    assert dev.size(idx) == orc.size(idx), (tag, "sequences")
    assert dev.consensus(idx) == orc.consensus(idx), (tag, "consensus")


def _same_alignment(dev, orc, tag):
    dn, dp, ds = dev.last_alignment()
    on, op, os_ = orc.last_alignment()
    assert ds == os_, (tag, "score", ds, os_)
    first = next((x for x in range(min(len(dn), len(on))) if dn[x] != on[x] or dp[x] != op[x]), None)
    assert first is None and len(dn) == len(on), (tag, "alignment differs at pair", first, len(dn), len(on),
                                                  None if first is None else (dn[first - 2:first + 3].tolist(), dp[first - 2:first + 3].tolist(),
                                                                              on[first - 2:first + 3].tolist(), op[first - 2:first + 3].tolist()))


def _add_both(dev, orc, idx, r, tag, w=1):
    dev.add(idx, r, w=w)
    orc.add(idx, r, w=w)
    _same_alignment(dev, orc, tag)
    _same_graph(dev, orc, idx, tag)


def _random_additions(ctx, poa_type):
    rng = random.Random(41)
    adds = 0
    for g in range(34):
        dev, orc = _stores(ctx, poa_type)
        ln = rng.choice([40, 90, 200, 260, 330, 700])
        truth = bytes(rng.choice(b"ACGT") for _ in range(ln))
        first = mutate(rng, truth, rng.choice([0.0, 0.05, 0.15]))
        dev.create(0, first)
        orc.create(0, first)
        _same_graph(dev, orc, 0, (g, "seed"))
        for t in range(rng.randint(4, 9)):
            r = random_addition(rng, truth, t)
            if not r:
                continue
            w = 1 + t % 3
            dev.add(0, r, w=w)
            orc.add(0, r, w=w)
            adds += 1
            _same_alignment(dev, orc, (g, t))
            _same_graph(dev, orc, 0, (g, t))
        dev.close()
        orc.close()
    assert adds >= 200


def test_random_additions_give_the_oracles_graphs(ctx):
    _random_additions(ctx, LOCAL)


@pytest.mark.parametrize("t", OFF_LOCAL)
def test_random_additions_give_the_oracles_graphs_off_local(ctx, t):
    _random_additions(ctx, t)


def _low_complexity(ctx, poa_type, **sc):
    rng = random.Random(43)
    for g in range(12):
        dev, orc = _stores(ctx, poa_type, **sc)
        unit = bytes(rng.choice(b"AC") for _ in range(rng.choice([2, 3, 5])))
        truth = (unit * 80)[: rng.choice([60, 150, 240])]
        dev.create(0, truth)
        orc.create(0, truth)
        for t in range(6):
            r = mutate(rng, truth, 0.08) if t % 2 else (unit * 80)[: rng.randint(20, len(truth))]
            dev.add(0, r, w=1 + t % 2)
            orc.add(0, r, w=1 + t % 2)
            _same_alignment(dev, orc, (g, t))
            _same_graph(dev, orc, 0, (g, t))
        dev.close()
        orc.close()


def test_low_complexity_and_tie_heavy_reads(ctx):
    """Repeats and two-letter sequences: many alignments of equal score, so the tie rules (first maximum, diagonal before the
    gaps, first predecessor, extension before opening) decide the graph."""
    _low_complexity(ctx, LOCAL)


@pytest.mark.parametrize("t", OFF_LOCAL)
def test_low_complexity_and_tie_heavy_reads_off_local(ctx, t):
    """... and the first maximum among the END cells: a read that is a prefix of a repeat ends with the same score in many rows"""
    _low_complexity(ctx, t)


def _purge_and_unrelated(ctx, poa_type):
    rng = random.Random(47)
    dev, orc = _stores(ctx, poa_type)
    truth = bytes(rng.choice(b"ACGT") for _ in range(300))
    dev.create(3, truth)
    orc.create(3, truth)
    for t in range(5):
        r = mutate(rng, truth, 0.1)
        dev.add(3, r)
        orc.add(3, r)
    cons = orc.consensus(3)
    assert dev.consensus(3) == cons
    assert dev.ops.purge(dev.ops.user, 0, 3, C.cast(C.c_char_p(cons), C.POINTER(C.c_char)), len(cons), 6) == 0
    orc.purge(3, cons, w=6)
    _same_graph(dev, orc, 3, "purged")
    other = b"T" * 40            # nothing in common with anything at m 4 / n -8? (single matches score 4: local alignment of one base)
    dev.add(3, other)
    orc.add(3, other)
    _same_alignment(dev, orc, "unrelated")
    _same_graph(dev, orc, 3, "unrelated")
    dev.close()
    orc.close()


def test_purge_and_unrelated_reads(ctx):
    """ConsPurge (src/consensus.cpp:128-137) restarts a graph from the representative with the old count as weight; a read that
    shares nothing with the graph has score 0 and is added as a chain of its own."""
    _purge_and_unrelated(ctx, LOCAL)


@pytest.mark.parametrize("t", OFF_LOCAL)
def test_purge_and_unrelated_reads_off_local(ctx, t):
    _purge_and_unrelated(ctx, t)


def _longer_than_a_tile_column(ctx, poa_type):
    rng = random.Random(53)
    for g, ln in enumerate([2101, 2302, 2563, 2048]):
        dev, orc = _stores(ctx, poa_type)
        truth = bytearray(rng.choice(b"ACGT") for _ in range(ln))
        truth[1000:1050] = (b"AC" * 25)
        truth = bytes(truth)
        first = mutate(rng, truth, 0.05)
        dev.create(0, first)
        orc.create(0, first)
        for t in range(5):
            r = mutate(rng, truth, rng.choice([0.03, 0.1]))
            if t == 2:
                a = rng.randint(900, 1100)
                r = r[:a] + r[a + rng.randint(30, 80):]
            if t == 3:
                r = r[rng.randint(0, 300): len(r) - rng.randint(0, 300)]
            dev.add(0, r, w=1 + t % 2)
            orc.add(0, r, w=1 + t % 2)
            _same_alignment(dev, orc, (g, t))
            _same_graph(dev, orc, 0, (g, t))
        dev.close()
        orc.close()


def test_reads_longer_than_a_tile_column(ctx):
    """2.1 - 2.6 kb reads (row widths of every residue mod 4: the cell arrays' pitch is padded) against graphs 35+ tile rows
    deep: the row carries (prefix maxima, strict-maximum flags, boundary H) cross waves AND column tiles, deletions of 30 - 80
    bases put edges across tile rows, a low-complexity stretch sits on the tile edge at column 1024."""
    _longer_than_a_tile_column(ctx, LOCAL)


@pytest.mark.parametrize("t", OFF_LOCAL)
def test_reads_longer_than_a_tile_column_off_local(ctx, t):
    """... with row 0 = gap(j) across every column tile and wave carry, and no floor under the deletions"""
    _longer_than_a_tile_column(ctx, t)


# ---- shapes that only matter off local alignment ---------------------------------------------------------------------------
@pytest.mark.parametrize("t", OFF_LOCAL)
def test_very_unequal_lengths(ctx, t):
    """A 40-node graph against 1500-base reads and a 1500-node graph against 30-base reads: global alignment walks row 0 and
    column 0 for more than 64, 256 and 1024 cells (the fill at the end of the traceback, a column tile, a wave carry, 16 tile
    rows); semi-global alignment leaves the same stretches to the unaligned head or ends in column L of a row far from a sink."""
    rng = random.Random(61 + t)
    small = _rand(rng, 40)
    dev, orc = _stores(ctx, t)
    dev.create(0, small)
    orc.create(0, small)
    _add_both(dev, orc, 0, mutate(rng, small, 0.1), "small graph, second read")
    assert len(orc.graph(0)[0]) < 64
    long_reads = [_rand(rng, 1100) + small + _rand(rng, 360),        # the graph's letters after more than 1024 columns of row 0
                  small + _rand(rng, 1460),                            # ... at the head: the rest is one horizontal run to column L
                  _rand(rng, 1500)]                                    # nothing in common
    for k, r in enumerate(long_reads):
        d2, o2 = _stores(ctx, t)                                      # (each against the same small graph, not against its predecessors' nodes)
        orc.copy_graph_to(0, o2, 0, 0)
        _copy_engine_graph(dev, 0, d2, 0)
        _same_graph(d2, o2, 0, ("small graph copied", k))
        _add_both(d2, o2, 0, r, ("1500-base read", k))
        if t == GLOBAL:
            nodes, pos, _ = o2.last_alignment()
            assert k == 2 or _longest_run(nodes, -1) > 1024
        d2.close()
        o2.close()
    dev.close()
    orc.close()
    big = _rand(rng, 1500)
    dev, orc = _stores(ctx, t)
    dev.create(0, big)
    orc.create(0, big)
    for k, r in enumerate([big[1200:1230], big[5:35], big[700:730], mutate(rng, big[1465:], 0.1)]):
        _add_both(dev, orc, 0, r, ("30-base read", k))
        if t == GLOBAL and k == 0:
            nodes, pos, _ = orc.last_alignment()
            assert _longest_run(pos, -1) > 1024
    dev.close()
    orc.close()


@pytest.mark.parametrize("t", OFF_LOCAL)
def test_long_insertion_and_long_deletion_in_a_2kb_read(ctx, t):
    """A 330-base insertion that starts before column 1024 and ends after it (one row, across a wave carry and two column
    tiles) and 320 / 340 / 310-base deletions at columns 1024, ~ 500 and ~ 1800 (five tile rows in one column): no zero floor cuts a long
    gap, it is the second affine piece (q, c) all the way, and the score stays below what came before it."""
    rng = random.Random(67 + t)
    truth = _rand(rng, 2000)
    dev, orc = _stores(ctx, t)
    first = mutate(rng, truth, 0.04)
    dev.create(0, first)
    orc.create(0, first)
    reads = [truth[:860] + _rand(rng, 330) + truth[860:],
             truth[:1024] + truth[1024 + 320:],
             mutate(rng, truth[:500], 0.03) + mutate(rng, truth[840:], 0.03),      # (not where the read before left an edge to take)
             mutate(rng, truth[:900], 0.03) + _rand(rng, 310) + mutate(rng, truth[900:1500], 0.03) + mutate(rng, truth[1810:], 0.03)]
    for k, r in enumerate(reads):
        _add_both(dev, orc, 0, r, ("long gap", k), w=1 + k % 2)
        nodes, pos, _ = orc.last_alignment()
        inner = slice(50, len(nodes) - 50)                          # (inside the alignment: not a head or a tail)
        if k in (0, 3):
            assert _longest_run(nodes[inner], -1) >= 300, k
        if k in (1, 2, 3):
            assert _longest_run(pos[inner], -1) >= 300, k
    dev.close()
    orc.close()


def _sources_and_sinks(store, idx):
    bases, rank, ef, et, ew = store.graph(idx)
    n = len(bases)
    return n - len(set(et.tolist())), n - len(set(ef.tolist()))


@pytest.mark.parametrize("t", OFF_LOCAL)
def test_several_sources_and_sinks(ctx, t):
    """Semi-global additions of truth + tail A, truth + tail B, head C + truth leave two tails and a head hanging off the
    truth; head C becomes the only source (AddAlignment links the unaligned head to the first aligned node), so head D +
    truth[60:] follows: it starts in column 0 of an inner row and its head is a second source (asserted from the exported
    graph).  Reads that end at the fork, that equal a branch, and the truth itself then have
    equal maxima in different sink rows and in column L of rows that are no sinks.  Global additions never make a second
    source or sink, so for type 1 that graph is copied into global stores: end cells in column L of several sinks, column 0
    reached from several sources."""
    rng = random.Random(71)
    truth = _rand(rng, 180, b"ACG")                                   # (no T: head D cannot match anything, it is one insertion)
    tail_a, tail_b, head_c, head_d = _rand(rng, 60, b"AC"), _rand(rng, 60, b"GT"), _rand(rng, 50), b"T" * 45
    dev, orc = _stores(ctx, SEMI_GLOBAL)
    dev.create(0, truth)
    orc.create(0, truth)
    for k, r in enumerate([truth + tail_a, truth + tail_b, head_c + truth, head_d + truth[60:]]):
        _add_both(dev, orc, 0, r, ("building", k))
    sources, sinks = _sources_and_sinks(orc, 0)
    assert sources >= 2 and sinks >= 2, (sources, sinks)
    assert _sources_and_sinks(dev, 0) == (sources, sinks)
    if t == GLOBAL:
        d2, o2 = _stores(ctx, GLOBAL)
        orc.copy_graph_to(0, o2, 0, 0)
        _copy_engine_graph(dev, 0, d2, 0)
        dev.close()
        orc.close()
        dev, orc = d2, o2
        _same_graph(dev, orc, 0, "copied")
    reads = [truth, truth + tail_a, truth + tail_b, head_c + truth, truth[:-1], truth[40:], truth[40:] + tail_b[:30],
             head_c[20:] + truth[:100], head_c + truth + tail_a, truth + tail_a[:25] + tail_b[25:], mutate(rng, truth, 0.1),
             tail_a, tail_b[10:], head_c, head_d + truth[60:], truth[60:], head_d[30:] + truth[60:120]]
    for k, r in enumerate(reads):
        _add_both(dev, orc, 0, r, ("read", k), w=1 + k % 2)
    dev.close()
    orc.close()


@pytest.mark.parametrize("t", [LOCAL, GLOBAL, SEMI_GLOBAL])
def test_unrelated_read(ctx, t):
    """A random read against a random graph, and a read without one letter of the graph.  Global: every base is aligned, the
    score is strongly negative.  Semi-global: whatever the rules give (the best end cell may be column 0 of a sink: an empty
    alignment, the read becomes a component of its own) — the same on both sides."""
    rng = random.Random(73)
    dev, orc = _stores(ctx, t)
    for g, (graph, read) in enumerate([(_rand(rng, 300), _rand(rng, 120)), (_rand(rng, 150, b"AC"), _rand(rng, 90, b"GT")),
                                        (_rand(rng, 90, b"AC"), _rand(rng, 400, b"GT"))]):
        dev.create(g, graph)
        orc.create(g, graph)
        _add_both(dev, orc, g, mutate(rng, graph, 0.05), (g, "related"))
        _add_both(dev, orc, g, read, (g, "unrelated"))
        score = orc.last_alignment()[2]
        if t != GLOBAL:
            assert score >= 0, (g, score)               # (local: the floor; semi-global: column 0 of a sink is an end cell)
        elif g >= 1:
            assert score < -200, (g, score)             # (no letter in common: at best every node and every base in a gap)
        _add_both(dev, orc, g, mutate(rng, read, 0.05), (g, "its copy"))
    dev.close()
    orc.close()


@pytest.mark.parametrize("t", OFF_LOCAL)
def test_tiny_graphs_and_reads(ctx, t):
    """the by-hand cases of tests/test_oracle_poa_modes.py (one node, one base, reads shorter and longer than the graph, an empty
    alignment, equal maxima in two end rows) through the engine: graphs far below one tile, alignments of zero or one pair"""
    cases = [[b"ACGT", b"TTACGT", b"GGACGT"], [b"TTACGT", b"ACGT", b"T"], [b"AAAA", b"CCC", b"CCC", b"AAAACCC"], [b"A", b"A", b"C", b"C", b"AC"],
             [b"ACAC", b"AC", b"CA"], [b"ACG", b"ACT", b"AC", b"ACT", b"A"], [b"G", b"ACGTACGTAC", b"G"]]
    dev, orc = _stores(ctx, t)
    for g, reads in enumerate(cases):
        dev.create(g, reads[0])
        orc.create(g, reads[0])
        _same_graph(dev, orc, g, (g, "seed"))
        for k, r in enumerate(reads[1:]):
            _add_both(dev, orc, g, r, (g, k))
    dev.close()
    orc.close()
