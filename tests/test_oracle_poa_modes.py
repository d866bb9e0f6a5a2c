"""The oracle's scalar POA under global and semi-global alignment (oracle/poa_oracle.cpp, OraclePoa(mode=1 | 2)) checked on
the CPU against what is stated without it: tests/poa_modes_common.py (the recurrence per type, itself pinned to a brute force
over paths by test_poa_modes_host.py), the path scorer and boundary rules there, the brute force directly on small graphs,
and pair lists worked out by hand from the rules in the oracle's header.  Only then is the oracle a checker of the engine
(tests/test_gpu_poa_oracle.py).  spoa is absent from the reference tree: this pins the oracle's statement, not spoa."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import pyoracle as po
from tests.poa_common import mutate, random_addition
from tests.poa_modes_common import (GLOBAL, LOCAL, SEMI_GLOBAL, boundary_violations, brute_force, gap, mode_path_score,
                                    mode_score)

MODES = [GLOBAL, SEMI_GLOBAL]


def _pairs(P):
    nodes, pos, score = P.last_alignment()
    return list(zip(nodes.tolist(), pos.tolist())), score


def _edges(P, idx=0):
    bases, rank, ef, et, ew = P.graph(idx)
    return sorted(zip(ef.tolist(), et.tolist(), ew.tolist()))


def _check_graph_invariants(P, idx, total_weight):
    """test_oracle_poa.py's: the order is a permutation that respects every edge; and every base of every read but its first
    gave one edge 2 w, so the weights sum to 2 w (len - 1) over the reads"""
    bases, rank, ef, et, ew = P.graph(idx)
    order = {int(v): i for i, v in enumerate(rank)}
    assert sorted(rank.tolist()) == list(range(len(bases)))
    assert all(order[int(a)] < order[int(b)] for a, b in zip(ef, et))
    assert len(set(zip(ef.tolist(), et.tolist()))) == len(ef)               # an edge exists once
    assert int(ew.sum()) == total_weight


@pytest.mark.parametrize("mode", MODES)
def test_score_and_path_equal_the_plain_statement(mode):
    rng = random.Random(5 + mode)
    adds = 0
    for g in range(14):
        P = po.OraclePoa(mode=mode)
        truth = bytes(rng.choice(b"ACGT") for _ in range(rng.choice([40, 90, 200])))
        first = mutate(rng, truth, 0.05)
        P.create(0, first)
        total, n_seq = 2 * (len(first) - 1), 1
        for t in range(rng.randint(4, 8)):
            r = random_addition(rng, truth, t)
            if not r:
                continue
            bases, rank, ef, et, ew = P.graph(0)
            want = mode_score(bases, rank, ef, et, r, mode)
            w = 1 + t % 3
            P.add(0, r, w=w)
            nodes, pos, score = P.last_alignment()
            adds += 1
            assert score == want, (g, t, score, want)
            assert mode_path_score(bases, ef, et, r, nodes, pos, mode) == score, (g, t)
            assert boundary_violations(ef, et, len(bases), len(r), nodes, pos, mode) == [], (g, t)
            total += 2 * w * (len(r) - 1)
            _check_graph_invariants(P, 0, total)
            n_seq += 1
            assert P.size(0) == n_seq
        P.close()
    assert adds > 50


@pytest.mark.parametrize("mode", MODES)
def test_small_graphs_equal_the_brute_force(mode):
    """graphs of 2 - 4 reads of at most 6 bases, built under the type (semi-global ones get extra sources and sinks), then
    one more read: the score is the best over every source-to-sink path of the plain sequence-to-sequence DP"""
    rng = random.Random(17 + mode)
    several = 0
    for case in range(300):
        P = po.OraclePoa(mode=mode)
        alphabet = b"ACGT" if case % 2 else b"AC"
        reads = [bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 6))) for _ in range(rng.randint(2, 4))]
        P.create(0, reads[0])
        for r in reads[1:]:
            bases, rank, ef, et, ew = P.graph(0)
            P.add(0, r)
            nodes, pos, score = P.last_alignment()
            assert score == brute_force(bases, ef, et, r, mode), (case, reads, r)
            assert mode_path_score(bases, ef, et, r, nodes, pos, mode) == score, (case, reads, r)
            assert boundary_violations(ef, et, len(bases), len(r), nodes, pos, mode) == [], (case, reads, r)
        bases, rank, ef, et, ew = P.graph(0)
        several += len(set(range(len(bases))) - set(ef.tolist())) > 1
        P.close()
    assert several > 20                                                      # (graphs with more than one sink were among them)


def test_global_by_hand_read_head_on_row_0():
    P = po.OraclePoa(mode=GLOBAL)
    P.create(0, b"ACGT")
    P.add(0, b"TTACGT")
    assert _pairs(P) == ([(-1, 0), (-1, 1), (0, 2), (1, 3), (2, 4), (3, 5)], 16 + gap(2))
    bases, rank, ef, et, ew = P.graph(0)
    assert bases == b"ACGTTT"                                                # the head's two bases are new nodes 4, 5
    assert _edges(P) == [(0, 1, 4), (1, 2, 4), (2, 3, 4), (4, 5, 2), (5, 0, 2)]
    assert rank.tolist() == [4, 5, 0, 1, 2, 3]
    P.close()


def test_semi_global_by_hand_read_head_left_to_add_alignment():
    P = po.OraclePoa(mode=SEMI_GLOBAL)
    P.create(0, b"ACGT")
    P.add(0, b"GGACGT")
    assert _pairs(P) == ([(0, 2), (1, 3), (2, 4), (3, 5)], 16 + gap(2))     # four pairs: the head is not in the alignment
    bases, rank, ef, et, ew = P.graph(0)
    assert bases == b"ACGTGG"                                                # ... and comes in as AddAlignment's prefix chain
    assert _edges(P) == [(0, 1, 4), (1, 2, 4), (2, 3, 4), (4, 5, 2), (5, 0, 2)]
    assert rank.tolist() == [4, 5, 0, 1, 2, 3]
    P.close()


def test_semi_global_by_hand_tie_between_columns_of_the_sink():
    """TTACGT against A-C-G-T: the four matches after the head cost 16 + gap(2) = 4 in column 6 of the sink's row, and the
    read's first T on the sink alone gives 4 in column 1 of the same row.  Every column of a sink is an end cell and the first
    maximum in (row, column) order wins: one pair, and the five bases after it are AddAlignment's unaligned tail."""
    P = po.OraclePoa(mode=SEMI_GLOBAL)
    P.create(0, b"ACGT")
    P.add(0, b"TTACGT")
    assert _pairs(P) == ([(3, 0)], 4)
    bases, rank, ef, et, ew = P.graph(0)
    assert bases == b"ACGTTACGT"
    assert _edges(P) == [(0, 1, 2), (1, 2, 2), (2, 3, 2), (3, 4, 2), (4, 5, 2), (5, 6, 2), (6, 7, 2), (7, 8, 2)]
    P.close()


def test_global_by_hand_graph_head_on_column_0():
    """a read shorter than the graph: TT of the graph is passed on column 0, as (node, -1) pairs"""
    P = po.OraclePoa(mode=GLOBAL)
    P.create(0, b"TTACGT")
    P.add(0, b"ACGT")
    assert _pairs(P) == ([(0, -1), (1, -1), (2, 0), (3, 1), (4, 2), (5, 3)], 16 + gap(2))
    assert _edges(P) == [(0, 1, 2), (1, 2, 2), (2, 3, 4), (3, 4, 4), (4, 5, 4)]
    P.add(0, b"T")                                                           # five nodes on column 0 (the second piece: gap(5) = -24), then the sink
    assert _pairs(P) == ([(0, -1), (1, -1), (2, -1), (3, -1), (4, -1), (5, 0)], 4 + gap(5))
    P.close()
    S = po.OraclePoa(mode=SEMI_GLOBAL)                                       # the same read under semi-global: the graph's head is free
    S.create(0, b"TTACGT")
    S.add(0, b"ACGT")
    assert _pairs(S) == ([(2, 0), (3, 1), (4, 2), (5, 3)], 16)
    S.close()


def test_semi_global_by_hand_unrelated_read():
    """every diagonal is a mismatch and column L costs gap or mismatches; column 0 of the sink is 0 and the only end cell that
    is not negative: an empty alignment, the read becomes a component of its own (a second source and a second sink)"""
    P = po.OraclePoa(mode=SEMI_GLOBAL)
    P.create(0, b"AAAA")
    P.add(0, b"CCC")
    assert _pairs(P) == ([], 0)
    bases, rank, ef, et, ew = P.graph(0)
    assert bases == b"AAAACCC" and P.size(0) == 2
    assert _edges(P) == [(0, 1, 2), (1, 2, 2), (2, 3, 2), (4, 5, 2), (5, 6, 2)]
    assert rank.tolist() == [0, 1, 2, 3, 4, 5, 6]
    G = po.OraclePoa(mode=GLOBAL)                                            # global: every base aligned, three mismatches and one node skipped
    G.create(0, b"AAAA")
    G.add(0, b"CCC")
    pairs, score = _pairs(G)
    assert score == 3 * -8 + gap(1) and [p for _, p in pairs if p >= 0] == [0, 1, 2]
    assert pairs == [(0, -1), (1, 0), (2, 1), (3, 2)]                        # diagonal first from the end cell: the gap is at the head
    G.close()


@pytest.mark.parametrize("mode", MODES)
def test_one_base_against_one_node(mode):
    P = po.OraclePoa(mode=mode)
    P.create(0, b"A")
    P.add(0, b"A")
    assert _pairs(P) == ([(0, 0)], 4)
    bases, rank, ef, et, ew = P.graph(0)
    assert bases == b"A" and len(ef) == 0 and P.size(0) == 2
    P.add(0, b"C")
    if mode == GLOBAL:                         # a mismatch (-8) beats two gaps (-16): C becomes an aligned node of A
        assert _pairs(P) == ([(0, 0)], -8)
        bases, rank, ef, et, ew, al = P.graph(0, aligned=True)
        assert bases == b"AC" and al == [[1], [0]]
    else:                                      # column 0 of the sink is 0, column 1 is -8: empty, C is a node of its own
        assert _pairs(P) == ([], 0)
        bases, rank, ef, et, ew, al = P.graph(0, aligned=True)
        assert bases == b"AC" and al == [[], []]
    P.close()


def test_equal_maxima_in_different_end_rows_the_earlier_row_wins():
    # semi-global, column L of two rows: AC ends with 8 in the rows of node 1 and of node 3 (the sink)
    P = po.OraclePoa(mode=SEMI_GLOBAL)
    P.create(0, b"ACAC")
    P.add(0, b"AC")
    assert _pairs(P) == ([(0, 0), (1, 1)], 8)
    assert _edges(P) == [(0, 1, 4), (1, 2, 2), (2, 3, 2)]
    P.close()
    # semi-global: ACT against A-C-G.  0 in column 3 of C's row (AC matched, T inserted), in columns 0 and 2 and 3 of the
    # sink G; C's row comes first, so T is inserted after C: a new node 3 and a second sink
    P = po.OraclePoa(mode=SEMI_GLOBAL)
    P.create(0, b"ACG")
    P.add(0, b"ACT")
    assert _pairs(P) == ([(0, 0), (1, 1), (-1, 2)], 0)
    bases, rank, ef, et, ew = P.graph(0)
    assert bases == b"ACGT" and _edges(P) == [(0, 1, 4), (1, 2, 2), (1, 3, 2)] and rank.tolist() == [0, 1, 2, 3]
    # global over that graph (two sinks: column L of both rows): AC ends with 8 + gap(1) under G and under T; G's row is first
    Q = po.OraclePoa(mode=GLOBAL)
    P.copy_graph_to(0, Q, 0, 0)
    Q.add(0, b"AC")
    assert _pairs(Q) == ([(0, 0), (1, 1), (2, -1)], 0)
    Q.add(0, b"ACT")                           # (and the later sink is taken when it is better)
    assert _pairs(Q) == ([(0, 0), (1, 1), (3, 2)], 12)
    P.close()
    Q.close()


class _PlainCreate(po.OraclePoa):
    """a store made by orp_create, the entry point that existed before the types"""

    def __init__(self):
        super().__init__()
        self.L.orp_destroy(self.h)
        sc = self.SC
        self.h = self.L.orp_create(sc["m"], sc["n"], sc["g"], sc["e"], sc["q"], sc["c"])
        self.L.orp_bind(self.h, C.addressof(self.ops))


def test_type_0_through_orp_create_mode_is_orp_create():
    """the workload of test_oracle_poa.py through both entry points: the same alignments, graphs and consensus"""
    rng = random.Random(5)
    for g in range(12):
        A, B = _PlainCreate(), po.OraclePoa(mode=LOCAL)
        truth = bytes(rng.choice(b"ACGT") for _ in range(rng.choice([40, 90, 200])))
        first = mutate(rng, truth, 0.05)
        A.create(0, first)
        B.create(0, first)
        for t in range(rng.randint(4, 8)):
            r = random_addition(rng, truth, t)
            if not r:
                continue
            A.add(0, r, w=1 + t % 3)
            B.add(0, r, w=1 + t % 3)
            assert _pairs(A) == _pairs(B), (g, t)
            ga, gb = A.graph(0, aligned=True), B.graph(0, aligned=True)
            assert ga[0] == gb[0] and ga[5] == gb[5] and all(np.array_equal(x, y) for x, y in zip(ga[1:5], gb[1:5])), (g, t)
            assert A.consensus(0) == B.consensus(0)
        if g == 0:
            cons = A.consensus(0)
            A.purge(0, cons, w=3)
            B.purge(0, cons, w=3)
            A.add(0, b"GGGGGGGG")
            B.add(0, b"GGGGGGGG")
            assert _pairs(A) == _pairs(B) and _edges(A) == _edges(B)
        A.close()
        B.close()


def test_unknown_type_is_refused():
    L = po.lib()
    for t in (-1, 3, 7):
        assert not L.orp_create_mode(t, 4, -8, -8, -4, -20, -1)
