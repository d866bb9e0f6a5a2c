"""The oracle's scalar POA (oracle/poa_oracle.cpp) at scores other than the reference's 4 / -8 / -8 / -4 / -20 / -1
(tests/poa_params_common.py has the sets and why each is there), under all three alignment types, on the CPU: the checks of
tests/test_oracle_poa_modes.py with the scores passed through — score = the plain recurrence, the path a walk that rescores to
it and keeps the type's boundaries, graph invariants, the brute force over the paths of small graphs.  Only then is the oracle
what the engine is compared with at these scores (tests/test_gpu_poa_params.py).  And the workload that comparison runs must
hold what it was chosen for: gap runs of both kinds under every set and type (or, without a match reward, no alignment at all).
The by-hand cases at the end state the tie rules of DESIGN.md 5.7 where these scores make them bite."""
import random

import pytest

from oracle import pyoracle as po
from tests.poa_common import _ref_score, mutate, random_addition
from tests.poa_modes_common import GLOBAL, LOCAL, SEMI_GLOBAL, boundary_violations, brute_force, gap, mode_path_score, mode_score
from tests.poa_params_common import (MIN_GAP_RUNS, PIECE_RULE_CASES, SCORE_NAMES, TYPE_IDS, TYPES, all_empty, gap_runs,
                                     piece_predecessor_ties, random_addition_graphs, scores)
from tests.test_oracle_poa_modes import _check_graph_invariants, _edges, _pairs

_type_ids = lambda t: TYPE_IDS[t]


@pytest.mark.parametrize("mode", TYPES, ids=_type_ids)
@pytest.mark.parametrize("name", SCORE_NAMES)
def test_score_and_path_equal_the_plain_statement(name, mode):
    sc = scores(name)
    rng = random.Random(5 + mode)
    adds = 0
    for g in range(14):
        P = po.OraclePoa(mode=mode, **sc)
        truth = bytes(rng.choice(b"ACGT") for _ in range(rng.choice([40, 90, 200])))
        first = mutate(rng, truth, 0.05)
        P.create(0, first)
        total, n_seq = 2 * (len(first) - 1), 1
        for t in range(rng.randint(4, 8)):
            r = random_addition(rng, truth, t)
            if not r:
                continue
            bases, rank, ef, et, ew = P.graph(0)
            want = mode_score(bases, rank, ef, et, r, mode, sc)
            if mode == LOCAL and len(bases) * len(r) <= 20000:          # (the cell-by-cell loops, where they are quick)
                assert _ref_score(bases, rank, ef, et, r, sc) == want, (g, t)
            w = 1 + t % 3
            P.add(0, r, w=w)
            nodes, pos, score = P.last_alignment()
            adds += 1
            assert score == want, (g, t, score, want)
            assert mode_path_score(bases, ef, et, r, nodes, pos, mode, sc) == score, (g, t)
            assert boundary_violations(ef, et, len(bases), len(r), nodes, pos, mode) == [], (g, t)
            total += 2 * w * (len(r) - 1)
            _check_graph_invariants(P, 0, total)
            n_seq += 1
            assert P.size(0) == n_seq
        P.close()
    assert adds > 50


@pytest.mark.parametrize("mode", [GLOBAL, SEMI_GLOBAL], ids=_type_ids)
@pytest.mark.parametrize("name", SCORE_NAMES)
def test_small_graphs_equal_the_brute_force(name, mode):
    """graphs of 2 - 4 reads of at most 6 bases built under the type and the scores, then one more read: the score is the best
    over every source-to-sink path of the plain sequence-to-sequence DP, which charges gap(k) per run and knows no pieces"""
    sc = scores(name)
    rng = random.Random(17 + mode)
    for case in range(100):
        P = po.OraclePoa(mode=mode, **sc)
        alphabet = b"ACGT" if case % 2 else b"AC"
        reads = [bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 6))) for _ in range(rng.randint(2, 4))]
        P.create(0, reads[0])
        for r in reads[1:]:
            bases, rank, ef, et, ew = P.graph(0)
            P.add(0, r)
            nodes, pos, score = P.last_alignment()
            assert score == brute_force(bases, ef, et, r, mode, sc), (case, reads, r)
            assert mode_path_score(bases, ef, et, r, nodes, pos, mode, sc) == score, (case, reads, r)
            assert boundary_violations(ef, et, len(bases), len(r), nodes, pos, mode) == [], (case, reads, r)
        P.close()


@pytest.mark.parametrize("mode", TYPES, ids=_type_ids)
@pytest.mark.parametrize("name", SCORE_NAMES)
def test_the_random_additions_hold_what_they_were_planted_for(name, mode):
    """The workload tests/test_gpu_poa_params.py compares engine and oracle on, on the oracle alone: 71 additions whose
    alignments show at least 30 vertical and 30 horizontal gap runs of two or more — the tie between extending and opening
    is met only inside such a run —, or are all empty where the scores allow no alignment (each read a chain of its own)."""
    vert = horz = adds = 0
    for first, reads in random_addition_graphs():
        P = po.OraclePoa(mode=mode, **scores(name))
        P.create(0, first)
        for r, w in reads:
            n_nodes, n_edges = len(P.graph(0)[0]), len(P.graph(0)[2])
            P.add(0, r, w=w)
            nodes, pos, score = P.last_alignment()
            adds += 1
            v, h = gap_runs(nodes, pos)
            vert, horz = vert + v, horz + h
            if all_empty(name, mode):
                assert len(nodes) == 0 and score == 0
                assert (len(P.graph(0)[0]), len(P.graph(0)[2])) == (n_nodes + len(r), n_edges + len(r) - 1)
        P.close()
    print(name, TYPE_IDS[mode], "additions", adds, "vertical runs", vert, "horizontal runs", horz)
    assert adds == 71
    if not all_empty(name, mode):
        assert vert >= MIN_GAP_RUNS and horz >= MIN_GAP_RUNS, (vert, horz)


def test_by_hand_the_second_piece_through_the_earlier_predecessor():
    """m 1, n -1, first piece -1 a base, second piece -2 flat: gap(1) = -1, gap(2) = -2 by either piece, gap(k > 2) = -2 by the
    second.  Global.  ACC, then CGACGC: CG on row 0, A C matched, G inserted, C matched — nodes 3 4 (C G) in front of 0 1 (A C),
    node 5 (G) between 1 and 2; the order is 3 4 0 1 5 2 and node 2's in-edges are (1, 2) from the first read, then (5, 2).
    Now AG.  The end cell is (node 2, column 2), H = -2, and no diagonal gives it (H of nodes 1 and 5 in column 1 is -2 and -3,
    the mismatch would need -1).  Vertically, through node 1: H = -2 there (A on node 3's C -1, G on node 4 +1, nodes 0 1
    skipped -2), so opening costs -3 and extending the first piece -3 (F1 = -2), but the second piece, opened under node 4
    where H = 0, is -2 flat: it gives H.  Through node 5: H = -1 there (nodes 3 4 skipped -2, A +1, node 1 skipped -1, G on
    node 5 +1) and opening the first piece gives -2: H as well.  The first piece through the later predecessor, the second
    piece through the earlier one: the earlier predecessor wins, the walk goes up the second piece to node
    4 and takes two diagonals.  (Preferring the first piece would give 3 4 skipped, A on 0, 1 skipped, G on 5, 2 skipped.)"""
    P = po.OraclePoa(mode=GLOBAL, m=1, n=-1, g=-1, e=-1, q=-2, c=0)
    P.create(0, b"ACC")
    P.add(0, b"CGACGC")
    assert _pairs(P) == ([(-1, 0), (-1, 1), (0, 2), (1, 3), (-1, 4), (2, 5)], 0)
    bases, rank, ef, et, ew = P.graph(0)
    assert bases == b"ACCCGG" and rank.tolist() == [3, 4, 0, 1, 5, 2]
    assert [(a, b) for a, b in zip(ef.tolist(), et.tolist()) if b == 2] == [(1, 2), (5, 2)]
    P.add(0, b"AG")
    assert _pairs(P) == ([(3, 0), (4, 1), (0, -1), (1, -1), (2, -1)], -2)
    P.close()


@pytest.mark.parametrize("case", range(len(PIECE_RULE_CASES)))
def test_the_piece_rule_cases_hold_what_they_were_planted_for(case):
    """each of the inputs the engine is compared on for the rule between the pieces has, in the oracle's alignment of its
    last read, a vertical gap entered where the first piece's best predecessor and the second piece's differ at equal score
    (read off the plain recurrence's rows) — and the alignment rescores to the plain recurrence's score"""
    s, mode, reads = PIECE_RULE_CASES[case]
    sc = dict(zip("mngeqc", s))
    P = po.OraclePoa(mode=mode, **sc)
    P.create(0, reads[0])
    for r in reads[1:-1]:
        P.add(0, r)
    bases, rank, ef, et, ew = P.graph(0)
    P.add(0, reads[-1])
    nodes, pos, score = P.last_alignment()
    assert score == mode_score(bases, rank, ef, et, reads[-1], mode, sc)
    assert mode_path_score(bases, ef, et, reads[-1], nodes, pos, mode, sc) == score
    assert piece_predecessor_ties(bases, rank, ef, et, reads[-1], mode, sc, nodes, pos) >= 1
    P.close()
