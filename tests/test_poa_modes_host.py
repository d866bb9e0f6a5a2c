"""CPU checks of the plain-Python statement of the POA engine's three alignment types (tests/poa_modes_common.py), which the
GPU tests hold the kernels to: local mode is poa_common's recurrence, global and semi-global are the best over every
source-to-sink path of a plain sequence-to-sequence DP with the type's boundaries."""
import random

import numpy as np
import pytest

from tests.poa_common import _ref_score
from tests.poa_modes_common import (GLOBAL, LOCAL, SEMI_GLOBAL, boundary_violations, brute_force, gap, mode_path_score,
                                    mode_score, seq_score)


def _random_dag(rng, n, p_edge):
    """n nodes with shuffled ids, edges only forward in a hidden order; returns bases, a topological order, edges"""
    ids = list(range(n))
    rng.shuffle(ids)                      # ids[k]: the node at hidden position k
    ef, et = [], []
    for a in range(n):
        for b in range(a + 1, n):
            if b == a + 1 and rng.random() < 0.6 or rng.random() < p_edge:
                ef.append(ids[a])
                et.append(ids[b])
    bases = bytes(rng.choice(b"ACGT") for _ in range(n))
    return bases, np.array(ids, np.int32), np.array(ef, np.int32), np.array(et, np.int32)


def test_gap_is_the_better_affine_piece():
    assert [gap(k) for k in range(6)] == [0, -8, -12, -16, -20, -24]
    assert gap(6) == -25 and gap(13) == -32 and gap(30) == -49           # (the second piece from 6 bases on)


def test_local_mode_is_the_local_recurrence():
    rng = random.Random(5)
    for _ in range(60):
        bases, rank, ef, et = _random_dag(rng, rng.randint(1, 25), 0.15)
        seq = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 30)))
        assert mode_score(bases, rank, ef, et, seq, LOCAL) == _ref_score(bases, rank, ef, et, seq)


@pytest.mark.parametrize("mode", [GLOBAL, SEMI_GLOBAL])
def test_global_and_semi_global_equal_the_brute_force(mode):
    rng = random.Random(11 + mode)
    for case in range(250):
        bases, rank, ef, et = _random_dag(rng, rng.randint(1, 7), 0.3)
        seq = bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 6)))
        if case % 3 == 0:                 # (reads that match part of the graph)
            seq = bases[:rng.randint(1, 6)]
        assert mode_score(bases, rank, ef, et, seq, mode) == brute_force(bases, ef, et, seq, mode), (case, bases, ef, et, seq)


def test_seq_score_by_hand():
    assert seq_score(b"ACGT", b"ACGT", GLOBAL) == 16
    assert seq_score(b"ACGT", b"TTACGT", GLOBAL) == 16 + gap(2)          # the read's head costs
    assert seq_score(b"TTACGT", b"ACGT", GLOBAL) == 16 + gap(2)          # so does the path's
    assert seq_score(b"TTACGT", b"ACGT", SEMI_GLOBAL) == 16              # ... but not in semi-global alignment
    assert seq_score(b"ACGT", b"TTACGT", SEMI_GLOBAL) == 16 + gap(2)
    assert seq_score(b"ACGT", b"ACGTTT", SEMI_GLOBAL) == 16              # the read's tail is free at the last node
    assert seq_score(b"ACGTTT", b"ACGT", SEMI_GLOBAL) == 16              # the path's tail in column L


def test_path_scorer_and_boundaries_by_hand():
    # graph: chain A-C-G-T (ids 0..3); read TTACGT
    bases, ef, et = b"ACGT", np.array([0, 1, 2]), np.array([1, 2, 3])
    seq = b"TTACGT"
    glob_nodes, glob_pos = np.array([-1, -1, 0, 1, 2, 3]), np.array([0, 1, 2, 3, 4, 5])
    assert mode_path_score(bases, ef, et, seq, glob_nodes, glob_pos, GLOBAL) == 16 + gap(2)
    assert boundary_violations(ef, et, 4, 6, glob_nodes, glob_pos, GLOBAL) == []
    # semi-global: the read's head left on row 0 (not in the path) costs gap(2)
    semi_nodes, semi_pos = np.array([0, 1, 2, 3]), np.array([2, 3, 4, 5])
    assert mode_path_score(bases, ef, et, seq, semi_nodes, semi_pos, SEMI_GLOBAL) == 16 + gap(2)
    assert boundary_violations(ef, et, 4, 6, semi_nodes, semi_pos, SEMI_GLOBAL) == []
    assert boundary_violations(ef, et, 4, 6, semi_nodes, semi_pos, GLOBAL) != []
    # a semi-global path that starts inside the graph must start in column 0
    assert boundary_violations(ef, et, 4, 6, np.array([1, 2]), np.array([3, 4]), SEMI_GLOBAL) != []
    assert boundary_violations(ef, et, 4, 2, np.array([1, 2]), np.array([0, 1]), SEMI_GLOBAL) == []
