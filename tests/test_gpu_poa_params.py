"""The POA engine (ioc_poa.hip) at scores other than the reference's 4 / -8 / -8 / -4 / -20 / -1, under all three alignment
types.  tests/poa_params_common.py has the score sets and what each reaches in k_poa_tile / k_poa_trace: open / extend ties
on every continued gap (`linear`), the two pieces tying in every cell (`equal_pieces`), flat prefix maxima (`free_ext`),
nothing but empty alignments (`m0`), the ends of the accepted range (`int8`).  Two references, both pinned on the CPU at
these sets by tests/test_oracle_poa_params.py: the plain recurrence of tests/poa_modes_common.py (scores, rescored paths,
boundaries — it knows no tie rules) and the oracle's scalar POA (every pair of every alignment, every graph: DESIGN.md 5.7's
tie rules).  Everything is integer and compared exactly."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests.poa_common import mutate, random_addition
from tests.poa_modes_common import GLOBAL, LOCAL, SEMI_GLOBAL, boundary_violations, gap, mode_path_score, mode_score
from tests.poa_params_common import (MIN_GAP_RUNS, PIECE_RULE_CASES, SCORE_NAMES, SCORE_TABLE, TYPE_IDS, TYPES, all_empty,
                                     gap_runs, random_addition_graphs, scores)
from tests.test_gpu_poa import Poa
from tests.test_gpu_poa_modes import ModePoa
from tests.test_gpu_poa_oracle import _add_both, _longest_run, _low_complexity, _rand, _same_alignment, _same_graph, _stores

pytestmark = pytest.mark.gpu

_type_ids = lambda t: TYPE_IDS[t]
IOC_ERR_ARG, IOC_ERR_CAPACITY = -1, -4


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def addition_graphs():
    return random_addition_graphs()


# ---- a. against the plain recurrence, independent of the oracle -------------------------------------------------------------
def _check_adds(poa, idx, reads, mode, sc):
    """test_gpu_poa_modes._check_adds with the scores passed through"""
    for t, read in enumerate(reads):
        bases, rank, ef, et, ew = poa.graph(idx)
        want = mode_score(bases, rank, ef, et, read, mode, sc)
        poa.add(idx, read)
        nodes, pos, score = poa.last_alignment()
        assert score == want, (mode, t, score, want)
        assert mode_path_score(bases, ef, et, read, nodes, pos, mode, sc) == score, (mode, t)
        assert boundary_violations(ef, et, len(bases), len(read), nodes, pos, mode) == [], (mode, t)


@pytest.mark.parametrize("mode", TYPES, ids=_type_ids)
@pytest.mark.parametrize("name", SCORE_NAMES)
def test_score_and_path_equal_the_plain_recurrence(ctx, name, mode):
    """a graph inside one tile with the read shapes of tools/fuzz_poa.py, and a graph of six tile rows with reads of two
    column tiles: a 30-base deletion, a fragment, an unrelated head in front of a 45-base deletion"""
    sc = scores(name)
    rng = random.Random(140 + mode)
    poa = Poa(ctx, **sc) if mode == LOCAL else ModePoa(ctx, mode, **sc)
    truth = _rand(rng, 150)
    poa.create(0, mutate(rng, truth, 0.08))
    _check_adds(poa, 0, [random_addition(rng, truth, t) for t in range(6)], mode, sc)
    truth = _rand(rng, 330)
    poa.create(1, mutate(rng, truth, 0.06))
    cut = lambda s, a, n: s[:a] + s[a + n:]
    reads = [mutate(rng, truth, 0.1), mutate(rng, cut(truth, 150, 30), 0.05), truth[:270],
             _rand(rng, 40) + mutate(rng, cut(truth, 100, 45), 0.05), mutate(rng, truth[60:], 0.12)]
    _check_adds(poa, 1, reads, mode, sc)
    assert len(poa.graph(1)[0]) > 320 and max(len(r) for r in reads) > 256
    poa.close()


# ---- b, c. against the oracle, rule for rule; and the workload holds what it was planted for -----------------------------------
@pytest.mark.parametrize("mode", TYPES, ids=_type_ids)
@pytest.mark.parametrize("name", SCORE_NAMES)
def test_random_additions_give_the_oracles_graphs(ctx, addition_graphs, name, mode):
    """The first 10 graphs of test_gpu_poa_oracle._random_additions, 71 additions: after each the engine's alignment (score,
    every pair) and graph (letters, weighted edges, topological order, size, consensus) are the oracle's.  The oracle's
    alignments must show what the set is here for: 30 runs of two or more of either kind of gap — or, without a match reward
    under local and semi-global alignment, no alignment at all, every read a chain of its own in both stores."""
    sc = scores(name)
    vert = horz = adds = 0
    for g, (first, reads) in enumerate(addition_graphs):
        dev, orc = _stores(ctx, mode, **sc)
        dev.create(0, first)
        orc.create(0, first)
        _same_graph(dev, orc, 0, (g, "seed"))
        for t, (r, w) in enumerate(reads):
            before = [(len(s.graph(0)[0]), len(s.graph(0)[2])) for s in (dev, orc)]
            dev.add(0, r, w=w)
            orc.add(0, r, w=w)
            adds += 1
            _same_alignment(dev, orc, (g, t))
            _same_graph(dev, orc, 0, (g, t))
            nodes, pos, score = orc.last_alignment()
            v, h = gap_runs(nodes, pos)
            vert, horz = vert + v, horz + h
            if all_empty(name, mode):
                assert len(nodes) == 0 and score == 0 and len(dev.last_alignment()[0]) == 0, (g, t)
                for s, (n_nodes, n_edges) in zip((dev, orc), before):
                    assert (len(s.graph(0)[0]), len(s.graph(0)[2])) == (n_nodes + len(r), n_edges + len(r) - 1), (g, t)
        dev.close()
        orc.close()
    print(name, TYPE_IDS[mode], "additions", adds, "vertical runs", vert, "horizontal runs", horz)
    assert adds == 71
    if not all_empty(name, mode):
        assert vert >= MIN_GAP_RUNS and horz >= MIN_GAP_RUNS, (vert, horz)


# ---- d. long gaps ---------------------------------------------------------------------------------------------------------------
def _counts(nodes, pos):
    return dict(vert=int(np.sum(pos < 0)), horz=int(np.sum(nodes < 0)), diag=int(np.sum((nodes >= 0) & (pos >= 0))),
                vrun=_longest_run(pos, -1), hrun=_longest_run(nodes, -1))


@pytest.mark.parametrize("mode", [GLOBAL, SEMI_GLOBAL], ids=_type_ids)
@pytest.mark.parametrize("name", ["linear", "free_ext"])
def test_long_gaps(ctx, name, mode):
    """A 300-base insertion and a 300-base deletion, alone and together in a 700-base read, a 300-base head on row 0 and 300
    nodes on column 0: gaps longer than a tile's 64 rows / 256 columns that nothing cuts — under `linear` every cell of such
    a run ties between extending and opening, under `free_ext` the run's cells all score the same.  The graph is a chain
    over A, C, G and the inserted bases are T, so what the oracle's alignment must contain follows from the scores alone
    (besides being the engine's pair for pair):
      * every base of the read that is no T matches its own node in the one best alignment; a T against a node costs a
        mismatch AND that node's match, so the T's are one horizontal run between two matched nodes (or on row 0);
      * a read shorter than the chain by 300 leaves 300 nodes in vertical gaps under global alignment; with `free_ext` a
        second run would cost another -3, so they are one run; with `linear` the run may split at equal score (a base of
        the read may match an equal letter inside the deleted stretch), so only their number is fixed;
      * `both` under `linear`: 300 mismatches (-2400) beat two gaps of 300 (-3600), nothing to assert but the oracle's pairs;
      * semi-global alignment under `linear`: a gap of 300 costs more than the read can win back, so the alignments are
        short or empty (asserted: what the oracle gives); under `free_ext` a gap costs 3 and the alignments are the global
        ones, but for a head on row 0, which stays unaligned, and the chain's head on column 0, which is free."""
    sc = scores(name)
    rng = random.Random(97)
    t = _rand(rng, 700, b"ACG")
    ins = b"T" * 300
    cases = {"insertion": (t[:400], t[:200] + ins + t[200:400]), "deletion": (t, t[:200] + t[500:]),
             "both": (t, t[:150] + ins + t[150:300] + t[600:]), "row0": (t[:400], ins + t[:400]), "col0": (t, t[300:])}
    follow = {k: mutate(rng, r, 0.05) for k, (_, r) in cases.items()}
    assert len(cases["both"][1]) == 700
    full = mode == GLOBAL or name == "free_ext"          # (the whole read is aligned, gaps and all)
    for k, (graph, read) in cases.items():
        dev, orc = _stores(ctx, mode, **sc)
        dev.create(0, graph)
        orc.create(0, graph)
        _add_both(dev, orc, 0, read, (k, "read"))
        nodes, pos, score = orc.last_alignment()
        c = _counts(nodes, pos)
        if k == "insertion" and full:
            assert (c["hrun"], c["horz"], c["vert"], c["diag"]) == (300, 300, 0, 400), (k, c)
            assert score == 400 * sc["m"] + gap(300, sc)
        if k == "deletion" and full:
            assert (c["vert"], c["horz"], c["diag"]) == (300, 0, 400) and (name == "linear" or c["vrun"] == 300), (k, c)
            assert score == 400 * sc["m"] + gap(300, sc)
        if k == "both" and name == "free_ext":
            assert (c["hrun"], c["horz"], c["vrun"], c["vert"], c["diag"]) == (300, 300, 300, 300, 400), (k, c)
        if k == "row0" and mode == GLOBAL:
            assert nodes[:300].tolist() == [-1] * 300 and pos[:300].tolist() == list(range(300)) and c["horz"] == 300, (k, c)
        if k == "row0" and mode == SEMI_GLOBAL and name == "free_ext":
            assert (c["diag"], c["horz"], c["vert"]) == (400, 0, 0) and int(pos[0]) == 300 and score == 800 + gap(300, sc), (k, c)
        if k == "col0" and mode == GLOBAL:             # (diagonal before vertical: the walk reaches column 0 in row 300)
            assert pos[:300].tolist() == [-1] * 300 and nodes[:300].tolist() == list(range(300)) and c["vert"] == 300, (k, c)
        if k == "col0" and mode == SEMI_GLOBAL:
            assert (c["diag"], c["horz"], c["vert"]) == (400, 0, 0) and int(nodes[0]) == 300 and score == 400 * sc["m"], (k, c)
        _add_both(dev, orc, 0, follow[k], (k, "noisy copy"), w=2)
        dev.close()
        orc.close()


# ---- e. tie-heavy input ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", TYPES, ids=_type_ids)
@pytest.mark.parametrize("name", ["linear", "equal_pieces"])
def test_low_complexity_and_tie_heavy_reads(ctx, name, mode):
    """repeats over two letters (test_gpu_poa_oracle._low_complexity): many alignments of equal score, and with these scores
    every continued gap and every branch node is a tie on top"""
    _low_complexity(ctx, mode, **scores(name))


# ---- f. predecessors from memory ------------------------------------------------------------------------------------------------
def test_equal_pieces_with_a_tiny_predecessor_staging_area(ctx, monkeypatch):
    """IOC_POA_PRED_LDS = 5: all but the first five predecessor entries of a tile are read from memory.  Deletions of
    different lengths in front of the same node give it many predecessors; with the two pieces equal, F1 and F2 tie in
    every cell below them, through the same predecessor each time, and the first piece has to stand at every one (the
    other half of that rule, the second piece through an EARLIER predecessor, is the next test's)."""
    monkeypatch.setenv("IOC_POA_PRED_LDS", "5")
    sc = scores("equal_pieces")
    rng = random.Random(160)
    dev, orc = _stores(ctx, GLOBAL, **sc)
    head, tail = _rand(rng, 80), _rand(rng, 80)
    dev.create(0, head + tail)
    orc.create(0, head + tail)
    ks = [k for k in range(76, 8, -4) if head[k - 1] != head[79]][:14]
    for x, k in enumerate(ks):
        _add_both(dev, orc, 0, head[:k] + tail, ("deletion", k), w=1 + x % 2)
    bases, rank, ef, et, ew = orc.graph(0)
    assert np.bincount(et).max() >= 6
    for x in range(4):
        _add_both(dev, orc, 0, mutate(rng, head[:rng.randint(10, 70)] + tail, 0.08), ("noisy", x))
    bases, rank, ef, et, ew = dev.graph(0)
    read = mutate(rng, head + tail, 0.1)
    want = mode_score(bases, rank, ef, et, read, GLOBAL, sc)
    _add_both(dev, orc, 0, read, "last")
    assert dev.last_alignment()[2] == want
    dev.close()
    orc.close()


@pytest.mark.parametrize("pred_lds", [None, "1"])
def test_the_second_piece_through_an_earlier_predecessor(ctx, monkeypatch, pred_lds):
    """Where the first piece through one predecessor ties with the second piece through another, the earlier predecessor wins
    (`f2p < f1p` in k_poa_tile).  `equal_pieces` cannot reach that — both pieces come through the same predecessor — and no
    random workload of this file does; the inputs of poa_params_common.PIECE_RULE_CASES do (checked on the CPU, the first one
    by hand: tests/test_oracle_poa_params.py).  Once with the predecessor lists in LDS, once with all but a tile's first
    entry read from memory."""
    if pred_lds:
        monkeypatch.setenv("IOC_POA_PRED_LDS", pred_lds)
    for k, (s, mode, reads) in enumerate(PIECE_RULE_CASES):
        sc = dict(zip("mngeqc", s))
        dev, orc = _stores(ctx, mode, **sc)
        dev.create(0, reads[0])
        orc.create(0, reads[0])
        for x, r in enumerate(reads[1:]):
            _add_both(dev, orc, 0, r, (k, x))
        if k == 0:
            nodes, pos, score = dev.last_alignment()
            assert (nodes.tolist(), pos.tolist(), score) == ([3, 4, 0, 1, 2], [0, 1, -1, -1, -1], -2)
        dev.close()
        orc.close()


# ---- g. what create refuses, and the sizes the accepted scores are safe up to ---------------------------------------------------
def _create_rc(ctx, mode, s):
    L = _lib.load()
    h = C.c_void_p()
    rc = L.ioc_poa_create_mode(ctx.h, mode, *s, C.byref(h)) if mode is not None else L.ioc_poa_create(ctx.h, *s, C.byref(h))
    if rc == 0:
        L.ioc_poa_destroy(h)
    return rc


def test_scores_out_of_order_or_out_of_range_are_refused(ctx):
    L = _lib.load()
    out_of_order = [(-1, -8, -8, -4, -20, -1), (4, 1, -8, -4, -20, -1), (4, -8, -3, -4, -20, -1), (4, -8, -8, 1, -20, -1),
                    (4, -8, 0, 1, -20, -1), (4, -8, -8, -4, -1, -2), (4, -8, -8, -4, -20, 1), (4, -8, -8, -4, 0, 1)]
    out_of_range = [(128, -8, -8, -4, -20, -1), (4, -129, -8, -4, -20, -1), (4, -8, -129, -4, -20, -1), (4, -8, -129, -129, -20, -1),
                    (4, -8, -8, -4, -129, -1), (4, -8, -8, -4, -129, -129), (1 << 20, -8, -8, -4, -20, -1), (4, -8, -(1 << 24), -4, -20, -1)]
    for mode in (None, LOCAL, GLOBAL, SEMI_GLOBAL):
        for s in out_of_order:
            assert _create_rc(ctx, mode, s) == IOC_ERR_ARG, (mode, s)
            assert b"g <= e <= 0" in L.ioc_last_error(ctx.h)
        for s in out_of_range:
            assert _create_rc(ctx, mode, s) == IOC_ERR_ARG, (mode, s)
            assert b"-128 .. 127" in L.ioc_last_error(ctx.h)
        for name in SCORE_NAMES:                                         # every set of the table, the corners of int8 among them
            assert _create_rc(ctx, mode, SCORE_TABLE[name][0]) == 0, (mode, name)
        assert _create_rc(ctx, mode, (0, 0, 0, 0, 0, 0)) == 0 and _create_rc(ctx, mode, (127, -128, -128, 0, -128, 0)) == 0


def test_int8_scores_at_the_largest_graph(ctx):
    """The accepted scores are safe because rows and columns are bounded (the arithmetic is at ioc_poa_create_mode): a chain of
    2^21 - 1 nodes, the most the engine takes, against one base under global alignment with the int8 corner scores.  Column 0
    falls to gap(R) = -128 - 127 (R - 1), about -2.7 * 10^8 — two thirds of the way to the engine's "no value" — and the one
    base meets the last node: the diagonal comes first, then column 0 all the way up.  One node more is refused."""
    sc = scores("int8")
    R = (1 << 21) - 1
    dev = ModePoa(ctx, GLOBAL, **sc)
    dev.create(0, b"C" * R)
    dev.add(0, b"A")
    nodes, pos, score = dev.last_alignment()
    assert score == sc["n"] + gap(R - 1, sc) == -128 - 128 - 127 * (R - 2)
    assert np.array_equal(nodes, np.arange(R, dtype=np.int32))
    assert np.array_equal(pos[:-1], np.full(R - 1, -1, np.int32)) and pos[-1] == 0
    dev.close()
    dev = ModePoa(ctx, GLOBAL, **sc)
    dev.create(0, b"C" * (R + 1))
    dev.add(0, b"A")                                    # (queued: the call that needs the alignment meets the refusal)
    assert dev.L.ioc_poa_last_alignment(dev.h, 0, None, None, None) == IOC_ERR_CAPACITY
    assert b"2^21 nodes" in dev.L.ioc_last_error(ctx.h)
    dev.close()
