"""Global and semi-global alignment in the POA engine (ioc_poa_create_mode, `cluster -A 1|2`).  As for local alignment
(test_gpu_poa.py) there is no spoa to pin them to: the GPU's score is held to the plain-Python recurrence of
tests/poa_modes_common.py, its path to a walk through the graph that rescores to it and keeps the type's boundaries."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests.poa_common import mutate, random_addition
from tests.poa_modes_common import GLOBAL, LOCAL, SEMI_GLOBAL, boundary_violations, mode_path_score, mode_score
from tests.test_gpu_poa import SC, Poa

pytestmark = pytest.mark.gpu


class ModePoa(Poa):
    """the engine of test_gpu_poa.Poa, created through ioc_poa_create_mode"""

    def __init__(self, ctx, mode, **sc):
        sc = dict(SC, **sc)
        self.L = _lib.load()
        self.h = C.c_void_p()
        rc = self.L.ioc_poa_create_mode(ctx.h, mode, sc["m"], sc["n"], sc["g"], sc["e"], sc["q"], sc["c"], C.byref(self.h))
        assert rc == 0, rc
        self.ops = _lib.ConsensusOps()
        self.L.ioc_poa_bind(self.h, C.byref(self.ops))


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _check_adds(poa, idx, reads, mode):
    for t, read in enumerate(reads):
        bases, rank, ef, et, ew = poa.graph(idx)
        want = mode_score(bases, rank, ef, et, read, mode)
        poa.add(idx, read)
        nodes, pos, score = poa.last_alignment()
        assert score == want, (mode, t, score, want)
        assert mode_path_score(bases, ef, et, read, nodes, pos, mode) == score, (mode, t)
        assert boundary_violations(ef, et, len(bases), len(read), nodes, pos, mode) == [], (mode, t)


@pytest.mark.parametrize("mode", [GLOBAL, SEMI_GLOBAL])
def test_score_and_path_on_noisy_copies(ctx, mode):
    """short graphs (one tile), the read shapes of tools/fuzz_poa.py: noisy copies, fragments, long deletions and
    insertions, unrelated heads and tails"""
    rng = random.Random(40 + mode)
    poa = ModePoa(ctx, mode)
    for g in range(3):
        truth = bytes(rng.choice(b"ACGT") for _ in range(rng.choice([60, 150, 220])))
        poa.create(g, mutate(rng, truth, 0.08))
        _check_adds(poa, g, [random_addition(rng, truth, t) for t in range(6)], mode)
    poa.close()


@pytest.mark.parametrize("mode", [GLOBAL, SEMI_GLOBAL])
def test_score_and_path_across_tiles(ctx, mode):
    """reads of 300-700 bases (more than one 256-column tile) against graphs of several hundred nodes (more than one 64-row
    tile), with deletions of 20-45 bases (predecessors out of the LDS ring or in the tile above)"""
    rng = random.Random(50 + mode)
    poa = ModePoa(ctx, mode)
    truth = bytes(rng.choice(b"ACGT") for _ in range(520))
    poa.create(0, mutate(rng, truth, 0.06))
    cut = lambda s, a, n: s[:a] + s[a + n:]
    reads = [mutate(rng, truth, 0.1), mutate(rng, cut(truth, 250, 30), 0.05), truth[:310],
             bytes(rng.choice(b"ACGT") for _ in range(40)) + mutate(rng, cut(truth, 100, 45), 0.05) + truth[:140],
             mutate(rng, truth[60:], 0.12)]
    _check_adds(poa, 0, reads, mode)
    bases, rank, ef, et, ew = poa.graph(0)
    assert len(bases) > 128 and max(len(r) for r in reads) > 600
    poa.close()


@pytest.mark.parametrize("mode", [GLOBAL, SEMI_GLOBAL])
def test_score_and_path_low_complexity_and_many_predecessors(ctx, mode):
    """homopolymers and dinucleotide repeats (many equal-score paths: the tie rules decide), and a node reached from many
    predecessors (deletions of different lengths that end in front of the same node)"""
    rng = random.Random(60 + mode)
    poa = ModePoa(ctx, mode)
    rep = b"AC" * 60 + b"GGGGGGGGGGGG" + b"TTA" * 30
    poa.create(0, rep)
    _check_adds(poa, 0, [mutate(rng, rep, 0.1) for _ in range(4)] + [rep[20:200], b"A" * 90 + rep[:100]], mode)
    head, tail = bytes(rng.choice(b"ACGT") for _ in range(80)), bytes(rng.choice(b"ACGT") for _ in range(80))
    poa.create(1, head + tail)
    # deletions of different lengths in front of tail[0]: most reads add an in-edge to that node (the others place their
    # deletion elsewhere at the same score, through an earlier read's edge)
    ks = [k for k in range(76, 8, -4) if head[k - 1] != head[79]][:14]
    _check_adds(poa, 1, [head[:k] + tail for k in ks], mode)
    bases, rank, ef, et, ew = poa.graph(1)
    assert np.bincount(et).max() >= 6
    poa.close()


def test_mode_0_is_ioc_poa_create(ctx):
    """ioc_poa_create_mode(..., 0, ...) and ioc_poa_create: the same alignments, graphs and consensus"""
    rng = random.Random(70)
    a, b = Poa(ctx), ModePoa(ctx, LOCAL)
    truth = bytes(rng.choice(b"ACGT") for _ in range(400))
    first = mutate(rng, truth, 0.08)
    for p in (a, b):
        p.create(3, first)
    for t in range(6):
        read = random_addition(rng, truth, t)
        results = []
        for p in (a, b):
            p.add(3, read, w=1 + t % 2)
            results.append(p.last_alignment())
        assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1]), t
        assert results[0][2] == results[1][2], t
    ga, gb = a.graph(3), b.graph(3)
    assert ga[0] == gb[0] and all(np.array_equal(x, y) for x, y in zip(ga[1:], gb[1:]))
    assert a.consensus(3) == b.consensus(3)
    a.close()
    b.close()


def test_the_types_align_the_ends_differently(ctx):
    """a read whose three first and three last bases mismatch the graph: local alignment leaves them unaligned, global
    alignment aligns every base, semi-global alignment pays for the read's head (a free start in the graph) and aligns it"""
    rng = random.Random(80)
    truth = bytes(rng.choice(b"ACGT") for _ in range(120))
    flip = {ord("A"): b"C", ord("C"): b"G", ord("G"): b"T", ord("T"): b"A"}
    read = b"".join(flip[x] for x in truth[:3]) + truth[3:-3] + b"".join(flip[x] for x in truth[-3:])
    aln = {}
    for mode in (LOCAL, GLOBAL, SEMI_GLOBAL):
        poa = ModePoa(ctx, mode)
        poa.create(0, truth)
        bases, rank, ef, et, ew = poa.graph(0)
        poa.add(0, read)
        aln[mode] = poa.last_alignment()
        assert aln[mode][2] == mode_score(bases, rank, ef, et, read, mode), mode
        poa.close()
    pos = {m: [int(p) for p in aln[m][1] if p >= 0] for m in aln}
    assert pos[LOCAL][0] == 3 and pos[LOCAL][-1] == len(read) - 4          # the mismatched ends stay out
    assert pos[GLOBAL] == list(range(len(read)))                           # every base aligned
    assert pos[SEMI_GLOBAL][0] < 3                                          # the read's head costs, so it is aligned too
    assert aln[LOCAL][2] > aln[SEMI_GLOBAL][2] >= aln[GLOBAL][2]            # (a global alignment is a semi-global one)


def test_unknown_mode_is_refused(ctx):
    L = _lib.load()
    h = C.c_void_p()
    for mode in (-1, 3, 9):
        assert L.ioc_poa_create_mode(ctx.h, mode, 4, -8, -8, -4, -20, -1, C.byref(h)) == -1      # IOC_ERR_ARG
    assert b"alignment type" in L.ioc_last_error(ctx.h)
    assert L.ioc_poa_create_mode(ctx.h, GLOBAL, 4, -8, -4, -8, -20, -1, C.byref(h)) == -1       # (the scores' own check)


def _run_consensus(ctx, rs, mode, poa_type, cons, window, speculate, monkeypatch):
    """test_gpu_poa._run_consensus with an engine of the given alignment type"""
    from isonclust2_amd import pipeline
    sb, _ = pipeline.sort_stage(ctx, rs, 11, 15)
    events = []

    def rep_changed(user, cls, rec):
        r = rec.contents
        events.append((int(cls), int(r.entry), C.string_at(r.raw_seq, r.raw_len), int(r.hpc_len), int(r.n_fwd), int(r.n_rev)))

    monkeypatch.setenv("IOC_CONS_SPECULATE", "1" if speculate else "0")
    monkeypatch.setenv("IOC_CONS_VIEW_CHECK", "1")
    if window:
        monkeypatch.setenv("IOC_CONS_WINDOW", str(window))
    else:
        monkeypatch.delenv("IOC_CONS_WINDOW", raising=False)
    poa = ModePoa(ctx, poa_type)
    cb = _lib.CONS_REP_CHANGED(rep_changed)
    poa.ops.rep_changed = cb
    cargs = _lib.ConsensusArgs(cons_min_size=cons[0], cons_max_size=cons[1], cons_period=cons[2], left_depth=-1, left_sizes=None)
    cls, strand, st = ctx.cluster_consensus(api.default_params(11, 15, mode), None, sb.view, cargs, poa.ops)
    db = ctx.index_export()
    graphs = {}
    for c in range(int(st["n_clusters"])):
        if poa.size(c) >= 0:
            g = poa.graph(c)
            graphs[c] = (g[0], tuple(g[1].tolist()), tuple(g[2].tolist()), tuple(g[3].tolist()), tuple(g[4].tolist()), poa.size(c))
    poa.close()
    return cls, strand, st, events, db, graphs


@pytest.mark.parametrize("poa_type", [GLOBAL, SEMI_GLOBAL])
@pytest.mark.parametrize("shape,mode,cons,window", [((300, 6, 600), "fast", (3, 12, 500), 7), ((260, 10, 500), "sahlin", (2, 8, 40), None)])
def test_deferred_consensus_equals_immediate(ctx, monkeypatch, poa_type, shape, mode, cons, window):
    """test_gpu_poa.test_deferred_consensus_equals_immediate under global and semi-global alignment: the batched, verified
    and rolled-back consensus requests give what taking every consensus at once gives, and the type matters (the graphs are
    not the local ones)"""
    from isonclust2_amd import synth
    rs = synth.generate(shape[0], shape[1], shape[2], 11, 21, seed=sum(shape) + len(mode), dup_every=2 if shape[1] > 8 else 0)
    a = _run_consensus(ctx, rs, mode, poa_type, cons, window, False, monkeypatch)
    b = _run_consensus(ctx, rs, mode, poa_type, cons, window, True, monkeypatch)
    assert a[2]["n_cons_invoked"] > 5
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[2]["n_cons_invoked"] == b[2]["n_cons_invoked"] and a[2]["n_clusters"] == b[2]["n_clusters"]
    assert a[3] == b[3]
    for x, y in zip(a[4], b[4]):
        assert np.array_equal(x, y)
    assert a[5] == b[5]
    monkeypatch.setenv("IOC_CONS_FORCE_ROLLBACK", "2")
    c = _run_consensus(ctx, rs, mode, poa_type, cons, window, True, monkeypatch)
    monkeypatch.delenv("IOC_CONS_FORCE_ROLLBACK")
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and a[3] == c[3]
    for x, y in zip(a[4], c[4]):
        assert np.array_equal(x, y)
    assert a[5] == c[5]
    loc = _run_consensus(ctx, rs, mode, LOCAL, cons, window, True, monkeypatch)
    assert loc[5] != a[5]
