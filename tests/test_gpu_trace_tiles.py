"""The tiled traceback of the version-2 aligner at every shape of tile and block its walk can enter: ioc_align_pairs against the
host aligner (score and ratio equal, as tests/test_gpu_align.py::_check) and, for the same pairs, ioc_align_pairs_ops byte for byte
against ioc_host_align_ops.  The tile step recomputes 128 x 128 cells from the checkpoints of a 512 x 512 block, one lane per two
columns, the lanes one row behind each other; the walk enters a tile (a block) at any point, so a tile has 1 .. 128 rows and
columns: lanes that never switch on, tiles with fewer rows than lanes, and the full tile.  Every case is seeded and built here;
nothing is left out of the comparison.  No tolerance: integers, doubles that must be equal, bytes."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests.align_ops_checks import revcomp

pytestmark = pytest.mark.gpu

E_CLASSES = (0.005, 0.03, 0.08, 0.2)      # one error sum per gap-open class of ioc_host_gap_open: 5, 4, 3, 2
KS = (5, 11, 32)
CLIPS = (1, 2, 3, 63, 64, 65, 127, 128)   # columns (rows) left of (above) the point where the walk enters a tile and a block
_host_cache = {}


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _rand(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _subst(rng, s, rate):
    """Substitutions only: the alignment stays on its diagonal, so the shapes the walk meets are the ones asked for."""
    return bytes(rng.choice(b"ACGT") if rng.random() < rate else ch for ch in s)


def _host(q, r, rc, e):
    """(score, comparison string, operation bytes) of the host aligner for one pair; cached by what the alignment depends on."""
    L = _lib.load()
    go = L.ioc_host_gap_open(e)
    key = (q, r, bool(rc), go)
    if key not in _host_cache:
        rr = revcomp(r) if rc else r
        cap = len(q) + len(rr) + 2
        comp, sc = C.create_string_buffer(cap), C.c_int32()
        n = L.ioc_host_align(q, len(q), rr, len(rr), 2, -2, go, 1, comp, cap, C.byref(sc))
        assert n >= 0
        ops, osc = api.host_align_ops(q, rr, gap_open=go)
        assert osc == sc.value
        _host_cache[key] = (sc.value, comp.raw[:n], ops)
    return _host_cache[key]


def _check(ctx, seqs, pairs, ks=KS):
    """Plain call: score and ratio equal the host's for every k; emitting call: the same three results and the host's bytes."""
    L = _lib.load()
    ctx.align_set_pool(seqs)
    for k in ks:
        score, win, ratio = ctx.align_pairs(pairs, k)
        oscore, owin, oratio, ops = ctx.align_pairs_ops(pairs, k)
        assert np.array_equal(score, oscore) and np.array_equal(win, owin) and np.array_equal(ratio, oratio), k
        for i, (qi, ri, rc, e) in enumerate(pairs):
            tag = (i, len(seqs[qi]), len(seqs[ri]), rc, e, k)
            hs, comp, hops = _host(seqs[qi], seqs[ri], rc, e)
            assert score[i] == hs, tag
            assert ratio[i] == L.ioc_host_aln_ratio(comp, len(comp), e, len(seqs[qi]), k), tag + (int(win[i]),)
            assert ops[i] == hops, tag


# lengths of the common part: multiples of 512 / of 128 only / of 4 only / of none of them
LENGTHS = (1536, 2176, 3000, 4099, 5120, 5998, 2560, 1501)


def _clipped(rng, d, mirror, n):
    """A pair on the diagonal j = i + d (mirror: i = j + d): every tile the walk enters over its bottom edge has d columns (rows)
    left of (above) the entry point, every tile it enters over its right (bottom) edge 128 - d rows (columns); blocks alike."""
    core = _rand(rng, n)
    longer, shorter = _rand(rng, d) + core, _subst(rng, core, 0.04)
    return (longer, shorter) if mirror else (shorter, longer)   # (query, reference): mirror = the query has the prefix


def test_every_clipped_shape_in_every_gap_open_class(ctx):
    """Entry points 1, 2, 3, 63, 64, 65, 127, 128 columns and rows into a tile and a block, both orientations, with the four
    gap-open penalties and k = 5, 11, 32; some of the references reverse-complemented."""
    rng = random.Random(101)
    seqs, pairs = [], []
    for x, d in enumerate(CLIPS):
        for mirror in (False, True):
            for c, e in enumerate(E_CLASSES):
                q, r = _clipped(rng, d, mirror, LENGTHS[(x + 3 * c + int(mirror)) % len(LENGTHS)])
                rc = (x + c) % 3 == 0
                seqs += [q, revcomp(r) if rc else r]
                pairs.append((len(seqs) - 2, len(seqs) - 1, int(rc), e))
    assert len(pairs) == 2 * len(CLIPS) * len(E_CLASSES)
    _check(ctx, seqs, pairs)


def test_clipped_shapes_with_indels_and_ragged_ends(ctx):
    """The same offsets with insertions and deletions (the walk leaves the diagonal and comes back, gap steps inside clipped
    tiles) and sequences that end a few bases past / before a tile and a block edge on either side."""
    from tests.test_gpu_align import _mutate
    rng = random.Random(103)
    seqs, pairs = [], []
    for x, d in enumerate(CLIPS):
        for mirror in (False, True):
            n = (1535, 1537, 2047, 2049, 2051, 3071, 4097, 5633)[(x + int(mirror)) % 8]
            core = _rand(rng, n)
            longer, shorter = _rand(rng, d) + _mutate(rng, core, 0.06), _mutate(rng, core, 0.06)
            seqs += [longer, shorter] if mirror else [shorter, longer]
            pairs.append((len(seqs) - 2, len(seqs) - 1, 0, E_CLASSES[x % 4]))
    _check(ctx, seqs, pairs)


def test_long_gaps_across_tile_and_block_edges(ctx):
    """Insertions and deletions of 300 and 700 bases: gap runs that cross tile edges (128) and block edges (512) in both
    directions, and gaps that begin or end exactly on an edge (the flank in front of them is 512 / 1024 / 640 bases)."""
    rng = random.Random(107)
    seqs, pairs = [], []
    cases = []
    for glen in (300, 700):
        for head in (1000, 1333, 512, 1024, 640):          # bases in front of the gap; 512 / 1024 / 640: the gap ends on an edge
            cases.append((glen, head, 1400 + 97 * (head % 7)))
    for x, (glen, head, tail) in enumerate(cases):
        a, g, b = _rand(rng, head), _rand(rng, glen), _rand(rng, tail)
        whole, cut = a + g + b, _subst(rng, a, 0.03) + _subst(rng, b, 0.03)
        for deletion in (True, False):                     # the query lacks the piece / has it
            seqs += [cut, whole] if deletion else [whole, cut]
            pairs.append((len(seqs) - 2, len(seqs) - 1, 0, E_CLASSES[(x + int(deletion)) % 4]))
    # ... and the gap's far end on an edge: head + gap = 1024, 1536
    for glen, total in ((300, 1024), (700, 1536)):
        a, g, b = _rand(rng, total - glen), _rand(rng, glen), _rand(rng, 1700)
        for deletion in (True, False):
            seqs += [a + b, a + g + b] if deletion else [a + g + b, a + b]
            pairs.append((len(seqs) - 2, len(seqs) - 1, 0, 0.2))
    _check(ctx, seqs, pairs)
    # the gaps are really there: the host's strings hold the gap's columns, in a run longer than a tile is wide
    for x, (glen, _, _) in enumerate(cases):
        for y, letter in enumerate((b"D", b"I")):
            qi, ri, rc, e = pairs[2 * x + y]
            ops = _host(seqs[qi], seqs[ri], rc, e)[2]
            assert ops.count(letter) >= glen and letter * 129 in ops, (glen, letter)


@pytest.mark.parametrize("early", ["1", "0"])
@pytest.mark.parametrize("count", [60, 300])
def test_unrelated_pairs_in_the_helper_launch(ctx, monkeypatch, early, count):
    """Unrelated pairs of >= 4096 bases with the verdict threshold set, fewer and more of them than the helper launch has
    workgroups (256): sent there at once by k_fwd2_ends (early = 1, the first 256), or parked by the first launch and taken on
    in turns (early = 0, and what is beyond 256).  Exact call against the host aligner; with the threshold the scores are
    exact and every verdict is the full count's; the emitting call gives the host's bytes."""
    monkeypatch.setenv("IOC_TRACE2_EARLY", early)
    L = _lib.load()
    rng = random.Random(109)
    seqs = [_rand(rng, rng.randrange(4096, 4700)) for _ in range(30)]
    seqs += [_subst(rng, seqs[i], 0.05) for i in range(3)]
    pairs = [(i, (i + 1 + j) % 30, (i + j) % 2, 0.12) for j in range(10) for i in range(30)][:count - 6]
    pairs += [(30 + i, i, 0, 0.12) for i in range(3)] + [(i, 30 + i, 0, 0.12) for i in range(3)]   # related: decided in the first launch
    assert len(pairs) == count
    thr, k = 0.2, 11
    ctx.align_set_pool(seqs)
    ctx.align_set_verdict_threshold(0.0)
    s0, w0, r0 = ctx.align_pairs(pairs, k)
    try:
        ctx.align_set_verdict_threshold(thr)
        s1, w1, r1 = ctx.align_pairs(pairs, k)
        so, wo, ro, ops = ctx.align_pairs_ops(pairs, k)       # (always exact)
    finally:
        ctx.align_set_verdict_threshold(0.0)
    assert np.array_equal(so, s0) and np.array_equal(wo, w0) and np.array_equal(ro, r0)
    assert np.array_equal(s1, s0) and np.all(w1 <= w0)
    for i, (qi, ri, rc, e) in enumerate(pairs):
        tag = (i, len(seqs[qi]), len(seqs[ri]), rc)
        hs, comp, hops = _host(seqs[qi], seqs[ri], rc, e)
        hr = L.ioc_host_aln_ratio(comp, len(comp), e, len(seqs[qi]), k)
        assert s0[i] == hs and r0[i] == hr, tag
        assert (r1[i] >= thr) == (hr >= thr), tag
        assert ops[i] == hops, tag
    assert int(np.count_nonzero(r0 >= thr)) == 6 and int(np.count_nonzero(r0 < thr)) == count - 6
