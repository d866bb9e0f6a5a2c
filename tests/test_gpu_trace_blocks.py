"""The block recomputation of the version-2 traceback at every shape of 512 x 512 block a walk can enter: ioc_align_pairs and
ioc_align_pairs_ops against the host aligner, as tests/test_gpu_trace_tiles.py does for the tiles (its _check: score, ratio and
operation bytes equal; no tolerance, nothing left out).  A block is recomputed in one of three shapes: lanes along the columns
with 8 columns per lane (more than 256 columns), with 4 (65 .. 256), and lanes along the ROWS with 8 rows per lane (<= 64 columns);
a walk enters a block at any point, so every shape meets blocks of 1 .. 512 rows.  The pairs are built so that the walks meet the
boundaries between the shapes (64 and 256 columns), the 8-row boundaries of the lanes, and narrow blocks of few rows — and the
test derives from the host aligner's operation bytes which blocks every walk enters and asserts that every class occurs."""
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests.align_ops_checks import revcomp
from tests.test_gpu_align import _mutate
from tests.test_gpu_trace_tiles import _check, _clipped, _host, _rand, _subst

E_CLASSES = (0.005, 0.03, 0.08, 0.2)      # one error sum per gap-open class of ioc_host_gap_open: 5, 4, 3, 2
KS = (5, 11)
BLOCK = 512
OFFSETS = (7, 8, 9, 56, 57, 63, 64, 65, 66, 129, 255, 256, 257, 383, 385, 447, 448, 449, 511)
RAGGED_ROWS = (1, 7, 8, 9, 127, 129, 511)
RAGGED_COLS = (1, 8, 63, 64, 65)
CORES = (1536, 1600, 1792, 1560, 1700, 1664, 1920)   # lengths of the common part (with the offset: 1 500 .. 3 600 bases)


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def offset_pairs():
    """Pairs on the diagonal j = i + d and mirrored (i = j + d) for the block-level offsets: a walk enters blocks of d columns by
    512 rows and of 512 columns by 512 - d rows (mirrored: d rows by 512 columns, 512 rows by 512 - d columns).  Every third
    pair has insertions and deletions at 6 %: its walk leaves and re-enters the narrow blocks."""
    rng = random.Random(211)
    seqs, pairs = [], []
    for x, d in enumerate(OFFSETS):
        for mirror in (False, True):
            y = 2 * x + int(mirror)
            n = CORES[y % len(CORES)]
            if y % 3 == 2:
                core = _rand(rng, n)
                longer, shorter = _rand(rng, d) + _mutate(rng, core, 0.06), _mutate(rng, core, 0.06)
                q, r = (longer, shorter) if mirror else (shorter, longer)
            else:
                q, r = _clipped(rng, d, mirror, n)
            rc = y % 4 == 1
            seqs += [q, revcomp(r) if rc else r]
            pairs.append((len(seqs) - 2, len(seqs) - 1, int(rc), E_CLASSES[(x + int(mirror)) % 4]))
    return seqs, pairs


def ragged_pairs():
    """Lengths n = 512 a + rows, m = 512 b + columns, the common part at the END of both (its last bases identical: the alignment
    ends in the corner): the first block the walk enters has `rows` rows and `columns` columns."""
    rng = random.Random(223)
    seqs, pairs, want = [], [], []
    for x, rows in enumerate(RAGGED_ROWS):
        for y, cols in enumerate(RAGGED_COLS):
            z = x * len(RAGGED_COLS) + y
            n, m = 1536 + rows, (1536, 2048, 2560)[z % 3] + cols
            core = _rand(rng, 1450)
            if z % 3 == 1:
                cq, cr = _mutate(rng, core[:-12], 0.06) + core[-12:], _mutate(rng, core[:-12], 0.06) + core[-12:]
            else:
                cq, cr = _subst(rng, core[:-12], 0.04) + core[-12:], core
            q, r = _rand(rng, n - len(cq)) + cq, _rand(rng, m - len(cr)) + cr
            assert len(q) == n and len(r) == m
            rc = z % 5 == 2
            seqs += [q, revcomp(r) if rc else r]
            pairs.append((len(seqs) - 2, len(seqs) - 1, int(rc), E_CLASSES[z % 4]))
            want.append((rows, cols))
    return seqs, pairs, want


def blocks_entered(ops, n, m):
    """(rows, columns) of every block a walk enters, from the alignment's operation bytes: the walk starts where the trailing end
    gaps begin and goes back; the block of the cell (i, j) is that of its tile, floor((i - 1) / 128) 128 rounded down to 512
    (columns alike), and its extents are clipped to the point where the walk enters it — the arithmetic of trace2_body."""
    t = len(ops)
    while t and ops[t - 1] in b"id":
        t -= 1
    i, j = n - ops[t:].count(b"i"), m - ops[t:].count(b"d")
    out, cur = [], None
    for op in reversed(ops[:t]):
        if i == 0 or j == 0 or op in b"id":
            break
        rb, cb = (i - 1) // 128 * 128 // BLOCK * BLOCK, (j - 1) // 128 * 128 // BLOCK * BLOCK
        if (rb, cb) != cur:
            cur = (rb, cb)
            out.append((i - rb, j - cb))
        if op in b"=X":
            i, j = i - 1, j - 1
        elif op == 0x49:   # 'I': a base of the query
            i -= 1
        else:
            j -= 1
    return out


def shape_classes(shapes):
    """How often each class of block occurs among (rows, columns) shapes."""
    return {
        "<= 64 columns, 512 rows": sum(c <= 64 and r == BLOCK for r, c in shapes),
        "<= 64 columns, < 512 rows": sum(c <= 64 and r < BLOCK for r, c in shapes),
        "65 .. 256 columns": sum(64 < c <= 256 for r, c in shapes),
        "> 256 columns": sum(c > 256 for r, c in shapes),
        "<= 64 rows": sum(r <= 64 for r, c in shapes),
    }


def host_shapes(seqs, pairs):
    return [blocks_entered(_host(seqs[qi], seqs[ri], rc, e)[2], len(seqs[qi]), len(seqs[ri])) for qi, ri, rc, e in pairs]


def _verdicts(ctx, seqs, pairs, k=11):
    """With a verdict threshold every pair gets the verdict of the host's ratio: at the threshold the existing tests use and at
    the median of the host's own ratios (pairs on either side of it: walks that stop early because the count is reached, and
    because it cannot be reached any more)."""
    L = _lib.load()
    hr = []
    for qi, ri, rc, e in pairs:
        _, comp, _ = _host(seqs[qi], seqs[ri], rc, e)
        hr.append(L.ioc_host_aln_ratio(comp, len(comp), e, len(seqs[qi]), k))
    hr = np.array(hr)
    ctx.align_set_pool(seqs)
    try:
        for thr in (0.2, float(np.median(hr))):
            ctx.align_set_verdict_threshold(thr)
            _, _, r1 = ctx.align_pairs(pairs, k)
            assert np.array_equal(r1 >= thr, hr >= thr), thr
    finally:
        ctx.align_set_verdict_threshold(0.0)


@pytest.mark.gpu
def test_block_level_offsets(ctx):
    """Offsets 7 .. 511 between the two sequences, both orientations, every gap-open class, some references reverse-complemented,
    a third with indels: narrow blocks of 512 rows, blocks of 512 - d rows, blocks of d rows; both sides of 64 and 256 columns."""
    seqs, pairs = offset_pairs()
    assert len(pairs) == 2 * len(OFFSETS) and {e for _, _, _, e in pairs} == set(E_CLASSES) and any(rc for _, _, rc, _ in pairs)
    assert all(1500 <= len(s) <= 3600 for s in seqs)
    _check(ctx, seqs, pairs, ks=KS)
    _verdicts(ctx, seqs, pairs)
    for y, sh in enumerate(host_shapes(seqs, pairs)):
        d, mirror = OFFSETS[y // 2], bool(y % 2)
        if y % 3 != 2:   # (substitutions only: the walk stays on its diagonal)
            assert ((d, BLOCK) if mirror else (BLOCK, d)) in sh and ((BLOCK, BLOCK - d) if mirror else (BLOCK - d, BLOCK)) in sh, (d, mirror, sh)


@pytest.mark.gpu
def test_ragged_first_block(ctx):
    """The first block of the walk with each of 1, 7, 8, 9, 127, 129, 511 rows and each of 1, 8, 63, 64, 65 columns."""
    seqs, pairs, want = ragged_pairs()
    assert len(pairs) == len(RAGGED_ROWS) * len(RAGGED_COLS) and all(1500 <= len(s) <= 3600 for s in seqs)
    _check(ctx, seqs, pairs, ks=KS)
    _verdicts(ctx, seqs, pairs)
    for sh, w in zip(host_shapes(seqs, pairs), want):
        assert sh[0] == w, (sh[0], w)


def test_every_shape_class_occurs():
    """What keeps the two tests above honest: among the blocks their walks enter (derived from the host aligner's operation bytes,
    no GPU involved) every class of shape occurs at least three times."""
    shapes = []
    for seqs, pairs in (offset_pairs(), ragged_pairs()[:2]):
        for sh in host_shapes(seqs, pairs):
            shapes += sh
    classes = shape_classes(shapes)
    assert all(v >= 3 for v in classes.values()), classes
