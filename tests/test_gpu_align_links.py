"""Links of the version-2 forward pass (v2_fwd_body): a wave that is about to finish tile (band b, strip p) goes on into
(b + 1, p) with its lanes' skew and registers as they are when that takes no wait — the tile has no left side (strip 0, or the
leftmost strip of its band's corridor), or its left neighbour is done.  IOC_ALIGN_V2_LINK=0 switches them off.  Every run here is
compared with the host aligner pair by pair, the run with links with the run without, and the count of links is read from the
`aligner v2: links:` line of IOC_TRACE.  Links with the left tile done depend on timing: their count is printed, never asserted.

Edge pairs: rows 2048 + d and 3072 + d, d in EDGE_D, so that the last band boundary falls on, before and after the kernel's 4-row
steps, the 128 rows the look-ahead ring fetches ahead (the decision falls 32 steps before the boundary) and the 512-row
checkpoint pitch; d = 1 .. 4 leave a last band of ONE row block, which ends before the band above is published in the loop.
Columns: 2 - 4 strips with a ragged last one.  Each shape twice, so that the aligner forms couples of it.  A batch of this size
runs in bands of one coarse row (512 rows = 128 row blocks: the shortest band a run may go on from).

Every launch shape of test_gpu_align_shapes.py that a batch of this size reaches: whole-tile waits with k_fwd2_w2 and with k_fwd2
(IOC_ALIGN_V2_FEW=0, IOC_ALIGN_V2_NO_W2), row-by-row waits with k_fwd2 (IOC_ALIGN_V2_FEW=100000); each run after the same pairs over
the reversed sequences (test_gpu_align_shapes._run: stale checkpoints must not stand in for a dependency that was skipped)."""
import random
import re

import numpy as np
import pytest

from isonclust2_amd import api
from tests.test_gpu_align_shapes import _Batch, _host_answers, _shapes
from tests.test_gpu_tile_list import _random, _related

pytestmark = pytest.mark.gpu

K = 11
EDGE_D = (-4, -1, 0, 1, 4, 128, 511, 512, 513)
CORRIDOR = "0.45"   # x the longer side: a half width of one strip or more (a corridor needs that) for the 3072-row shapes
THRESHOLD = 0.2     # verdict mode
SHAPES = [
    pytest.param({"IOC_ALIGN_V2_FEW": "0"}, "tiles", "k_fwd2_w2", id="tiles-w2"),
    pytest.param({"IOC_ALIGN_V2_FEW": "0", "IOC_ALIGN_V2_NO_W2": "1"}, "tiles", "k_fwd2", id="tiles-w3"),
    pytest.param({"IOC_ALIGN_V2_FEW": "100000"}, "rows", "k_fwd2", id="rows-w3"),
    pytest.param({"IOC_ALIGN_V2_FEW": "100000", "IOC_ALIGN_V2_NO_W2": "1"}, "rows", "k_fwd2", id="rows-w3-no-w2"),
]
_LINKS = re.compile(r"aligner v2: links: (\d+) of (\d+) \((\d+) without a left side, (\d+) with the left tile done\)")


def _answered(b):
    return b.seqs, b.pairs, _host_answers(b)


@pytest.fixture(scope="module")
def edge():
    """36 related pairs (2 % error): rows 2048 + d over 2 - 3 strips, rows 3072 + d over 4 strips"""
    rng = random.Random(20260)
    b = _Batch()
    for i, d in enumerate(EDGE_D):
        for n, m in ((2048 + d, (1900, 2040, 2300, 2500)[i % 4]), (3072 + d, (3100, 3300, 3500)[i % 3])):
            rc, e = rng.randint(0, 1), rng.choice((0.05, 0.12))
            for _ in range(2):
                b.add(*_related(rng, n, m), rc, e)
    return _answered(b)


@pytest.fixture(scope="module")
def refuted():
    """Two copies of one sequence, each without another block of 1100 bases (tests/test_gpu_align_ops.refuted_pairs with shorter
    blocks): equal lengths, a score 2 x 1100 + two long gaps below what the corridor's certificate asks for — the pair comes back
    refuted and runs again with every tile.  Beside it a pair the corridor vouches for."""
    rng = random.Random(72)
    base = _random(rng, 9000)
    b = _Batch()
    b.add(base[:3000] + base[4100:], base[:6000] + base[7100:], 0, 0.05)
    b.add(*_related(rng, 7900, 7850), 0, 0.05)
    return _answered(b)


@pytest.fixture(scope="module")
def wrong():
    """an unrelated pair of 4200 x 4300 bases beside a related one of its size"""
    rng = random.Random(73)
    b = _Batch()
    b.add(_random(rng, 4200), _random(rng, 4300), 0, 0.05)
    b.add(*_related(rng, 4200, 4300), 0, 0.05)
    return _answered(b)


@pytest.fixture(scope="module")
def unequal():
    """Two couples of one batch each, one pair a band shorter than the other: the longer one is the heavier (it comes first in the
    aligner's order: the low halves go on alone), and the shorter one is (four strips against two: the HIGH halves go on alone —
    the idle low halves are put back to the bias once per band)."""
    rng = random.Random(74)
    one, two = _Batch(), _Batch()
    one.add(*_related(rng, 3172, 2100), 0, 0.05)
    one.add(*_related(rng, 2660, 2100), 0, 0.05)
    two.add(*_related(rng, 2660, 4000, 0.01), 0, 0.05)
    two.add(*_related(rng, 3172, 2100), 0, 0.05)
    return _answered(one), _answered(two)


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _run(ctx, batch, monkeypatch, capfd, env, verdict=False):
    """test_gpu_align_shapes._run with a verdict mode: one ioc_align_pairs under `env` and IOC_TRACE behind the same call over the
    reversed sequences; every pair against the host.  -> ((score, windows, ratio), calls as _shapes gives them, (links, tiles
    computed, links without a left side, links with the left tile done) over all calls, grids (bands, strips) per couple, stderr)"""
    seqs, pairs, want = batch
    for name in ("IOC_ALIGN_V2_FEW", "IOC_ALIGN_V2_NO_W2", "IOC_ALIGN_CK_BUDGET_MB", "IOC_ALIGN_WAVES", "IOC_ALIGN_CORRIDOR", "IOC_ALIGN_V2_LINK",
                 "IOC_V2_ITEMS_CHECK"):
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    ctx.align_set_verdict_threshold(THRESHOLD if verdict else 0.0)
    try:
        ctx.align_set_pool([s[::-1] for s in seqs])
        ctx.align_pairs(pairs, K)
        monkeypatch.setenv("IOC_TRACE", "1")
        ctx.align_set_pool(seqs)
        refused = ctx.timings()["n_align_refused"]
        capfd.readouterr()
        score, win, ratio = ctx.align_pairs(pairs, K)
        err = capfd.readouterr().err
    finally:
        ctx.align_set_verdict_threshold(0.0)
        monkeypatch.delenv("IOC_TRACE", raising=False)
    tm = ctx.timings()
    assert tm["align_version"] == 2 and tm["n_align_refused"] == refused, (tm["align_version"], tm["n_align_refused"] - refused)
    bad = []
    for i, (q, r, rc, e) in enumerate(pairs):
        hs, hr = want[i]
        if verdict:
            ok = score[i] == hs and (ratio[i] >= THRESHOLD) == (hr >= THRESHOLD)
        else:
            ok = score[i] == hs and ratio[i] == hr and win[i] == round(hr * len(seqs[q]))
        if not ok:
            bad.append((i, len(seqs[q]), len(seqs[r]), rc, e, int(score[i]), hs, float(ratio[i]), hr, int(win[i])))
    assert not bad, f"{len(bad)} of {len(pairs)} pairs differ from the host aligner under {env}, verdict mode {verdict}: {bad[:5]}"
    found = [tuple(map(int, m.groups())) for m in _LINKS.finditer(err)]
    calls = _shapes(err)
    assert calls and len(found) == len(calls), err[-2000:]
    links = tuple(sum(f[x] for f in found) for x in range(4))
    assert links[0] == links[2] + links[3] and links[0] < links[1], found
    grids = []   # (IOC_V2_ITEMS_CHECK alone: a couple's bands x strips, then its probe grid if it has one, as in test_gpu_tile_list.py)
    for line in re.findall(r"IOC_V2_ITEMS_CHECK: slice \d+ grids:(.*)", err):
        for g in line.split():
            m = re.fullmatch(r"(\d+)x(\d+)(?:c\d+x\d+)?(?:/1)?", g)
            assert m, g
            grids.append((int(m[1]), int(m[2])))
    with capfd.disabled():   # (the figures of every run, whatever the asserts say: pytest -s)
        print("links:", env, "verdict" if verdict else "exact", found)
    return (np.array(score), np.array(win), np.array(ratio)), calls, links, grids, err


def _both(ctx, batch, monkeypatch, capfd, env, verdict=False):
    """the run with links and the run with IOC_ALIGN_V2_LINK=0: the same answers, no link in the second"""
    on = _run(ctx, batch, monkeypatch, capfd, env, verdict)
    off = _run(ctx, batch, monkeypatch, capfd, dict(env, IOC_ALIGN_V2_LINK="0"), verdict)
    assert np.array_equal(on[0][0], off[0][0])
    if verdict:
        assert np.array_equal(on[0][2] >= THRESHOLD, off[0][2] >= THRESHOLD)
    else:
        assert np.array_equal(on[0][1], off[0][1]) and np.array_equal(on[0][2], off[0][2])
    assert off[2][0] == 0 and off[2][1] == on[2][1], (on[2], off[2])   # (the same tiles computed, none of them entered by a link)
    return on, off


def _assert_shape(calls, wait, kernel):
    assert all(s["wait"] == wait and s["kernel"] == kernel for c in calls for s in c["slices"]), (wait, kernel, calls)


@pytest.mark.parametrize("env, wait, kernel", SHAPES)
@pytest.mark.parametrize("verdict", [False, True], ids=["exact", "verdict"])
def test_corridor_links(ctx, edge, monkeypatch, capfd, env, wait, kernel, verdict):
    on, off = _both(ctx, edge, monkeypatch, capfd, dict(env, IOC_ALIGN_CORRIDOR=CORRIDOR), verdict)
    for r in (on, off):
        _assert_shape(r[1], wait, kernel)
        skipped = [int(x) for x in re.findall(r"corridor: (\d+) of \d+ tiles skipped", r[4])]
        assert skipped and skipped[0] > 0, "no corridor was planned"
    assert on[2][2] >= 1, on[2]


@pytest.mark.parametrize("env, wait, kernel", SHAPES)
@pytest.mark.parametrize("verdict", [False, True], ids=["exact", "verdict"])
def test_full_grid_links(ctx, edge, monkeypatch, capfd, env, wait, kernel, verdict):
    """no corridor: strip 0 has no left side in any band — one wave runs it from the top to the bottom of every couple"""
    on, off = _both(ctx, edge, monkeypatch, capfd, dict(env, IOC_ALIGN_CORRIDOR="0", IOC_V2_ITEMS_CHECK="1"), verdict)
    for r in (on, off):
        _assert_shape(r[1], wait, kernel)
    grids = on[3]
    assert len(grids) == (len(edge[1]) + 1) // 2 and all(nb >= 4 for nb, _ in grids), grids
    assert on[2][2] >= sum(nb - 1 for nb, _ in grids), (on[2], grids)


@pytest.mark.parametrize("env, wait, kernel", SHAPES[:3])
def test_refuted_pair_runs_again_with_every_tile(ctx, refuted, monkeypatch, capfd, env, wait, kernel):
    on, off = _both(ctx, refuted, monkeypatch, capfd, dict(env, IOC_ALIGN_CORRIDOR="0.15"))
    again = [re.findall(r"(\d+) of 2 pairs run again without a corridor", r[4]) for r in (on, off)]
    assert again[0] == again[1] and again[0] and int(again[0][0]) >= 1, again
    assert on[2][2] >= 1, on[2]


@pytest.mark.parametrize("env, wait, kernel", SHAPES[:3])
def test_wrong_candidate_pair(ctx, wrong, monkeypatch, capfd, env, wait, kernel):
    """(the probe opens its couple's grid, or the certificate refutes it and it runs again with every tile: either way as without links)"""
    on, off = _both(ctx, wrong, monkeypatch, capfd, dict(env, IOC_ALIGN_CORRIDOR="0.3"))   # (a half width of 1290 columns: a corridor is planned)
    assert len(on[1]) == len(off[1]) and ("run again without a corridor" in on[4]) == ("run again without a corridor" in off[4])
    assert on[2][2] >= 1, on[2]


@pytest.mark.parametrize("env, wait, kernel", SHAPES[:3])
@pytest.mark.parametrize("which", [0, 1], ids=["low-half-goes-on", "high-half-goes-on"])
def test_couple_of_unequal_pairs(ctx, unequal, monkeypatch, capfd, env, wait, kernel, which):
    on, off = _both(ctx, unequal[which], monkeypatch, capfd, dict(env, IOC_ALIGN_CORRIDOR="0", IOC_V2_ITEMS_CHECK="1"))
    (nb, ns), = on[3]
    assert nb == 7 and ns == (3, 4)[which], on[3]
    assert on[2][2] >= nb - 1, on[2]   # (strip 0 down all seven bands: the last link with one pair only)
