"""The tapered corridor of the version-2 forward pass and its certificate by exit cells (plan_corridor, k_fwd2_cert, k_fwd2_ends;
DESIGN 5.5).  Pairs of 9 - 12 kb — the smallest whose corridor has bands enough to taper — through the two launch shapes
tests/test_gpu_align_shapes.py forces: a few couples (tiles wait row by row, k_fwd2) and, with 560 one-tile fillers, many couples
(tiles wait for tiles, k_fwd2_w2), in exact and in verdict mode.  Every run
  * comes after the same pairs over the reversed sequences: the arena keeps the last call's checkpoints where this one skips a tile,
    and k_fwd2_cert must not read them;
  * has IOC_V2_CERT_CHECK=1: the library recomputes every pair that kept its corridor on the host (ioc_host_align_corridor) and fails
    the call where the device's restricted score, end cell or bounds differ;
  * is compared pair by pair with the host aligner and with the same call under IOC_ALIGN_CORRIDOR=0 (every tile).
The corridor's model is the prior throughout (IOC_ALIGN_CORRIDOR_NO_FIT=1): what the context has fitted to earlier tests' pairs does
not move a plan."""
import random
import re

import numpy as np
import pytest

from isonclust2_amd import api
from tests.test_gpu_align_shapes import _Batch, _host_answers, _join, _shapes
from tests.test_gpu_tile_list import _random, _related

pytestmark = pytest.mark.gpu

K = 11
THRESHOLD = 0.2
SWITCHES = ("IOC_ALIGN_V2_FEW", "IOC_ALIGN_V2_NO_W2", "IOC_ALIGN_CK_BUDGET_MB", "IOC_ALIGN_WAVES", "IOC_ALIGN_CORRIDOR", "IOC_ALIGN_V2_LINK",
            "IOC_V2_ITEMS_CHECK", "IOC_ALIGN_CORRIDOR_TAPER", "IOC_ALIGN_CORRIDOR_MARGIN", "IOC_V2_CERT_CHECK", "IOC_TRACE")
SHAPES = [pytest.param(False, "rows", "k_fwd2", id="few-rows-k_fwd2"), pytest.param(True, "tiles", "k_fwd2_w2", id="fillers-tiles-k_fwd2_w2")]
MODES = pytest.mark.parametrize("verdict", [False, True], ids=["exact", "verdict"])
_SKIPPED = re.compile(r"corridor: (\d+) of (\d+) tiles skipped")
_AGAIN = re.compile(r"(\d+) of \d+ pairs run again without a corridor")
_CHECKED = re.compile(r"IOC_V2_CERT_CHECK: slice \d+: (\d+) pairs equal the host's \((\d+) with a tapered corridor, (\d+) refuted\)")


def _answered(b):
    return b.seqs, b.pairs, _host_answers(b)


def _light(rng, s, rate=0.01):
    from tests.test_gpu_align import _mutate
    return _mutate(rng, s, rate)


@pytest.fixture(scope="module")
def fillers():
    rng = random.Random(81)
    b = _Batch()
    for t in range(560):
        b.add(*_related(rng, rng.randint(40, 120), rng.randint(40, 120), rng.uniform(0.05, 0.10)), t % 2, (0.05, 0.12, 0.2)[t % 3])
    return _answered(b)


@pytest.fixture(scope="module")
def related():
    """per summed error rate a couple of same-transcript pairs, e handed in as it is (0.03: 11.8 kb — the prior's half width of
    0.10 x length has to reach one strip for a corridor to be planned at all)"""
    out = {}
    for e, (n, m) in ((0.03, (11800, 11700)), (0.07, (9900, 9800)), (0.12, (9900, 9800))):
        rng = random.Random(int(e * 1000))
        b = _Batch()
        b.add(*_related(rng, n, m, e / 2), 0, e)
        b.add(*_related(rng, n - 60, m - 40, e / 2), 1, e)
        out[e] = _answered(b)
    return out


def _with_companion(rng, q, r, e):
    """the pair under test first (the heavier), a related pair of nearly its size beside it: one couple"""
    b = _Batch()
    b.add(q, r, 0, e)
    b.add(*_related(rng, len(q) - 30, len(r) - 30, 0.02), 0, e)
    return _answered(b)


@pytest.fixture(scope="module")
def deletion_early():
    """10 kb against the same without 2.5 kb in its first fifth, both 10 kb long: the path runs 2.5 kb left of the diagonal from row
    4000 on — inside the top width of e = 0.12 (0.26 x length), outside the taper further down"""
    rng = random.Random(82)
    base = _random(rng, 12500)
    return _with_companion(rng, _light(rng, base[:10000]), _light(rng, base[:1500] + base[4000:12500]), 0.12)


@pytest.fixture(scope="module")
def deletion_late():
    rng = random.Random(83)
    base = _random(rng, 12500)
    return _with_companion(rng, _light(rng, base[:10000]), _light(rng, base[:8000] + base[10500:12500]), 0.12)


@pytest.fixture(scope="module")
def repeated_block():
    """The query's last 3 kb also stand 2.5 kb left of the diagonal in the reference, in place of what the diagonal would match there:
    a route that leaves the diagonal at row 4500 and runs through cells the taper skips, late in the grid, scores about 12 000.
    [0] the reference ends as the query does: the diagonal's route scores more (14 745 — at gap open 2 the unrelated 3 kb in
    between align at + 0.4 per base), whatever the certificate says the answer is the diagonal's; [1] the reference ends in
    unrelated bases: the route through the skipped cells is the alignment, the pair must come back refuted."""
    rng = random.Random(84)
    base = _random(rng, 10000)
    decoy = _with_companion(rng, _light(rng, base), _light(rng, base[:4500] + base[7000:10000] + base[7500:10000]), 0.12)
    best = _with_companion(rng, _light(rng, base), _light(rng, base[:4500] + base[7000:10000] + _random(rng, 2500)), 0.12)
    return decoy, best


@pytest.fixture(scope="module")
def unequal():
    """a couple of 9.9 kb and 8 kb: the shorter pair's exit cells are those inside its own rows and columns"""
    rng = random.Random(85)
    b = _Batch()
    b.add(*_related(rng, 9900, 9800, 0.035), 0, 0.07)
    b.add(*_related(rng, 8000, 7900, 0.035), 0, 0.07)
    return _answered(b)


@pytest.fixture(scope="module")
def short_pairs():
    """4.2 kb: nine bands of 512 rows over five strips"""
    rng = random.Random(86)
    b = _Batch()
    b.add(*_related(rng, 4200, 4300, 0.08), 0, 0.2)
    b.add(*_related(rng, 4150, 4250, 0.08), 0, 0.2)
    return _answered(b)


@pytest.fixture(scope="module")
def long_query():
    """12 kb of query against 10 kb of reference: the last band lies wholly left of the taper's columns — no taper can be planned,
    the couple gets one width and the parent's certificate"""
    rng = random.Random(87)
    b = _Batch()
    b.add(*_related(rng, 12000, 10000, 0.035), 0, 0.07)
    b.add(*_related(rng, 11950, 9950, 0.035), 0, 0.07)
    return _answered(b)


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _call(ctx, batch, monkeypatch, capfd, env, verdict, reversed_first=True):
    """one ioc_align_pairs under `env` (+ the prior, + IOC_TRACE) -> ((score, windows, ratio), stderr)"""
    seqs, pairs, _ = batch
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("IOC_ALIGN_CORRIDOR_NO_FIT", "1")
    for name, v in env.items():
        if name != "IOC_V2_CERT_CHECK":
            monkeypatch.setenv(name, v)
    ctx.align_set_verdict_threshold(THRESHOLD if verdict else 0.0)
    try:
        if reversed_first:
            ctx.align_set_pool([s[::-1] for s in seqs])
            ctx.align_pairs(pairs, K)
        for name, v in env.items():
            monkeypatch.setenv(name, v)
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
    return (np.array(score), np.array(win), np.array(ratio)), err


def _same(a, b, verdict):
    assert np.array_equal(a[0], b[0]), np.nonzero(a[0] != b[0])
    if verdict:
        assert np.array_equal(a[2] >= THRESHOLD, b[2] >= THRESHOLD)
    else:
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _run(ctx, batch, fillers, monkeypatch, capfd, with_fillers, wait, kernel, verdict, env=None):
    """the batch (beside the fillers) under the taper with the host's check, against the host aligner and against every tile
    -> (answers, tiles skipped in the first call, pairs run again, (pairs checked, tapered, refuted) by IOC_V2_CERT_CHECK, stderr)"""
    n_long = len(batch[1])
    batch = _join(batch, fillers) if with_fillers else batch
    seqs, pairs, want = batch
    got, err = _call(ctx, batch, monkeypatch, capfd, dict(env or {}, IOC_V2_CERT_CHECK="1"), verdict)
    calls = _shapes(err)
    sl = calls[0]["slices"][0]   # (the long pairs are the heaviest: first in the aligner's order)
    assert sl["wait"] == wait and sl["kernel"] == kernel, calls
    bad = []
    for i, (q, r, rc, e) in enumerate(pairs):
        hs, hr = want[i]
        ok = got[0][i] == hs and ((got[2][i] >= THRESHOLD) == (hr >= THRESHOLD) if verdict else (got[2][i] == hr and got[1][i] == round(hr * len(seqs[q]))))
        if not ok:
            bad.append((i, len(seqs[q]), len(seqs[r]), rc, e, int(got[0][i]), hs, float(got[2][i]), hr))
    assert not bad, f"{len(bad)} of {len(pairs)} pairs differ from the host aligner: {bad[:5]}"
    every, _ = _call(ctx, batch, monkeypatch, capfd, dict(env or {}, IOC_ALIGN_CORRIDOR="0"), verdict, reversed_first=False)
    _same(got, every, verdict)
    skipped = [int(m[1]) for m in _SKIPPED.finditer(err)]
    again = sum(int(m[1]) for m in _AGAIN.finditer(err))
    checked = [sum(int(m[x]) for m in _CHECKED.finditer(err)) for x in (1, 2, 3)]
    assert skipped and _CHECKED.search(err), err[-3000:]
    assert checked[0] <= n_long
    with capfd.disabled():   # (the figures of every run, whatever the asserts say: pytest -s)
        print(f"taper: fillers {with_fillers}, verdict {verdict}, env {env}: skipped {skipped}, run again {again}, checked / tapered / refuted {checked}")
    return got, skipped[0], again, checked, err


def _skipped_under(ctx, batch, monkeypatch, capfd, env):
    _, err = _call(ctx, batch, monkeypatch, capfd, env, False, reversed_first=False)
    return int(_SKIPPED.search(err)[1])


@MODES
@pytest.mark.parametrize("with_fillers, wait, kernel", SHAPES)
@pytest.mark.parametrize("e", [0.03, 0.07, 0.12])
def test_related_pairs_taper_and_pass(ctx, related, fillers, monkeypatch, capfd, e, with_fillers, wait, kernel, verdict):
    _, skipped, again, checked, _ = _run(ctx, related[e], fillers, monkeypatch, capfd, with_fillers, wait, kernel, verdict)
    uniform = _skipped_under(ctx, related[e], monkeypatch, capfd, {"IOC_ALIGN_CORRIDOR_TAPER": "0"})
    assert skipped > uniform > 0, (skipped, uniform)
    assert checked == [2, 2, 0] and again == 0, (checked, again)


@MODES
@pytest.mark.parametrize("with_fillers, wait, kernel", SHAPES)
def test_deletion_in_the_first_fifth_is_refuted(ctx, deletion_early, fillers, monkeypatch, capfd, with_fillers, wait, kernel, verdict):
    _, skipped, again, checked, _ = _run(ctx, deletion_early, fillers, monkeypatch, capfd, with_fillers, wait, kernel, verdict)
    assert checked[1] == 2 and checked[2] >= 1 and again >= 1, (checked, again)


@MODES
@pytest.mark.parametrize("with_fillers, wait, kernel", SHAPES)
def test_deletion_in_the_last_fifth(ctx, deletion_late, fillers, monkeypatch, capfd, with_fillers, wait, kernel, verdict):
    _, skipped, again, checked, _ = _run(ctx, deletion_late, fillers, monkeypatch, capfd, with_fillers, wait, kernel, verdict)
    assert checked[1] == 2, checked


@MODES
@pytest.mark.parametrize("with_fillers, wait, kernel", SHAPES)
@pytest.mark.parametrize("which", [0, 1], ids=["second-best", "best"])
def test_high_scoring_route_through_skipped_cells(ctx, repeated_block, fillers, monkeypatch, capfd, with_fillers, wait, kernel, verdict, which):
    _, skipped, again, checked, _ = _run(ctx, repeated_block[which], fillers, monkeypatch, capfd, with_fillers, wait, kernel, verdict)
    assert checked[1] == 2, checked
    if which:
        assert checked[2] >= 1 and again >= 1, (checked, again)


@MODES
@pytest.mark.parametrize("with_fillers, wait, kernel", SHAPES)
def test_couple_of_two_lengths(ctx, unequal, fillers, monkeypatch, capfd, with_fillers, wait, kernel, verdict):
    _, skipped, again, checked, _ = _run(ctx, unequal, fillers, monkeypatch, capfd, with_fillers, wait, kernel, verdict)
    assert checked == [2, 2, 0] and again == 0, (checked, again)


@MODES
@pytest.mark.parametrize("with_fillers, wait, kernel", SHAPES)
def test_short_pairs(ctx, short_pairs, fillers, monkeypatch, capfd, with_fillers, wait, kernel, verdict):
    _, skipped, again, checked, _ = _run(ctx, short_pairs, fillers, monkeypatch, capfd, with_fillers, wait, kernel, verdict)
    assert checked[0] == 2 and again == 0, (checked, again)


@MODES
@pytest.mark.parametrize("with_fillers, wait, kernel", SHAPES)
def test_no_taper_fits_one_width_instead(ctx, long_query, fillers, monkeypatch, capfd, with_fillers, wait, kernel, verdict):
    _, skipped, again, checked, _ = _run(ctx, long_query, fillers, monkeypatch, capfd, with_fillers, wait, kernel, verdict)
    assert skipped == _skipped_under(ctx, long_query, monkeypatch, capfd, {"IOC_ALIGN_CORRIDOR_TAPER": "0"}) > 0
    assert checked[:2] == [2, 0], checked


# tiles skipped by the commit before the taper (its library, these fixtures, the prior): what IOC_ALIGN_CORRIDOR_TAPER=0 and a fixed
# fraction must still plan
PARENT_SKIPPED = {"related_0.07": 56, "related_0.07_fixed_0.45": 20, "unequal": 56}


def test_switches_keep_the_parents_plan(ctx, related, unequal, monkeypatch, capfd):
    got = {"related_0.07": _skipped_under(ctx, related[0.07], monkeypatch, capfd, {"IOC_ALIGN_CORRIDOR_TAPER": "0"}),
           "related_0.07_fixed_0.45": _skipped_under(ctx, related[0.07], monkeypatch, capfd, {"IOC_ALIGN_CORRIDOR": "0.45"}),
           "unequal": _skipped_under(ctx, unequal, monkeypatch, capfd, {"IOC_ALIGN_CORRIDOR_TAPER": "0"})}
    with capfd.disabled():
        print("taper: switches:", got)
    assert got == PARENT_SKIPPED
    # (a fixed fraction keeps the parent's certificate too: nothing is vouched for by exit cells)
    _, err = _call(ctx, related[0.07], monkeypatch, capfd, {"IOC_ALIGN_CORRIDOR": "0.45", "IOC_V2_CERT_CHECK": "1"}, False)
    assert [int(m[2]) for m in _CHECKED.finditer(err)] == [0], err[-2000:]


@pytest.mark.parametrize("with_fillers, wait, kernel", SHAPES)
def test_taper_without_links(ctx, related, deletion_early, fillers, monkeypatch, capfd, with_fillers, wait, kernel):
    for batch in (related[0.07], deletion_early):
        on = _run(ctx, batch, fillers, monkeypatch, capfd, with_fillers, wait, kernel, False)
        off = _run(ctx, batch, fillers, monkeypatch, capfd, with_fillers, wait, kernel, False, env={"IOC_ALIGN_V2_LINK": "0"})
        _same(on[0], off[0], False)
        assert on[1:4] == off[1:4], (on[1:4], off[1:4])
