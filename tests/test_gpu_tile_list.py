"""The list of tiles of the version-2 aligner, made on the device (k_fwd2_items), against the host's (tile_lists): under
IOC_V2_ITEMS_CHECK=1 every slice's list is poisoned, made, read back and compared item by item, and the call fails on the first
difference.

The batch holds every branch of the list's order.  The aligner couples neighbours of its own order of the pairs (by tiles, then by
rows) and a couple's grid is the larger of its two pairs' in either direction, so every shape is in the batch TWICE and forms a
couple of its own kind (a strip is 1024 columns, a coarse row 512 rows, a band one or more coarse rows):
  300 x 300 (one tile; once, last: the odd pair, a couple of one), 300 x 2 500 (one band of 3 strips), 2 500 x 300 (one strip of
  several bands), 1 300 x 1 500 (several bands by 2 strips), 5 000 x 4 100 (several bands by 5 strips);
  two couples of same-transcript pairs of 9 - 10 kb at a low error rate (corridor, probe), and a third couple of that kind with an
  unrelated pair in it, whose grid the probe opens.
The test asserts from the check's IOC_TRACE lines that these grids were planned, that corridors were, and that the probe opened
the couple with the unrelated pair and neither of the other two.
Once in one slice, once in several, once without a corridor (no probe tiles).  Scores and window counts against the host aligner,
computed once.

(tests/fuzz_cases.py offers whole-batch runners only — corridor_batch draws, runs and compares in one function —, so the pairs
are drawn here the way its generators draw related pairs: test_gpu_align._mutate over a common random base.)"""
import random
import re

import pytest

from isonclust2_amd import _lib, api
from tests.test_gpu_align import _host, _mutate

pytestmark = pytest.mark.gpu

K = 11


def _related(rng, n, m, rate=0.02):
    base = bytes(rng.choice(b"ACGT") for _ in range(max(n, m) + 400))
    return _mutate(rng, base, rate)[:n], _mutate(rng, base, rate)[:m]


def _random(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


@pytest.fixture(scope="module")
def batch():
    rng = random.Random(67)
    seqs, pairs = [], []

    def add(q, r, e):
        seqs.extend([q, r])
        pairs.append((len(seqs) - 2, len(seqs) - 1, 0, e))

    # rows x columns, each shape twice (the same count of 512 x 512 tiles and of coarse rows: neighbours in the aligner's order)
    for n, m in ((300, 2500), (2500, 300), (1300, 1500), (5000, 4100)):
        add(*_related(rng, n, m, 0.05), 0.12)
        add(*_related(rng, n - 10, m - 10, 0.05), 0.12)
    # two couples of same-transcript pairs, a third with an unrelated pair of the same size beside a related one
    for n, m in ((9900, 9800), (9850, 9750), (9500, 9450), (9480, 9400), (9100, 9050)):
        add(*_related(rng, n, m), 0.05)
    add(_random(rng, 9090), _random(rng, 9040), 0.05)
    add(*_related(rng, 300, 300, 0.05), 0.12)   # the odd pair, last in the aligner's order: a couple of one
    assert len(pairs) % 2 == 1
    L = _lib.load()
    want = [_host(L, seqs[q], seqs[r], rc, e, K) for q, r, rc, e in pairs]
    return seqs, pairs, want


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _run(ctx, batch, capfd):
    """-> tiles skipped by the corridors, per slice the probe's tile count, all planned grids as (bands, strips, probe grid or
    None, couple of one pair) in the aligner's order, (couples planned a corridor, the couples the probe opened) over all slices"""
    seqs, pairs, want = batch
    ctx.align_set_pool(seqs)
    capfd.readouterr()
    score, win, ratio = ctx.align_pairs(pairs, K)   # (raises when the lists differ: IOC_ERR_STATE names the first index)
    err = capfd.readouterr().err
    for i, (q, _, _, _) in enumerate(pairs):
        hs, hr = want[i]
        assert score[i] == hs, (i, int(score[i]), hs)
        assert ratio[i] == hr and win[i] == round(hr * len(seqs[q])), (i, float(ratio[i]), hr, int(win[i]))
    skipped = [int(x) for x in re.findall(r"corridor: (\d+) of \d+ tiles skipped", err)]
    probe = [int(x) for x in re.findall(r"IOC_V2_ITEMS_CHECK: slice \d+: \d+ tiles \((\d+) of the probe\) equal", err)]
    grids = []
    for line in re.findall(r"IOC_V2_ITEMS_CHECK: slice \d+ grids:(.*)", err):
        for g in line.split():
            m = re.fullmatch(r"(\d+)x(\d+)(?:c(\d+)x(\d+))?(/1)?", g)
            assert m, g
            grids.append((int(m[1]), int(m[2]), (int(m[3]), int(m[4])) if m[3] else None, bool(m[5])))
    verdicts = [(int(a), [int(x) for x in b.split()])
                for a, b in re.findall(r"(\d+) couples with a corridor planned, \d+ opened by the probe \(couples:([ \d]*)\)", err)]
    assert skipped and probe and grids and len(verdicts) == len(probe), err[-2000:]
    assert len(grids) == (len(pairs) + 1) // 2
    # the shapes the batch was built for
    assert any(nb == 1 and ns == 1 and one for nb, ns, _, one in grids), grids            # one tile, a couple of one pair
    assert sum(one for _, _, _, one in grids) == 1, grids
    assert any(nb == 1 and ns == 3 for nb, ns, _, _ in grids), grids                      # one band of three strips
    assert any(nb >= 3 and ns == 1 for nb, ns, _, _ in grids), grids                      # one strip of several bands
    assert any(nb >= 3 and ns == 2 for nb, ns, _, _ in grids), grids                      # several bands by two strips
    assert any(nb >= 5 and ns == 5 for nb, ns, _, _ in grids), grids                      # several bands by five strips
    assert sum(ns >= 9 for _, ns, _, _ in grids) == 3, grids                              # the three couples of long pairs
    return skipped, probe, grids, (sum(a for a, _ in verdicts), [x for _, b in verdicts for x in b])


def test_device_list_equals_host_list_one_slice(ctx, batch, monkeypatch, capfd):
    monkeypatch.setenv("IOC_V2_ITEMS_CHECK", "1")
    monkeypatch.setenv("IOC_TRACE", "1")
    skipped, probe, grids, (planned, opened) = _run(ctx, batch, capfd)
    assert ctx.timings()["align_version"] == 2
    assert skipped[0] > 0, "no corridor was planned: the probe's part of the list is untested"
    assert len(probe) == 1 and probe[0] > 0
    # The three couples of long pairs come first in the aligner's order (most tiles) and were planned a corridor with a probe.  The
    # probe opens the third, which holds the unrelated pair, and leaves the two of low-error same-transcript pairs their corridors.
    # (It may also give up the corridor of a shorter, more divergent couple whose score rate contradicts the plan: k_fwd2_probe.)
    assert all(pg is not None and ns >= 9 for _, ns, pg, _ in grids[:3]), grids
    assert planned >= 3 and 2 in opened and 0 not in opened and 1 not in opened, (planned, opened)


def test_device_list_equals_host_list_several_slices(ctx, batch, monkeypatch, capfd):
    monkeypatch.setenv("IOC_V2_ITEMS_CHECK", "1")
    monkeypatch.setenv("IOC_TRACE", "1")
    monkeypatch.setenv("IOC_ALIGN_CK_BUDGET_MB", "6")
    skipped, probe, grids, (planned, opened) = _run(ctx, batch, capfd)
    assert skipped[0] > 0 and sum(probe) > 0
    assert len(probe) >= 2 and ctx.timings()["align_slices"] == len(probe)   # (no pair was run again: one run's slices)
    assert planned >= 3 and 2 in opened and 0 not in opened and 1 not in opened, (planned, opened)


def test_device_list_equals_host_list_without_a_corridor(ctx, batch, monkeypatch, capfd):
    monkeypatch.setenv("IOC_V2_ITEMS_CHECK", "1")
    monkeypatch.setenv("IOC_TRACE", "1")
    monkeypatch.setenv("IOC_ALIGN_CORRIDOR", "0")
    skipped, probe, grids, (planned, opened) = _run(ctx, batch, capfd)
    assert skipped[0] == 0 and all(p == 0 for p in probe)   # n_probe == 0
    assert planned == 0 and all(pg is None for _, _, pg, _ in grids)
