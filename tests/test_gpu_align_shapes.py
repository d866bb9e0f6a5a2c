"""The version-2 forward pass (v2_fwd_body) in every shape align_v2_run / v2_slice launch it in, against the host aligner at the
kernel's edge sizes.  The shape is chosen by the call's couple count and by what the chip reports:
  how a tile waits for its left neighbour: row by row (v2_wait_rows, a slice of at most few_limit = 128 couples) or for the whole
      tile (v2_wait on its flag);
  the build of the kernel: k_fwd2 (three waves per SIMD) or k_fwd2_w2 (two; launches of at most 2 workgroups per CU);
  the bands: band_target asks for 12 .. 40 from the call's couple count (at most 17 in a few-couples call), and plan_bands cuts bands
      of one coarse row (512 rows) only when more than 16 are wanted — two coarse rows or more otherwise.
A batch of a few dozen pairs only ever runs as rows / k_fwd2 / target 17; the benchmark's sahlin step runs as tiles / k_fwd2_w2 /
target 12.  Here the same edge pairs go through six shapes (run a .. f below), each ASSERTED from the `aligner v2: shape:` lines
IOC_TRACE prints — a run in another shape fails instead of passing for nothing —, and every pair's score, window count and ratio
must equal the host's.  align_version must be 2 and n_align_refused must not move: a bounded wait that runs out falls back to
version 1 and would hide the shape.

Edge pairs: rows n = 1024 + d.  Row 1024 starts a band whether bands are one or two coarse rows tall, so the last band has d rows;
d from the kernel's constants: 4-row steps (FW_R), the first wait for min(32, nblk_band) blocks = 128 rows, need_rows =
min(16 (blk + 2), nblk_band), publishing from step 64 = 256 rows, the 512-row checkpoint pitch.  Columns m cycled over {1500, 1536,
1537, 2049, 2500, 3073}: a tile always has a left neighbour, and the last strip takes both of its widths (8 columns per lane when
at most 512 columns remain).  Every such shape twice, so that the aligner — which couples neighbours of its own order of the pairs —
forms couples of it; the same n once more over m = 900 (one strip: no left wait), and 3073 x 3073, 2560 x 1025, 300 x 2500 and an
unrelated 2049 x 2049.  Fillers: 560 related pairs of 40 - 120 bases, one tile each, only there to raise the call's couple count
above few_limit and far enough for the band target to drop to 16 or below.

The corridor (probe launch, skipped tiles) under whole-tile waits: three couples of 9 - 10 kb pairs as in test_gpu_tile_list.py."""
import random
import re

import pytest

from isonclust2_amd import _lib, api
from tests.test_gpu_align import _host, _mutate
from tests.test_gpu_tile_list import _random, _related

pytestmark = pytest.mark.gpu

K = 11
EDGE_D = (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 260, 511, 512, 513)
EDGE_M = (1500, 1536, 1537, 2049, 2500, 3073)
N_FILLERS = 560


class _Batch:
    def __init__(self):
        self.seqs, self.pairs = [], []

    def add(self, q, r, rc, e):
        if rc:   # (the pair stays related: the aligner takes the reference's reverse complement)
            r = bytes({65: 84, 67: 71, 71: 67, 84: 65}[ch] for ch in reversed(r))
        self.seqs.extend([q, r])
        self.pairs.append((len(self.seqs) - 2, len(self.seqs) - 1, rc, e))


def _host_answers(b):
    L = _lib.load()
    return [_host(L, b.seqs[q], b.seqs[r], rc, e, K) for q, r, rc, e in b.pairs]


@pytest.fixture(scope="module")
def batches():
    """-> (edge pairs, fillers), each (seqs, pairs, host answers); drawn and answered once"""
    rng = random.Random(20250)
    edge = _Batch()

    def shape(n, m, times):   # the copies of a shape in one gap-open class: neighbours in the aligner's order
        rc, e = rng.randint(0, 1), rng.choice((0.05, 0.12, 0.2))
        for _ in range(times):
            edge.add(*_related(rng, n, m, rng.uniform(0.05, 0.10)), rc, e)

    for i, d in enumerate(EDGE_D):
        shape(1024 + d, EDGE_M[i % len(EDGE_M)], 2)
    for d in EDGE_D:
        shape(1024 + d, 900, 1)
    for n, m in ((3073, 3073), (2560, 1025), (300, 2500)):
        shape(n, m, 2)
    edge.add(_random(rng, 2049), _random(rng, 2049), 0, 0.12)
    edge.add(_random(rng, 2049), _random(rng, 2049), 1, 0.12)
    fill = _Batch()
    for t in range(N_FILLERS):
        n = rng.randint(40, 120)
        fill.add(*_related(rng, n, rng.randint(40, 120), rng.uniform(0.05, 0.10)), t % 2, (0.05, 0.12, 0.2)[t % 3])
    return (edge.seqs, edge.pairs, _host_answers(edge)), (fill.seqs, fill.pairs, _host_answers(fill))


@pytest.fixture(scope="module")
def long_pairs():
    """two couples of same-transcript pairs of 9 - 10 kb at 2 % error, a third with an unrelated pair of the same size beside a related one"""
    rng = random.Random(71)
    b = _Batch()
    for n, m in ((9900, 9800), (9850, 9750), (9500, 9450), (9480, 9400), (9100, 9050)):
        b.add(*_related(rng, n, m), 0, 0.05)
    b.add(_random(rng, 9090), _random(rng, 9040), 0, 0.05)
    return b.seqs, b.pairs, _host_answers(b)


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _join(*parts):
    seqs, pairs, want = [], [], []
    for s, p, w in parts:
        pairs += [(q + len(seqs), r + len(seqs), rc, e) for q, r, rc, e in p]
        seqs += s
        want += w
    return seqs, pairs, want


_CALL = re.compile(r"aligner v2: shape: (\d+) couples, band target (\d+), few_limit (\d+), occ (\d+), n_cu (\d+)")
_SLICE = re.compile(r"aligner v2: shape: slice (\d+): (\d+) couples, waits for (rows|tiles), per_cu (\d+), n_wg (\d+), kernel (k_fwd2(?:_w2)?), n_probe (\d+)")


def _shapes(err):
    """the calls of align_v2_run in one ioc_align_pairs, each with its slices, from the IOC_TRACE lines"""
    calls = []
    for line in err.splitlines():
        m = _CALL.search(line)
        if m:
            calls.append(dict(zip(("couples", "target", "few_limit", "occ", "n_cu"), map(int, m.groups())), slices=[]))
            continue
        m = _SLICE.search(line)
        if m:
            assert calls, "a slice's line before its call's"
            si, nc, wait, per_cu, n_wg, kernel, n_probe = m.groups()
            assert int(si) == len(calls[-1]["slices"]), line
            calls[-1]["slices"].append(dict(couples=int(nc), wait=wait, per_cu=int(per_cu), n_wg=int(n_wg), kernel=kernel, n_probe=int(n_probe)))
    return calls


def _run(ctx, batch, monkeypatch, capfd, env):
    """one ioc_align_pairs under `env` and IOC_TRACE; every pair against the host; -> (calls as _shapes gives them, stderr)"""
    seqs, pairs, want = batch
    for name in ("IOC_ALIGN_V2_FEW", "IOC_ALIGN_V2_NO_W2", "IOC_ALIGN_CK_BUDGET_MB", "IOC_ALIGN_WAVES", "IOC_ALIGN_CORRIDOR"):
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    # The checkpoint arena keeps what the last call wrote, and the runs of this file lay the same couples out in the same places: a
    # tile that did not wait for its neighbour would find the right values there, left by the run before.  So first the same pairs
    # over every sequence read backwards, in the same shape: the same layout, other values in every checkpoint.
    ctx.align_set_pool([s[::-1] for s in seqs])
    ctx.align_pairs(pairs, K)
    monkeypatch.setenv("IOC_TRACE", "1")
    ctx.align_set_pool(seqs)
    refused = ctx.timings()["n_align_refused"]
    capfd.readouterr()
    score, win, ratio = ctx.align_pairs(pairs, K)
    err = capfd.readouterr().err
    tm = ctx.timings()
    calls = _shapes(err)
    print("shape:", env, calls)
    assert tm["align_version"] == 2 and tm["n_align_refused"] == refused, (tm["align_version"], tm["n_align_refused"] - refused)
    bad = []
    for i, (q, r, rc, e) in enumerate(pairs):
        hs, hr = want[i]
        if score[i] != hs or ratio[i] != hr or win[i] != round(hr * len(seqs[q])):
            bad.append((i, len(seqs[q]), len(seqs[r]), rc, e, int(score[i]), hs, float(ratio[i]), hr, int(win[i])))
    assert not bad, f"{len(bad)} of {len(pairs)} pairs differ from the host aligner under {env}: (pair, n, m, rc, e, score, host's, ratio, host's, windows) {bad[:5]}"
    assert calls and all(c["slices"] for c in calls), err[-2000:]
    assert all(sum(s["couples"] for s in c["slices"]) == c["couples"] for c in calls), calls
    return calls, err


def _edge_slices(call, n_edge_pairs):
    """the slices that hold edge pairs: they come first in the aligner's order (heaviest first)"""
    out, first = [], 0
    for s in call["slices"]:
        if 2 * first < n_edge_pairs:
            out.append(s)
        first += s["couples"]
    return out


def _assert_shape(call, n_edge_pairs, wait, kernel):
    sl = _edge_slices(call, n_edge_pairs)
    assert sl and all(s["wait"] == wait and s["kernel"] == kernel for s in sl), (wait, kernel, call)
    for s in call["slices"]:   # what the lines say of one another
        assert (s["wait"] == "rows") == (call["few_limit"] > 0 and s["couples"] <= call["few_limit"]), call
        assert 1 <= s["per_cu"] <= call["occ"] and 1 <= s["n_wg"] <= s["per_cu"] * call["n_cu"], call


def test_a_few_couples_rows_three_waves(ctx, batches, monkeypatch, capfd):
    edge, _ = batches
    (call,), _ = _run(ctx, edge, monkeypatch, capfd, {})
    assert call["few_limit"] == 128 and call["couples"] == (len(edge[1]) + 1) // 2 <= 128
    assert call["target"] == 17, call
    _assert_shape(call, len(edge[1]), "rows", "k_fwd2")


def test_b_many_couples_tiles_two_waves_the_benchmarks_shape(ctx, batches, monkeypatch, capfd):
    edge, fill = batches
    (call,), _ = _run(ctx, _join(edge, fill), monkeypatch, capfd, {})
    assert call["few_limit"] == 128 and call["couples"] > 128
    assert call["target"] <= 16, f"{call}: this chip needs more fillers for bands of two coarse rows"
    _assert_shape(call, len(edge[1]), "tiles", "k_fwd2_w2")


def test_c_many_couples_tiles_three_waves(ctx, batches, monkeypatch, capfd):
    edge, fill = batches
    (call,), _ = _run(ctx, _join(edge, fill), monkeypatch, capfd, {"IOC_ALIGN_V2_NO_W2": "1"})
    assert call["target"] <= 16, call
    _assert_shape(call, len(edge[1]), "tiles", "k_fwd2")
    assert all(s["kernel"] == "k_fwd2" for s in call["slices"]), call


def test_d_few_couples_tiles_bands_of_one_coarse_row(ctx, batches, monkeypatch, capfd):
    edge, _ = batches
    (call,), _ = _run(ctx, edge, monkeypatch, capfd, {"IOC_ALIGN_V2_FEW": "0"})
    assert call["few_limit"] == 0 and call["target"] > 17, call
    _assert_shape(call, len(edge[1]), "tiles", "k_fwd2_w2")


def test_e_many_couples_rows_bands_of_two_coarse_rows(ctx, batches, monkeypatch, capfd):
    edge, fill = batches
    (call,), _ = _run(ctx, _join(edge, fill), monkeypatch, capfd, {"IOC_ALIGN_V2_FEW": "100000"})
    assert call["few_limit"] == 100000 and call["couples"] > 128 and call["target"] <= 16, call
    _assert_shape(call, len(edge[1]), "rows", "k_fwd2")


def test_f_slices_of_both_wait_modes_in_one_call(ctx, batches, monkeypatch, capfd):
    """few_couples is decided per slice, the band target from the call's total.  (A filler couple takes 10 KB of the budget — its
    query profiles —, an edge couple ~170 KB: 2 MB cut the edge couples into slices of a dozen and the fillers into slices of ~200.)"""
    edge, fill = batches
    (call,), _ = _run(ctx, _join(edge, fill), monkeypatch, capfd, {"IOC_ALIGN_CK_BUDGET_MB": "2"})
    assert len(call["slices"]) > 1 and ctx.timings()["align_slices"] == len(call["slices"]), call
    assert call["few_limit"] == 128 and call["target"] <= 16, call
    waits = {s["wait"] for s in call["slices"]}
    assert waits == {"rows", "tiles"}, call
    for s in call["slices"]:
        assert (s["wait"] == "rows") == (s["couples"] <= 128), call
        assert (s["kernel"] == "k_fwd2_w2") == (s["per_cu"] <= 2), call
    assert _edge_slices(call, len(edge[1]))


@pytest.mark.parametrize("no_w2", [False, True])
def test_corridor_under_whole_tile_waits(ctx, long_pairs, monkeypatch, capfd, no_w2):
    env = {"IOC_ALIGN_V2_FEW": "0"}
    if no_w2:
        env["IOC_ALIGN_V2_NO_W2"] = "1"
    calls, err = _run(ctx, long_pairs, monkeypatch, capfd, env)
    call = calls[0]   # (a pair whose corridor could not be certified runs again without one: a second call, behind this one)
    skipped = [int(x) for x in re.findall(r"corridor: (\d+) of \d+ tiles skipped", err)]
    assert skipped and skipped[0] > 0, "no corridor was planned"
    assert call["few_limit"] == 0 and call["couples"] == 3
    assert all(s["wait"] == "tiles" and s["kernel"] == ("k_fwd2" if no_w2 else "k_fwd2_w2") for c in calls for s in c["slices"]), calls
    assert sum(s["n_probe"] for s in call["slices"]) > 0, call


def test_no_shape_lines_without_the_trace_switch(ctx, batches, monkeypatch, capfd):
    _, (seqs, pairs, want) = batches
    monkeypatch.delenv("IOC_TRACE", raising=False)
    ctx.align_set_pool(seqs)
    capfd.readouterr()
    score, _, _ = ctx.align_pairs(pairs[:40], K)
    assert "[ioc]" not in capfd.readouterr().err
    assert [int(s) for s in score] == [w[0] for w in want[:40]]
