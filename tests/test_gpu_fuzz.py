"""Bounded slices of the randomised differential battery (tools/fuzz_*.py) inside the driver-run `-m gpu` suite
(VERDICT r3 "what's missing" 4: the one real parity bug of round 3 — a Size-1 key reordering two tied clusters,
src/cluster.cpp:622-636 — was found by a fuzz seed the driver never ran).

Every slice = FIXED cases first (every case that ever failed, and tie-heavy shapes), then cases drawn from a seed that ROTATES
with the build: the sha of the library's sources (the .git directory does not travel to the GPU box), so that every code
change is met by cases no earlier build saw.  A slice stops drawing new cases when its share of the time is spent
(IOC_FUZZ_SECONDS, default 12 s per slice; the fixed cases always run).  A failure prints the reproducer: the case's full
parameter dict, `python tools/fuzz_parity.py --case '<dict>'` (or fuzz_consensus.py) replays it."""
import glob
import hashlib
import os
import random
import time

import numpy as np
import pytest

from isonclust2_amd import api
from tests import fuzz_cases as fz

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = float(os.environ.get("IOC_FUZZ_SECONDS", "12"))


def _build_seed():
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "isonclust2_amd", "csrc", "*.*")) + glob.glob(os.path.join(ROOT, "include", "*.h"))):
        if f.endswith((".hip", ".cpp", ".h", ".inc")):
            h.update(open(f, "rb").read())
    return int.from_bytes(h.digest()[:4], "little")


SEED = _build_seed()


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _slice(run, fixed, draw, min_random=4):
    """fixed cases, then random ones until the budget is spent (at least min_random); returns the failures."""
    bad, t0, n = [], time.time(), 0
    for c in fixed:
        ok, why = run(c)
        if not ok:
            bad.append((c, why))
    while n < min_random or time.time() - t0 < BUDGET:
        c = draw()
        ok, why = run(c)
        n += 1
        if not ok:
            bad.append((c, why))
        if n >= 400:
            break
    return bad, n


# tie-heavy fixed shapes: short duplicated transcripts (many clusters tied at the top Size: the libstdc++ order decides)
_PARITY_FIXED = [
    dict(n=200, g=12, ln=200, qlo=11.0, qhi=19.0, dup=2, jit=0.0, k=11, w=15, seed=101, mode="fast"),
    dict(n=259, g=23, ln=120, qlo=9.0, qhi=21.0, dup=3, jit=0.3, k=10, w=14, seed=202, mode="fast"),
    dict(n=150, g=6, ln=350, qlo=7.0, qhi=11.0, dup=2, jit=0.0, k=13, w=20, seed=303, mode="fast"),
    dict(n=1, g=1, ln=120, qlo=14.0, qhi=18.0, dup=0, jit=0.0, k=15, w=22, seed=404, mode="fast"),
    # structured reads (fuzz_cases.parity_reads): a gene family that shares a core — walks of dozens of near-equal candidates —,
    # and a shared tandem repeat — reads that repeat one minimizer value, one posting list hit by every query
    dict(n=160, g=40, ln=600, qlo=10.0, qhi=21.0, dup=0, jit=0.0, k=11, w=15, seed=505, mode="fast", shape="family",
         sargs=dict(core_frac=0.55, truncate=0.0)),
    dict(n=120, g=10, ln=700, qlo=11.0, qhi=19.0, dup=0, jit=0.0, k=11, w=15, seed=606, mode="fast", shape="repeat",
         sargs=dict(period=3, block_frac=0.5, truncate=0.4)),
]


@pytest.mark.parametrize("mode", ["fast", "sahlin", "furious"])
def test_fuzz_parity(ctx, mode):
    rng = np.random.default_rng([SEED, {"fast": 1, "sahlin": 2, "furious": 3}[mode]])
    fixed = [dict(c, mode=mode, n=min(c["n"], 70 if mode != "fast" else c["n"]), ln=min(c["ln"], 350 if mode != "fast" else c["ln"])) for c in _PARITY_FIXED]
    count = [0]

    def run(c):
        count[0] += 1
        return fz.run_parity(ctx, c, merge=(count[0] % 4 == 0))

    bad, n = _slice(run, fixed, lambda: fz.draw_parity(rng, None if mode == "fast" else mode))
    assert not bad, f"{len(bad)} of {n + len(fixed)} cases differ from the oracle; first: python tools/fuzz_parity.py --case \"{bad[0][0]}\"  ({bad[0][1]})"


# off the default point (fuzz_cases.draw_parity_params): a query without a cluster candidate under MinShared 0, MinFraction above 1,
# a non-ascending gap-limit column with a limit above the LDS halo of k_gap_bounds
_PARAMS_FIXED = [
    dict(n=180, g=10, ln=300, qlo=9.0, qhi=20.0, dup=2, jit=0.0, k=11, w=15, seed=601, mode="fast",
         params=dict(min_shared=0, min_fraction=0.5, mapped_threshold=0.65, min_prob_no_hits=1e-4)),
    dict(n=120, g=6, ln=600, qlo=11.0, qhi=19.0, dup=0, jit=0.0, k=13, w=20, seed=602, mode="fast",
         params=dict(min_shared=3, min_fraction=1.25, mapped_threshold=0.3, min_prob_no_hits=0.1)),
    dict(n=40, g=4, ln=2500, qlo=8.0, qhi=11.0, dup=2, jit=0.0, k=21, w=50, seed=603, mode="fast",
         params=dict(min_shared=1, min_fraction=0.8, mapped_threshold=0.99, min_prob_no_hits=0.1)),
]


def test_fuzz_parity_params(ctx):
    rng = np.random.default_rng([SEED, 4])
    count = [0]

    def run(c):
        count[0] += 1
        return fz.run_parity(ctx, c, merge=(count[0] % 4 == 0))

    bad, n = _slice(run, _PARAMS_FIXED, lambda: fz.draw_parity_params(rng))
    assert not bad, f"{len(bad)} of {n + len(_PARAMS_FIXED)} cases differ from the oracle; first: python tools/fuzz_parity.py --case \"{bad[0][0]}\"  ({bad[0][1]})"


_CONS_FIXED = [
    # tools/fuzz_consensus.py seed 34, case 52 (round 3): entry 82 meets two clusters tied at the top Size, both pass, and the
    # reference's hit order between them hangs on a Size-1 key of a THIRD cluster whose representative changed one entry earlier
    dict(n=162, g=5, ln=1200, cmax=12, cmin=2, period=25, seed=163853082, dup=0, mode="fast", qlo=11, qhi=22),
    # tie-heavy: duplicated transcripts, short reads, consensus at every second member
    dict(n=200, g=8, ln=300, cmax=3, cmin=2, period=500, seed=77, dup=2, mode="fast", qlo=11, qhi=22),
    dict(n=219, g=11, ln=500, cmax=6, cmin=2, period=5, seed=78, dup=2, mode="fast", qlo=11, qhi=22),
]


@pytest.mark.parametrize("mode,speculate", [("fast", None), ("fast", False), ("sahlin", None)])
def test_fuzz_consensus(ctx, mode, speculate):
    rng = np.random.default_rng([SEED, 10 + (0 if mode == "fast" else 1) + (2 if speculate is False else 0)])
    fixed = [dict(c, mode=mode, n=min(c["n"], 120 if mode != "fast" else c["n"]), ln=min(c["ln"], 800 if mode != "fast" else c["ln"])) for c in _CONS_FIXED]
    bad, n = _slice(lambda c: fz.run_consensus(ctx, c, speculate=speculate), fixed, lambda: fz.draw_consensus(rng, mode))
    env = "IOC_CONS_SPECULATE=0 " if speculate is False else ""
    assert not bad, f"{len(bad)} of {n + len(fixed)} cases differ from the oracle; first: {env}python tools/fuzz_consensus.py --case \"{bad[0][0]}\"  ({bad[0][1]})"


def _fuzz_real_graphs(ctx, poa_type):
    rng = np.random.default_rng([SEED, 20] if poa_type == 0 else [SEED, 20, poa_type])
    more = {"poa_type": poa_type} if poa_type else {}        # (type 0: the cases and the draws as before the types existed)

    def draw():
        c = fz.draw_consensus(rng, "fast")
        c.update(n=min(c["n"], 150), ln=min(c["ln"], 500), **more)
        return c

    fixed = [dict(c, n=min(c["n"], 150), ln=min(c["ln"], 500), **more) for c in _CONS_FIXED[1:]]
    bad, n = _slice(lambda c: fz.run_consensus_poa(ctx, c), fixed, draw, min_random=3)
    assert not bad, (f"{len(bad)} of {n + len(fixed)} cases differ from the oracle; first: python tools/fuzz_poa.py --case \"{bad[0][0]}\""
                     f"  ({bad[0][1]})")


def test_fuzz_consensus_with_real_graphs(ctx):
    """the POA engine behind the product, the oracle's scalar POA behind the oracle (spoa itself: unpinned)"""
    _fuzz_real_graphs(ctx, 0)


@pytest.mark.parametrize("poa_type", [1, 2])
def test_fuzz_consensus_with_real_graphs_off_local(ctx, poa_type):
    """the same under global and semi-global alignment (`cluster -A 1 | 2`) on both sides"""
    _fuzz_real_graphs(ctx, poa_type)


def test_fuzz_align(ctx):
    bad, t0, n = [], time.time(), 0
    for s in [31, SEED & 0xFFFF] + [((SEED >> 8) + i) & 0xFFFFFF for i in range(200)]:
        ok, why = fz.align_batch(ctx, random.Random(s))
        n += 1
        if not ok:
            bad.append((s, why))
        if n >= 3 and time.time() - t0 > BUDGET:
            break
    assert not bad, f"{len(bad)} of {n} batches differ from the host aligner; first: python tools/fuzz_align.py --seed {bad[0][0]}  ({bad[0][1]})"


def test_fuzz_verdict(ctx):
    bad, t0, n = [], time.time(), 0
    for s in [32, SEED & 0xFFFF] + [((SEED >> 12) + i) & 0xFFFFFF for i in range(200)]:
        ok, why = fz.verdict_batch(ctx, random.Random(s))
        n += 1
        if not ok:
            bad.append((s, why))
        if n >= 2 and time.time() - t0 > BUDGET:
            break
    assert not bad, f"{len(bad)} of {n} batches: verdict mode differs from the exact mode; first: python tools/fuzz_verdict.py --seed {bad[0][0]}  ({bad[0][1]})"


def test_fuzz_corridor(ctx):
    """long pairs: the aligner's corridor (probe launch, certificate, second pass) against every tile, and the host aligner"""
    bad, t0, n = [], time.time(), 0
    for s in [33, 34, SEED & 0xFFFF] + [((SEED >> 4) + i) & 0xFFFFFF for i in range(200)]:
        ok, why = fz.corridor_batch(ctx, random.Random(s))
        n += 1
        if not ok:
            bad.append((s, why))
        if n >= 3 and time.time() - t0 > BUDGET:
            break
    assert not bad, f"{len(bad)} of {n} batches: the corridor's results differ; first: python tools/fuzz_corridor.py --seed {bad[0][0]}  ({bad[0][1]})"
