"""The certificate of a tapered corridor, on the host (ioc_host_align_corridor: the statement of what version 2 of the GPU aligner
computes under a corridor).  The aligner restricted to a corridor of tiles returns a score, an end cell, an operation
string and three bounds; whenever the score strictly beats min(parent bound, max(start bound, exit bound)) all three must be the
full-matrix host aligner's (ioc_host_align_ops), byte for byte.

Cases: tile edges 16 and 32, lengths 120 - 400; related pairs at 2 - 15 % error, a long insertion or deletion, a shifted fragment,
unrelated pairs; corridors that taper down the grid as plan_corridor's do (a top width, a slope, a margin, all drawn) and irregular
ones (the same, every band's ends jittered and shifted, made monotone again — they may leave out the diagonal).  The widths are
drawn for 2 / -2 / 3 / 1 and scaled for another score set by what an error costs there in matches (_loss: the same error rates
take a wider corridor where a gap costs four matches than where it costs two, as plan_corridor's own widths do).  At least a quarter
of the cases with skipped tiles must certify: a certificate that refuted everything would pass the first check for nothing.

The corridors here are drawn, and cover shapes the planner never makes.  The planner's own corridors — the bands and plo / phi that
plan_couples (csrc/ioc_align_plan.h) plans for pairs of 5 - 9 kb, tapered and of one width — go through the same certificate in
tools/align_plan_check.cpp, a stand-alone program for the CPU."""
import ctypes as C
import random

import pytest

from isonclust2_amd import _lib

INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
# (match, mismatch, gap_open, gap_extend): the default scores and the tie-rich set of tests/test_gpu_align_params.py
SCORES = [(2, -2, 3, 1), (1, -1, 3, 1)]
N_CASES = 560   # per tile edge and score set: 2240 in all


def _mutate(rng, s, e):
    out = bytearray()
    for ch in s:
        x = rng.random()
        if x < e / 3:
            out.append(rng.choice(b"ACGT"))
        elif x < 2 * e / 3:
            continue
        elif x < e:
            out.append(ch)
            out.append(rng.choice(b"ACGT"))
        else:
            out.append(ch)
    return bytes(out)


def _pair(rng):
    L = rng.randrange(120, 400)
    base = bytes(rng.choice(b"ACGT") for _ in range(L))
    kind = rng.random()
    if kind < 0.6:
        a, b = _mutate(rng, base, rng.uniform(0.02, 0.15)), _mutate(rng, base, rng.uniform(0.0, 0.1))
    elif kind < 0.8:   # a long insertion or deletion
        k = rng.randrange(10, 60)
        p = rng.randrange(0, L - k)
        a, b = base, base[:p] + base[p + k:]
        if rng.random() < 0.5:
            a, b = b, a
    elif kind < 0.9:   # a shifted fragment: the path runs far off the diagonal
        a, b = base, base[rng.randrange(0, L // 2):]
        if rng.random() < 0.5:
            a, b = b, a
    else:
        a, b = base, bytes(rng.choice(b"ACGT") for _ in range(L))
    return a[:400], b[:400], ("related" if kind < 0.6 else "indel" if kind < 0.8 else "shifted" if kind < 0.9 else "unrelated")


def _loss(scores):
    """what an error costs, in matches: the corridor model's (CorridorModel::pair_width) — a third each of substitutions,
    insertions and deletions"""
    match, mismatch, go, _ = scores
    return ((match - mismatch) / 3 + 2 / 3 * (go + match)) / match


def _corridor(rng, n, m, T, scale):
    nb, ns = (n + T - 1) // T, (m + T - 1) // T
    top, g, margin = min(0.9, rng.uniform(0.1, 0.5) * scale) * max(n, m), rng.uniform(0.0, 0.3) * scale, rng.uniform(0, 2 * T)
    irregular = rng.random() < 0.3
    shift = rng.randint(-1, 1) if irregular else 0
    lo, hi = [], []
    for b in range(nb):
        r0, r1 = b * T, min(n, (b + 1) * T)
        d = max(top - r0, g * (n - r0), margin)
        l, h = max(0, int(r0 - d)) // T, int(r1 + d) // T
        if irregular:
            l, h = l + shift + rng.randint(-1, 1), h + shift + rng.randint(-1, 1)
        h = max(0, min(ns - 1, h))
        lo.append(max(0, min(l, h)))
        hi.append(h)
    for b in range(1, nb):   # monotone down the bands
        hi[b] = max(hi[b], hi[b - 1])
        lo[b] = min(max(lo[b], lo[b - 1]), hi[b])
    return lo, hi, irregular


def _restricted(L, q, r, sc, T, lo, hi):
    nb = len(lo)
    i32 = C.c_int32 * nb
    out = (C.c_int32 * 8)()
    ops = C.create_string_buffer(len(q) + len(r) + 1)
    n = L.ioc_host_align_corridor(q, len(q), r, len(r), sc[0], sc[1], sc[2], sc[3], i32(*([T] * nb)), nb, T, i32(*lo), i32(*hi), ops, len(q) + len(r) + 1, out)
    assert n >= 0, n
    return ops.raw[:n], list(out)


def _full(L, q, r, sc):
    ops, s = C.create_string_buffer(len(q) + len(r) + 1), C.c_int32()
    n = L.ioc_host_align_ops(q, len(q), r, len(r), sc[0], sc[1], sc[2], sc[3], ops, len(q) + len(r) + 1, C.byref(s))
    assert n >= 0, n
    o = ops.raw[:n]
    td = len(o) - len(o.rstrip(b"d"))
    ti = len(o) - td - len(o[:len(o) - td].rstrip(b"i"))
    return o, s.value, len(q) - ti, len(r) - td


@pytest.mark.parametrize("scores", SCORES, ids=lambda s: "%d_%d_%d_%d" % s)
@pytest.mark.parametrize("T", [16, 32])
def test_certified_results_are_the_full_matrix(T, scores):
    L = _lib.load()
    rng = random.Random(9000 + T * 10 + scores[0])
    scale = _loss(scores) / _loss(SCORES[0])
    with_skipped = certified = by_parent_alone = irregular_certified = 0
    kinds = {}
    for case in range(N_CASES):
        q, r, kind = _pair(rng)
        lo, hi, irregular = _corridor(rng, len(q), len(r), T, scale)
        ops, out = _restricted(L, q, r, scores, T, lo, hi)
        score, ei, ej, parent, start, exit_, skipped, tiles = out
        fops, fscore, fi, fj = _full(L, q, r, scores)
        assert score <= fscore, (case, kind, score, fscore)
        if skipped == 0:
            assert (ops, score, ei, ej) == (fops, fscore, fi, fj), (case, kind, "nothing skipped")
            assert parent == start == exit_ == INT32_MIN, (case, out)
            continue
        with_skipped += 1
        cert = min(parent, max(start, exit_))
        k = kinds.setdefault(kind, [0, 0])
        k[0] += 1
        if score > cert:
            certified += 1
            k[1] += 1
            irregular_certified += irregular
            by_parent_alone += not score > max(start, exit_)
            assert (score, ei, ej) == (fscore, fi, fj) and ops == fops, (case, kind, T, lo, hi, out, fscore, fi, fj)
    print(f"tile {T}, scores {scores}: {with_skipped} cases with skipped tiles, {certified} certified ({by_parent_alone} by the parent bound alone, "
          f"{irregular_certified} in irregular corridors); per kind [cases, certified]: {kinds}")
    assert with_skipped >= N_CASES // 2, with_skipped
    assert 4 * certified >= with_skipped, (certified, with_skipped)


def test_a_corridor_that_skips_nothing_and_bad_arguments():
    L = _lib.load()
    q, r = b"ACGTACGTAC" * 5, b"ACGTTCGTAC" * 5
    ops, out = _restricted(L, q, r, SCORES[0], 16, [0, 0, 0, 0], [9, 9, 9, 9])   # (phi is cut to the pair's last strip)
    fops, fscore, fi, fj = _full(L, q, r, SCORES[0])
    assert (ops, out[0], out[1], out[2]) == (fops, fscore, fi, fj) and out[3:8] == [INT32_MIN] * 3 + [0, 16]
    i32 = C.c_int32 * 2
    o8 = (C.c_int32 * 8)()
    # heights that do not reach the last row; a band with plo above phi
    assert L.ioc_host_align_corridor(q, 50, r, 50, 2, -2, 3, 1, i32(16, 16), 2, 16, i32(0, 0), i32(3, 3), None, 0, o8) < 0
    assert L.ioc_host_align_corridor(q, 32, r, 50, 2, -2, 3, 1, i32(16, 16), 2, 16, i32(0, 2), i32(3, 1), None, 0, o8) < 0


def test_a_skipped_diagonal_has_no_parent_bound():
    """two identical sequences, the tiles on the lower half of the diagonal left out: the restricted score is lower, nothing certifies it"""
    L = _lib.load()
    rng = random.Random(5)
    q = bytes(rng.choice(b"ACGT") for _ in range(64))
    ops, out = _restricted(L, q, q, SCORES[0], 16, [0, 0, 3, 3], [1, 1, 3, 3])
    assert out[0] < 128 and out[3] == INT32_MAX and not out[0] > min(out[3], max(out[4], out[5])), out
