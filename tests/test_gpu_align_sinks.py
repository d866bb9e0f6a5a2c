"""The five sinks of the batched GPU aligner's operation bytes, one after the other on ONE context and ONE pool: ioc_align_pairs_ops,
_stats, _pileup, _polish and _polish_weighted share the device buffers their tables live in (a_pile, a_pile_ins, a_pile_w) and the
code that reserves and zeroes them, so a call must not see what a call of another kind, or a call over more rows, left there.
Each kind's own test file uses one kind; this one runs them in order, in reverse, and a call over fewer rows behind one over more.
Bytes and integers only, no tolerance."""
import random

import numpy as np
import pytest

from isonclust2_amd import api
from tests import polish_weight_common as pw
from tests.test_gpu_align import _mutate
from tests.test_gpu_align_pileup import _sum_of
from tests.test_gpu_align_polish import _segments
from tests.test_gpu_align_stats import _rec

pytestmark = pytest.mark.gpu

K = 11
EMPTY = 8


def _pool():
    """Two references of different lengths (300, 150), three reads of each (one a 40-base piece), and an empty sequence; ten pairs
    on them, one with an empty query and one with an empty reference."""
    rng = random.Random(77)
    a = bytes(rng.choice(b"ACGT") for _ in range(300))
    b = bytes(rng.choice(b"ACGT") for _ in range(150))
    seqs = [a, b, _mutate(rng, a, 0.08), _mutate(rng, a, 0.12), _mutate(rng, a[100:150], 0.05)[:40], _mutate(rng, b, 0.08), _mutate(rng, b, 0.12),
            _mutate(rng, b[20:110], 0.1), b""]
    assert all(40 <= len(s) <= 330 for s in seqs[:EMPTY])
    pairs = [(2, 0, 0, 0.1), (5, 1, 0, 0.1), (3, 0, 0, 0.15), (EMPTY, 0, 0, 0.1), (6, 1, 0, 0.15), (4, 0, 0, 0.05), (7, 1, 0, 0.1), (5, EMPTY, 0, 0.1),
             (3, 1, 0, 0.3), (1, 0, 0, 0.3)]
    return seqs, pairs


def _round(ctx, pairs, segs, sop, n_rows, row_base, order):
    """The five calls in `order`: {kind: result}."""
    calls = {"ops": lambda: ctx.align_pairs_ops(pairs, K),
             "stats": lambda: ctx.align_pairs_stats(pairs, K),
             "pileup": lambda: ctx.align_pairs_pileup(pairs, K, row_base, n_rows, stats=True),
             "polish": lambda: ctx.align_pairs_polish(pairs, K, segs, sop, 3, stats=True, tables=True),
             "weighted": lambda: ctx.align_pairs_polish_weighted(pairs, K, segs, sop, 3, stats=True, tables=True)}
    return {kind: calls[kind]() for kind in order}


def _same_round(a, b):
    for kind in ("ops", "stats", "pileup"):
        assert len(a[kind]) == len(b[kind])
        for x, y in zip(a[kind], b[kind]):
            assert x == y if isinstance(x, list) else np.array_equal(x, y), kind
    for kind in ("polish", "weighted"):
        assert a[kind].keys() == b[kind].keys()
        for key, x in a[kind].items():
            assert x == b[kind][key] if isinstance(x, list) else np.array_equal(x, b[kind][key]), (kind, key)


def _layout(seqs, segs, sop):
    row0 = np.concatenate([[0], np.cumsum([len(seqs[ref]) + 1 for ref, _ in segs])])
    return int(row0[-1]), [int(row0[g]) for g in sop]


def test_one_context_every_kind_in_turn():
    seqs, pairs = _pool()
    ctx = api.Context(0)
    ctx.align_set_pool(seqs)
    ctx.align_set_pool_qual(pw.random_quals(np.random.default_rng(5), seqs))
    plain = ctx.align_pairs(pairs, K)  # (no verdict threshold is set on this context)
    order = ("ops", "stats", "pileup", "polish", "weighted")
    segs, sop = _segments(pairs)
    assert len(segs) == 3 and len({len(seqs[ref]) for ref, _ in segs}) == 3  # (300, 150 and the empty reference's one row)
    n_rows, row_base = _layout(seqs, segs, sop)

    first = _round(ctx, pairs, segs, sop, n_rows, row_base, order)
    strings = first["ops"][3]
    # score, windows and ratio: the same from every kind, and a plain ioc_align_pairs'
    for kind in order:
        got = first[kind]
        got = (got["score"], got["windows"], got["ratio"]) if isinstance(got, dict) else got[:3]
        assert all(np.array_equal(g, p) for g, p in zip(got, plain)), kind
    # the records: those of the returned bytes
    for stats in (first["stats"][3], first["pileup"][4], first["polish"]["stats"], first["weighted"]["stats"]):
        assert [_rec(stats, i) for i in range(len(pairs))] == [api.ops_stats(s) for s in strings]
    # the table of counts: that of the returned bytes
    want = _sum_of(seqs, pairs, strings, row_base, n_rows)
    for cols in (first["pileup"][3], first["polish"]["cols"], first["weighted"]["cols"]):
        assert cols.shape == (n_rows,) and np.array_equal(cols, want)
    assert [int(x) for x in first["polish"]["row0"]] == [int(x) for x in first["weighted"]["row0"]] == sorted(set(row_base))
    # the two pairs with an empty sequence: one free end gap, a record that is all leading, nothing piled
    for i, pr in enumerate(pairs):
        n, m = len(seqs[pr[0]]), len(seqs[pr[1]])
        if n and m:
            continue
        assert strings[i] == (b"i" if n else b"d") * (n + m)
        rec = dict.fromkeys(api.ALN_STATS_FIELDS, 0)
        rec.update({"length": n + m, "lead_i" if n else "lead_d": n + m})
        assert {f: int(first["stats"][3][f][i]) for f in api.ALN_STATS_FIELDS} == rec
    empty_row = row_base[[pr[1] for pr in pairs].index(EMPTY)]
    for tab in (first["pileup"][3], first["polish"]["cols"], first["polish"]["ins"], first["weighted"]["cols"], first["weighted"]["wcols"], first["weighted"]["wins"]):
        assert not tab[empty_row:empty_row + 1].tobytes().strip(b"\0")

    # the same calls in reverse
    _same_round(_round(ctx, pairs, segs, sop, n_rows, row_base, order[::-1]), first)

    # over more rows — a segment without pairs in front, and for the pileup 50 unused rows more behind the last — the tables are the
    # first round's behind rows of zeros ...
    big_segs, big_sop = [(2, 0)] + segs, [g + 1 for g in sop]
    shift = len(seqs[2]) + 1
    big_rows, big_base = _layout(seqs, big_segs, big_sop)
    assert big_rows == n_rows + shift and big_base == [rb + shift for rb in row_base]
    big = _round(ctx, pairs, big_segs, big_sop, big_rows + 50, big_base, order)
    for got, small, tail in ((big["pileup"][3], first["pileup"][3], 50), (big["polish"]["cols"], first["polish"]["cols"], 0),
                             (big["polish"]["ins"], first["polish"]["ins"], 0), (big["weighted"]["cols"], first["weighted"]["cols"], 0),
                             (big["weighted"]["wcols"], first["weighted"]["wcols"], 0), (big["weighted"]["wins"], first["weighted"]["wins"], 0)):
        assert got.shape == (big_rows + tail,) and np.array_equal(got[shift:big_rows], small)
        assert not got[:shift].tobytes().strip(b"\0") and not got[big_rows:].tobytes().strip(b"\0")
    for kind in ("polish", "weighted"):
        assert big[kind]["seq"][1:] == first[kind]["seq"] and big[kind]["qual"][1:] == first[kind]["qual"]
        assert big[kind]["seq"][0] == seqs[2] and np.array_equal(big[kind]["stats"], first[kind]["stats"])
    assert np.array_equal(big["pileup"][4], first["pileup"][4]) and big["ops"][3] == strings

    # ... and the calls over fewer rows behind it give what they gave at first
    _same_round(_round(ctx, pairs, segs, sop, n_rows, row_base, order), first)
