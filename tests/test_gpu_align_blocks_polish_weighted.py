"""ioc_align_pairs_blocks_polish_weighted: ioc_align_pairs_blocks_polish with the seven weight planes projected beside the eight
(k_ops_project_weights), and k_group_pile_weighted and the weighted call kernels behind the block kernels.  Everything but the
isoforms' sequences, qualities and records must equal ioc_align_pairs_blocks_polish on the same pairs, as bytes; the isoforms'
calls must equal the host pipeline's, as bytes — the host aligner, the three host projections, api.planes_blocks and the weighted
definition (iso_polish_weight_common.host_groups_polish_weighted).  On the property case of test_iso_polish_host.py under random
quality lines plus correct_common.isoform_case as a second segment, the pairs interleaved."""
import ctypes as C

import numpy as np
import pytest

from isonclust2_amd import api
from tests import blocks_common as bc
from tests import correct_common as cc
from tests import iso_polish_common as ic
from tests import iso_polish_weight_common as iw
from tests import polish_weight_common as pw

pytestmark = pytest.mark.gpu

BLOCK_KEYS = ("score", "windows", "ratio", "block_off", "reads", "seg", "stats", "cols", "row0", "gseg_off")


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


@pytest.fixture(scope="module")
def case():
    """the two segments with their pairs interleaved, a random quality line per sequence of the pool, and the host pipeline: the
    four planes of every pair once, and the blocks of every segment"""
    T, reads, true = bc.property_case(ic.SEED)
    T2, reads2, _ = cc.isoform_case(cc.SEED)
    frames, groups = [T, T2], [reads, reads2]
    seqs, pairs = list(frames), []
    for g, rds in enumerate(groups):
        for rd in rds:
            pairs.append((len(seqs), g, 0, 0.1))
            seqs.append(rd)
    order = sorted(range(len(pairs)), key=lambda x: (sum(1 for y in range(x) if pairs[y][1] == pairs[x][1]), pairs[x][1]))
    pairs = [pairs[x] for x in order]
    sop = [p[1] for p in pairs]
    mine = [[x for x, s in enumerate(sop) if s == g] for g in range(2)]
    quals = pw.random_quals(np.random.default_rng(ic.SEED), seqs, 33, 75)
    planes = [iw.host_planes(frames[sop[x]], [seqs[pairs[x][0]]], [quals[pairs[x][0]]]) for x in range(len(pairs))]
    base, slots, wbase, wslots = ([p[k][0] for p in planes] for k in range(4))
    blocks = [api.planes_blocks(np.array([base[x] for x in mine[g]], np.uint8), **bc.DEFAULT) for g in range(2)]
    return dict(frames=frames, seqs=seqs, quals=quals, pairs=pairs, sop=sop, segs=[(0, 0), (1, 0)], mine=mine, base=base, slots=slots, wbase=wbase, wslots=wslots,
                blocks=blocks)


def _host(case, max_iso, min_depth):
    """the weighted definition on the host pipeline's planes and isoforms"""
    group = [-1] * len(case["pairs"])
    for g in range(2):
        for x, h in zip(case["mine"][g], case["blocks"][g]["reads"]["group"].tolist()):
            group[x] = h
    ng = [min(int(case["blocks"][g]["seg"]["n_groups"]), max_iso) for g in range(2)]
    return iw.host_groups_polish_weighted(case["frames"], case["sop"], group, ng, case["base"], case["slots"], case["wbase"], case["wslots"], min_depth), ng


def _same_but_the_calls(got, plain):
    for f in BLOCK_KEYS:
        assert np.asarray(got[f]).tobytes() == np.asarray(plain[f]).tobytes(), f
    for f in ("blocks", "rows"):
        assert len(got[f]) == len(plain[f]) and all(a.tobytes() == b.tobytes() for a, b in zip(got[f], plain[f])), f
    assert [len(s) for s in got["gseq"]] == [len(s) for s in plain["gseq"]]


def test_against_the_unweighted_call_and_the_host_pipeline(ctx, case):
    ctx.align_set_pool(case["seqs"])
    ctx.align_set_pool_qual(case["quals"])
    plain = ctx.align_pairs_blocks_polish(case["pairs"], 11, case["segs"], case["sop"], tables=True, stats=True)
    got = ctx.align_pairs_blocks_polish_weighted(case["pairs"], 11, case["segs"], case["sop"], tables=True, stats=True)
    _same_but_the_calls(got, plain)
    want, ng = _host(case, 16, 3)
    iw.same_groups_weighted(got, want, tables=False)
    assert ng[0] == 4 and got["gseg_off"].tolist() == [0, ng[0], ng[0] + ng[1]]
    assert got["gqual"] != plain["gqual"]   # (under random qualities the two calls are not the same bytes)
    lean = ctx.align_pairs_blocks_polish_weighted(case["pairs"], 11, case["segs"], case["sop"], rows=False, polish_min_depth=1, max_iso=2)
    assert "cols" not in lean and "rows" not in lean and lean["reads"].tobytes() == got["reads"].tobytes()
    iw.same_groups_weighted(lean, _host(case, 2, 1)[0], tables=False)
    # the unweighted call behind it on the same context is what it was: the weight planes are a weighted call's alone
    again = ctx.align_pairs_blocks_polish(case["pairs"], 11, case["segs"], case["sop"], tables=True, stats=True)
    _same_but_the_calls(again, plain)
    ic.same_groups(again, plain, tables=False)


@pytest.mark.parametrize("byte", [b"I", b"\""])
def test_with_uniform_qualities_the_whole_result_is_the_unweighted_call(ctx, case, byte):
    ctx.align_set_pool(case["seqs"])
    ctx.align_set_pool_qual([byte * len(s) for s in case["seqs"]])
    plain = ctx.align_pairs_blocks_polish(case["pairs"], 11, case["segs"], case["sop"], tables=True, stats=True)
    got = ctx.align_pairs_blocks_polish_weighted(case["pairs"], 11, case["segs"], case["sop"], tables=True, stats=True)
    _same_but_the_calls(got, plain)
    ic.same_groups(got, plain, tables=False)
    assert sum(len(s) for s in got["gseq"]) >= 5


def test_a_pool_without_qualities_is_refused_with_nothing_written(ctx, case):
    ctx.align_set_pool(case["seqs"])          # (every align_set_pool drops the qualities)
    with pytest.raises(api.IocError) as e:
        ctx.align_pairs_blocks_polish_weighted(case["pairs"], 11, case["segs"], case["sop"])
    assert e.value.code == -1
    ctx.align_set_pool([b"ACGTACGTAC", b"ACGTTCGTAC", b"ACGTTCGTACG"])
    pairs, segs, sop = [(1, 0, 0, 0.1), (2, 0, 0, 0.1)], [(0, 0)], [0, 0]
    arr = ctx._aln_pairs(pairs)
    sarr, sop32, rlen, n_rows = ctx._seg_args(2, segs, sop)
    i32, i64, f64 = (lambda n: np.full(n, -9, np.int32)), (lambda n: np.full(n, -9, np.int64)), (lambda n: np.full(n, -9.0, np.float64))
    score, win, ratio, boff, off, goff = i32(2), i64(2), f64(2), i64(2), i64(3), i64(2)
    blob = lambda n: np.full(n, 0xA5, np.uint8)
    st, tab, blocks, reads, seg, cols = blob(2 * api.ALN_STATS_DTYPE.itemsize), blob(n_rows * api.BLOCK_ROW_DTYPE.itemsize), blob(10 * api.PILE_BLOCK_DTYPE.itemsize), \
        blob(2 * api.READ_BLOCKS_DTYPE.itemsize), blob(api.BLOCKS_SEG_DTYPE.itemsize), blob(n_rows * api.PILEUP_DTYPE.itemsize)
    cap = 2 * api.pileup_call_bound(10)
    seq, qual, pol = blob(cap), blob(cap), blob(2 * api.POLISH_STATS_DTYPE.itemsize)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    args = (ctx.h, 2, arr, 11, 2, -2, 1, p(score, C.c_int32), p(win, C.c_int64), p(ratio, C.c_double), st.ctypes.data, 1, sarr, p(sop32, C.c_int32),
            *[bc.DEFAULT[f] for f in ("min_gap", "min_depth", "min_alt", "min_pct", "min_block", "max_blocks")], tab.ctypes.data, blocks.ctypes.data, 10,
            p(boff, C.c_int64), reads.ctypes.data, seg.ctypes.data, cols.ctypes.data, 16, 3, seq.ctypes.data, qual.ctypes.data, cap, p(off, C.c_int64),
            pol.ctypes.data, 2, p(goff, C.c_int64))
    assert ctx.L.ioc_align_pairs_blocks_polish_weighted(*args) == -1
    assert all((a == -9).all() for a in (score, win, ratio, boff, off, goff))
    assert all((a == 0xA5).all() for a in (st, tab, blocks, reads, seg, cols, seq, qual, pol))
    assert ctx.L.ioc_align_pairs_blocks_polish(*args) == 0 and off[0] == 0 and (score != -9).all()   # (the call itself was a good one)
    ctx.align_set_pool_qual([b"IIIIIIIIII", b"5555555555", b"55555555555"])
    assert ctx.L.ioc_align_pairs_blocks_polish_weighted(*args) == 0
