"""ioc_planes_correct: k_read_correct over host planes and host tables that are uploaded, against the host definition,
ioc_host_read_correct pair by pair.  One call holds segments of 0, 1, 63, 64, 65, 127, 128, 129 and 600 bases (around the 64 rows
a wave takes per step) with 0, 1, 3, 4, 5 and 130 pairs (around the four waves of a workgroup), the segments' pairs interleaved;
runs of "fill" and of "remove" of 10, 11, 64, 65 and 130 rows that start at rows 0, 62, 63, 64 and 127, end at row rlen - 1 and
span a whole step and both its neighbours (tests/correct_common.py, planted_case); insertions in front of row 0 and of row rlen;
rows of low depth.  Sequences, qualities, offsets and records are compared as bytes."""
import ctypes as C

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import correct_common as cc

pytestmark = pytest.mark.gpu

MAX_RUNS = (0, 10, 64)


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


@pytest.fixture(scope="module")
def case():
    planted = cc.planted_case()
    return planted, {mr: cc.host_correct_planes(*planted, max_run=mr) for mr in MAX_RUNS}


def _same(got, want):
    seqs, quals, recs = got
    assert recs.dtype == api.CORRECT_STATS_DTYPE and recs.tobytes() == want[2].tobytes()
    assert seqs == want[0] and quals == want[1]
    assert [len(s) for s in seqs] == recs["out_len"].tolist()  # (the offsets: a pair's bytes are as many as its record says)


@pytest.mark.parametrize("max_run", MAX_RUNS)
def test_against_the_definition(ctx, case, max_run):
    planted, want = case
    assert sorted(set(np.bincount(planted[3], minlength=len(cc.SHAPES)).tolist())) == [0, 1, 3, 4, 5, 130]
    got = ctx.planes_correct(*planted, max_run=max_run)
    _same(got, want[max_run])
    total = {f: int(got[2][f].sum()) for f in cc.FIELDS}
    print(total)
    # every branch was taken: the guard turned runs back, and below it runs were applied
    assert total["n_sub"] and total["n_ins_add"] and total["n_ins_drop"] and total["n_low"] and total["n_guarded"]
    assert (total["n_fill"] > 0 and total["n_remove"] > 0) == (max_run > 0)
    # ... of either kind, also at max_run 64: what is guarded there is the rows of the runs of 65 and of 130 rows
    if max_run == 64:
        longer = {kind: sum(n for _, _, n in cc.planted_runs(planted, kind) if n > 64) for kind in ("fill", "remove")}
        assert longer["fill"] > 0 and longer["remove"] > 0 and longer["fill"] + longer["remove"] == total["n_guarded"]


def test_the_planted_runs_tell_max_run_from_max_run_plus_1(ctx, case):
    """What the planted runs are for, on the device: runs of exactly 11 and of exactly 64 rows exist of either kind
    (test_read_correct_host.py holds that against the restatement), so between max_run 10 and 11 and between 63 and 64 more rows
    are filled and more are removed."""
    planted, want = case
    for lo, hi in ((10, 11), (63, 64)):
        recs = {}
        for mr in (lo, hi):
            got = ctx.planes_correct(*planted, max_run=mr)
            _same(got, want[mr] if mr in want else cc.host_correct_planes(*planted, max_run=mr))
            recs[mr] = got[2]
        for f in ("n_fill", "n_remove"):
            assert int(recs[lo][f].sum()) < int(recs[hi][f].sum()), (lo, hi, f)


def test_nothing_is_carried_between_calls(ctx, case):
    """A small call behind the large one on the same context, at another rule."""
    planted, _ = case
    frames, cols, ins, sop, base, slots = planted
    ctx.planes_correct(*planted)
    row0 = np.concatenate([[0], np.cumsum([len(f) + 1 for f in frames])]).astype(int)
    keep = [i for i in range(len(sop)) if sop[i] in (3, 7)]
    remap = {7: 0, 3: 1}
    rows = np.r_[row0[7]:row0[8], row0[3]:row0[4]]
    small = ([frames[7], frames[3]], cols[rows], ins[rows], [remap[sop[i]] for i in keep], [base[i] for i in keep], [slots[i] for i in keep])
    rule = dict(min_depth=2, min_alt=2, min_pct=10, max_run=3)
    _same(ctx.planes_correct(*small, **rule), cc.host_correct_planes(*small, **rule))


def test_the_empty_call_and_segments_without_pairs(ctx):
    none = np.zeros(0, api.PILEUP_DTYPE), np.zeros(0, api.PILEUP_INS_DTYPE)
    seqs, quals, recs = ctx.planes_correct([], *none, [], [], [])
    assert seqs == [] and quals == [] and recs.shape == (0,)
    frames = [b"ACGTN", b"", b"GG"]
    seqs, quals, recs = ctx.planes_correct(frames, np.zeros(10, api.PILEUP_DTYPE), np.zeros(10, api.PILEUP_INS_DTYPE), [], [], [])
    assert seqs == [] and quals == [] and recs.shape == (0,)
    # a read that covers nothing, and a read of a segment of no bases
    base, slots = [np.full(6, cc.NONE, np.uint8), np.full(1, cc.NONE, np.uint8)], [np.ones((cc.SLOTS, 6), np.uint8), np.ones((cc.SLOTS, 1), np.uint8)]
    seqs, quals, recs = ctx.planes_correct(frames, np.zeros(10, api.PILEUP_DTYPE), np.zeros(10, api.PILEUP_INS_DTYPE), [0, 1], base, slots)
    assert seqs == [b"", b""] and quals == [b"", b""] and not recs.tobytes().strip(b"\0")


def test_refusals_write_nothing(ctx):
    L = _lib.load()
    frames = [b"ACGT", b"GATTACA"]
    sop = np.array([0, 1, 1], np.int32)
    rlen, f_off = np.array([4, 7], np.int32), np.array([0, 4], np.int64)
    P, R = 5 + 8 + 8, 5 + 8
    base, slots = np.zeros(P, np.uint8), np.zeros(cc.SLOTS * P, np.uint8)
    cols, ins = np.zeros(R, api.PILEUP_DTYPE), np.zeros(R, api.PILEUP_INS_DTYPE)
    cols["a"] = 10
    bound = api.pileup_call_bound(4) + 2 * api.pileup_call_bound(7)
    seq, qual = np.full(bound, 0xA5, np.uint8), np.full(bound, 0xA5, np.uint8)
    off, rec = np.full(4, -9, np.int64), np.full(3 * 8, -9, np.int32)
    p32, p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)), lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    d = lambda a: a.ctypes.data

    def call(ns=2, np_=3, rlen_=rlen, frames_=b"".join(frames), f_off_=f_off, cols_=d(cols), ins_=d(ins), sop_=sop, base_=d(base), slots_=d(slots),
             rule=(3, 3, 25, 10), seq_=d(seq), qual_=d(qual), cap=bound, off_=off):
        s_arr = None if sop_ is None else np.asarray(sop_, np.int32)   # (alive until the call returns)
        return L.ioc_planes_correct(ctx.h, ns, p32(rlen_) if rlen_ is not None else None, frames_, p64(f_off_) if f_off_ is not None else None, cols_, ins_,
                                    np_, p32(s_arr) if s_arr is not None else None, base_, slots_, *rule, seq_, qual_, cap,
                                    p64(off_) if off_ is not None else None, d(rec))

    for rule in ((0, 3, 25, 10), (3, 0, 25, 10), (3, 3, 0, 10), (3, 3, 51, 10), (3, 3, 25, -1), (3, 3, 25, 65)):
        assert call(rule=rule) == -1
    assert call(ns=-1) == -1 and call(np_=-1) == -1 and call(cap=-1) == -1
    assert call(sop_=[0, 2, 1]) == -1 and call(sop_=[-1, 1, 1]) == -1
    assert call(rlen_=np.array([4, -1], np.int32)) == -1 and call(f_off_=np.array([0, -4], np.int64)) == -1
    assert call(rlen_=None) == -1 and call(f_off_=None) == -1 and call(frames_=None) == -1 and call(sop_=None) == -1
    assert call(cols_=None) == -1 and call(ins_=None) == -1
    assert call(base_=None) == -1 and call(slots_=None) == -1 and call(off_=None) == -1 and call(seq_=None) == -1 and call(qual_=None) == -1
    assert call(cap=bound - 1) == -4
    assert (seq == 0xA5).all() and (qual == 0xA5).all() and (off == -9).all() and (rec == -9).all()
    # planes of zeros: A at every row of every pair, kept at 10 of 10
    assert call() == 0 and off.tolist() == [0, 4, 11, 18]
    assert bytes(seq[:18]) == b"A" * 18 and bytes(qual[:18]) == b"I" * 18 and (seq[18:] == 0xA5).all()
    assert rec.reshape(3, 8)[:, 0].tolist() == [4, 7, 7] and not rec.reshape(3, 8)[:, 1:].any()
