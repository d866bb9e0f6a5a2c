"""Plumbing shared by the tests of ioc_left_adopt and of the batches beyond one device pass: oracle-prepared sorted batches
as pipeline.SortedBatch, views padded with gated entries, and the comparisons used more than once."""
import numpy as np

from isonclust2_amd import pipeline
from oracle import pyoracle as po


def with_sequences(rs, view):
    """A copy of an oracle-prepared view with the raw sequences of its entries (sahlin / furious, consensus)."""
    seqs = [rs.read(int(i))[0] for i in view["orig"]]
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    v = dict(view)
    v.update(raw_seq=b"".join(seqs), raw_off=off)
    return v


def sorted_batch(view, start=0):
    v = {k: x for k, x in view.items() if k != "orig"}
    return pipeline.SortedBatch(view=v, read_ids=np.asarray(view["orig"], np.int64), batch_start=start, batch_end=start + len(view["orig"]) - 1)


def gate_mask(view, k=11):
    """The gates of the clustering loop (src/cluster.cpp:116-160) on a view, as the product applies them."""
    with np.errstate(divide="ignore"):
        q = -10 * np.log10(np.asarray(view["raw_err"], np.float64))
    return ((np.asarray(view["state"]) == 1) | (np.asarray(view["score"]) < 0) | (np.asarray(view["raw_len"]) < 2 * k) |
            (np.asarray(view["hpc_len"]) < 2 * k) | (q <= float(view.get("min_qual", 7.0))))


def two_batches(rs, oparams, k=11, w=15):
    """Globally sorted reads cut into two consecutive batches under the oracle's parameters `oparams`:
    ([oracle Batch, oracle Batch], [SortedBatch, SortedBatch])."""
    R = po.ReadSet.from_flat(rs.seq, rs.qual, rs.offs)
    R.score_sort(k, w)
    cuts = [0, rs.n // 2, rs.n]
    obs, sbs = [], []
    for b in range(2):
        B = po.Batch(R, cuts[b], cuts[b + 1] - 1, oparams, batch_nr=b)
        info, off_f, off_r, mn, ps = B.minimizer_soa()
        view = dict(off_fwd=off_f, off_rev=off_r, min_val=mn, min_pos=ps, raw_len=info["raw_len"], hpc_len=info["hpc_len"],
                    score=info["score"], raw_err=info["raw_err"], hpc_err=info["hpc_err"], state=info["state"].astype(np.uint8),
                    min_qual=oparams.min_qual)
        obs.append(B)
        sbs.append(pipeline.SortedBatch(view=view, read_ids=info["orig"].astype(np.int64), batch_nr=b, batch_start=cuts[b],
                                        batch_end=cuts[b + 1] - 1))
    return obs, sbs


def pad_view(view, n_total, real_pos):
    """The entries of `view` at the ascending positions `real_pos` of a view of n_total entries; every other entry is gated:
    state 1, score -1, no minimizers, no sequence (the gates skip such an entry, src/cluster.cpp:116-160)."""
    real_pos = np.asarray(real_pos, np.int64)
    n = len(real_pos)
    assert n == len(view["hpc_len"]) and np.all(np.diff(real_pos) > 0) and real_pos[-1] < n_total
    r = np.searchsorted(real_pos, np.arange(n_total + 1), side="left")      # real entries in front of each position
    out = dict(off_fwd=np.asarray(view["off_fwd"], np.int64)[r], off_rev=np.asarray(view["off_rev"], np.int64)[r],
               min_val=view["min_val"], min_pos=view["min_pos"], min_qual=view.get("min_qual", 7.0))
    fill = dict(raw_len=0, hpc_len=0, score=-1.0, raw_err=0.5, hpc_err=0.5, state=1)
    for key, val in fill.items():
        a = np.full(n_total, val, np.asarray(view[key]).dtype)
        a[real_pos] = view[key]
        out[key] = a
    if view.get("raw_seq") is not None:
        out.update(raw_seq=view["raw_seq"], raw_off=np.asarray(view["raw_off"], np.int64)[r])
    return out


def same_mindb(got, want):
    for g, w_, name in zip(got, want, ("keys", "offs", "postings")):
        assert np.array_equal(g, w_), name


def merge_resident(ctx, p, left_hpc_err, right, **extra_left):
    """The clusters of the ClusteredBatch `right` merged against the left state that is ON the device (n_keys == -1)."""
    counts = np.bincount(right.member_cls, minlength=right.n_clusters).astype(np.int32)
    rv = dict(right.rep_view)
    rv.update(n_members=counts, depth=right.depth, min_cls_size=3)
    if right.rep_seq is not None and extra_left:
        rv.update(raw_seq=right.rep_seq, raw_off=right.rep_off)
    return ctx.cluster_merge(p, dict(resident=True, cls_hpc_err=left_hpc_err, **extra_left), rv)


def right_reads_equal_oracle(left_o, right, cls, strand, n_reads):
    """After the oracle merged the right batch into left_o: the reads of `right` sit where (cls, strand) of their clusters say."""
    ocl, ost = left_o.assignments(n_reads)
    rcl, rst = right.assignments(n_reads)
    reads = np.nonzero(rcl >= 0)[0]
    assert np.array_equal(cls[rcl[reads]], ocl[reads])
    assert np.array_equal(strand[rcl[reads]].astype(np.int32) * rst[reads], ost[reads])
