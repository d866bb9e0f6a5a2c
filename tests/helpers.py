"""Shared test plumbing: oracle-side preparation of a sorted batch and comparison helpers.
(The oracle is test infrastructure; the product never imports it.)"""
import numpy as np

from isonclust2_amd import synth
from oracle import pyoracle as po


def oracle_sorted_batch(rs, k=11, w=15, params=None):
    """FillQualScores -> SortByQualScores -> PrepareSortedBatch (one batch holding every read) on the
    oracle; returns (oracle Batch, dict in the layout of ioc_batch_view)."""
    R = po.ReadSet.from_flat(rs.seq, rs.qual, rs.offs)
    R.score_sort(k, w)
    p = params or po.default_params(k, w)
    B = po.Batch(R, 0, rs.n - 1, p)
    info, off_f, off_r, mn, ps = B.minimizer_soa()
    view = dict(off_fwd=off_f, off_rev=off_r, min_val=mn, min_pos=ps, raw_len=info["raw_len"],
                hpc_len=info["hpc_len"], score=info["score"], raw_err=info["raw_err"],
                hpc_err=info["hpc_err"], state=info["state"].astype(np.uint8), min_qual=p.min_qual,
                orig=info["orig"])
    return B, view


def oracle_entry_assignments(B, view, mode="fast"):
    """Run the oracle's ClusterSortedReads; returns (cls, strand) per batch entry + stats."""
    st = B.cluster(mode=mode)
    n = len(view["orig"])
    acl, ast = B.assignments(int(view["orig"].max()) + 1 if n else 0)
    return acl[view["orig"]], ast[view["orig"]], st


def oracle_traced_run(rs, entries=None, k=11, w=15):
    """One fast-mode run of the oracle over `rs` as a single batch with the candidate tables of `entries` (default: all)
    traced.  Returns dict(batch, view, cls, strand, stats, rows, calls, entries)."""
    B, view = oracle_sorted_batch(rs, k, w)
    entries = list(range(rs.n)) if entries is None else list(entries)
    po.trace_set(entries, mapped_calls=True)
    try:
        ocl, ost, ostat = oracle_entry_assignments(B, view)
        rows, calls = po.trace_rows(), po.trace_mapped_calls()
    finally:
        po.trace_set(())
    return dict(batch=B, view=view, cls=ocl, strand=ost, stats=ostat, rows=rows, calls=calls, entries=entries)


def walk_lengths(rows, n, min_shared=5, min_fraction=0.8):
    """Per entry the number of candidates getBestClusterMapping's walk can reach (src/cluster.cpp:355-406): those with
    int(Size) >= int(top * MinFraction), 0 where top < MinShared or the entry has no candidate."""
    out = np.zeros(n, np.int64)
    order = np.argsort(rows["entry"], kind="stable")
    ent, size = rows["entry"][order], rows["size"][order].astype(np.int64)
    cuts = np.flatnonzero(np.diff(ent)) + 1
    for e, sz in zip(ent[np.r_[0, cuts]] if len(ent) else [], np.split(size, cuts)):
        top = int(sz.max())
        if top >= min_shared:
            out[e] = int((sz >= int(float(top) * min_fraction)).sum())
    return out


PARAM_KEYS = ("min_shared", "min_fraction", "mapped_threshold", "min_prob_no_hits", "aligned_threshold")


def param_pair(d=None, mode="fast"):
    """(api.Params, po.Params) with the same values: the defaults of CmdArgs overridden by the dict `d` (k, w and any of
    PARAM_KEYS).  The one place the product's and the oracle's parameters are made alike."""
    from isonclust2_amd import api
    d = d or {}
    bad = set(d) - set(PARAM_KEYS) - {"k", "w"}
    assert not bad, bad
    k, w = int(d.get("k", 11)), int(d.get("w", 15))
    a, o = api.default_params(k, w, mode), po.default_params(k, w, mode)
    for key in PARAM_KEYS:
        if key in d:
            setattr(a, key, d[key])
            setattr(o, key, d[key])
    return a, o


def compare_candidate_tables(ctx, view, rows, calls, entries, tgt, thr=0.65, size_cut=0, cid=None, bound=None, size_rule=0,
                             floor=None):
    """The device's candidate table of every traced entry (ctx.query_candidates) against the oracle's trace rows: the multiset of
    (cluster, strand, Size, first index), and every totalMapped either side evaluated.  thr: the MappedThreshold of the run (a
    candidate the upper bound rejected must fail it on the oracle's exact total).  size_cut: the Size below which the Size rule
    alone excludes a candidate whatever its total (int(MinShared * MinFraction), see ioc_set_params' `keep`), which the list
    cut also marks rejected: allowed to pass the threshold, never walked by the oracle.
    cid: cluster id (in the oracle's numbering) of every device target, for runs with left clusters (default: a single batch,
    L = 0, where target = the entry that opened the cluster).  bound(entry, target, strand, Size): an independent restatement of
    the upper bound of totalMapped (tests/bound_common.MappedBound) — a candidate the device rejected must be rejected by it
    too, unless the Size rule alone excludes it (Size < size_rule = int(MinShared * MinFraction)): a sound but over-tight
    device bound fails here.  floor(entry, need): the restated per-query cut of the candidate lists (tests/bound_common.size_floor,
    fast mode) — the converse for the cut: a candidate with size_rule <= Size < floor is exported as rejected, so a device cut that
    is too slack fails here.  Returns (rows, walked, device-evaluated)."""
    from isonclust2_amd import api
    n = len(tgt)
    opener = tgt < 0
    # single batch, L = 0: target = entry that opened the cluster -> cluster id in creation order
    if cid is None:
        cid = np.full(n, -1, np.int64)
        gated = np.asarray(view["state"]) != 0
        cid[opener & ~gated] = np.arange(int((opener & ~gated).sum()))
    cid = np.asarray(cid, np.int64)
    n_rows = n_walked = n_dev_eval = n_bound = 0
    for e in entries:
        m = rows["entry"] == e
        t, s, sz, fi, tm = ctx.query_candidates(int(e), 2 * max(n, len(cid)) + 2)
        dev = sorted(zip(cid[t].tolist(), s.tolist(), sz.tolist(), fi.tolist()))
        orc = sorted(zip(rows["cls"][m].tolist(), rows["strand"][m].tolist(), rows["size"][m].tolist(),
                         rows["first_index"][m].tolist()))
        assert dev == orc, (e, len(dev), len(orc))
        n_rows += len(orc)
        tot = {(c, st): (x, w) for c, st, x, w in zip(rows["cls"][m].tolist(), rows["strand"][m].tolist(),
                                                      rows["total_mapped"][m].tolist(), rows["walked"][m].tolist())}
        need = api.host_min_total(int(view["hpc_len"][e]), thr)
        for c, st, x, z, tg in zip(cid[t].tolist(), s.tolist(), tm.tolist(), sz.tolist(), t.tolist()):
            want, walked = tot[(c, st)]
            if bound is not None and x == 0xFFFFFFFE and z >= size_rule:
                assert bound(int(e), tg, st, z) < need, (e, c, st, z, bound(int(e), tg, st, z), need)
            if floor is not None and size_rule <= z < floor(int(e), need):
                assert x == 0xFFFFFFFE, (e, c, st, z, floor(int(e), need), x)
            if x == 0xFFFFFFFE and z < size_cut and want >= need:
                assert not walked, (e, c, st, z, size_cut)
                n_bound += 1
                continue
            if x == 0xFFFFFFFE:
                # rejected by the upper bound of totalMapped (k_gap_bounds) without an evaluation: the bound is sound iff the
                # oracle's exact total fails the threshold as well
                assert want < need, (e, c, st, want, need)
                n_bound += 1
                n_walked += 1 if walked else 0
                continue
            if walked:
                assert x == want, (e, c, st, x, want)          # the reference called getMappedRatio here
                n_walked += 1
            if x != 0xFFFFFFFF:
                assert x == want, (e, c, st, x, want)          # whatever the device evaluated is the oracle's value
                n_dev_eval += 1
    return n_rows, n_walked, n_dev_eval + n_bound


from isonclust2_amd.digest import fnv1a  # noqa: E402,F401  (one definition for tests, goldens and bench)


class ToyGraphs:
    """A stand-in for the per-cluster spoa graphs of the consensus (spoa is absent from the reference tree):
    the same five operations, deterministic and cheap — a "graph" is the list of (sequence, weight) it was fed,
    its consensus the heaviest sequence (ties: the latest), truncated by one base per call so that the
    representative really changes.  The SAME store semantics serve the oracle (orc_set_consensus) and the
    product (ioc_cluster_consensus): what the tests pin is everything AROUND the graphs."""

    def __init__(self, right_sizes=None):
        import ctypes as C
        from isonclust2_amd import _lib
        self.g = {0: {}, 1: {}}
        self.calls = 0
        self.rep_events = []
        self.rep_records = []  # (cluster, full ioc_rep_record as a dict of copies): what a later merge needs of a replaced representative
        self.log = []          # (operation, side, idx, sequence length / weight): compared between the two sides
        for i, s in (right_sizes or {}).items():
            self.g[1][i] = [(b"", 1)] * s
        self._C = C

        def create(user, side, idx, seq, n):
            self.g[side][idx] = [(C.string_at(seq, n), 1)]
            self.log.append(("create", side, idx, n))
            return 0

        def size(user, side, idx):
            return len(self.g[side][idx]) if idx in self.g[side] else -1

        def add(user, side, idx, seq, n, weight):
            if idx not in self.g[side]:
                return -1
            self.g[side][idx].append((C.string_at(seq, n), int(weight)))
            self.log.append(("add", side, idx, n, int(weight)))
            return 0

        def consensus(user, side, idx, out, cap):
            self.calls += 1
            items = self.g[side][idx]
            best = max(range(len(items)), key=lambda t: (items[t][1], t))
            s = items[best][0]
            s = s[: max(64, len(s) - (self.calls % 7))]
            if len(s) > cap:
                return -1
            C.memmove(out, s, len(s))
            self.log.append(("consensus", side, idx, len(s)))
            return len(s)

        def purge(user, side, idx, seq, n, weight):
            self.g[side][idx] = [(C.string_at(seq, n), int(weight))]
            self.log.append(("purge", side, idx, n, int(weight)))
            return 0

        def rep_changed(user, cls, rec):
            r = rec.contents
            self.rep_events.append((int(cls), int(r.entry), C.string_at(r.raw_seq, r.raw_len), float(r.raw_err), float(r.hpc_err),
                                    int(r.hpc_len), int(r.n_fwd), int(r.n_rev)))
            import numpy as _np
            take = lambda ptr, n: _np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else _np.zeros(0, _np.uint32)
            self.rep_records.append((int(cls), dict(
                raw_seq=C.string_at(r.raw_seq, r.raw_len), raw_len=int(r.raw_len), raw_err=float(r.raw_err),
                score=float(r.raw_score), hpc_len=int(r.hpc_len), hpc_err=float(r.hpc_err),
                fwd_min=take(r.fwd_min, r.n_fwd), fwd_pos=take(r.fwd_pos, r.n_fwd),
                rev_min=take(r.rev_min, r.n_rev), rev_pos=take(r.rev_pos, r.n_rev), entry=int(r.entry))))

        self._keep = (_lib.CONS_CREATE(create), _lib.CONS_SIZE(size), _lib.CONS_ADD(add), _lib.CONS_CONSENSUS(consensus),
                      _lib.CONS_PURGE(purge), _lib.CONS_REP_CHANGED(rep_changed))
        self.ops = _lib.ConsensusOps(None, *self._keep)

    def reset(self, right_sizes=None):
        self.g = {0: {}, 1: {}}
        self.calls = 0
        self.rep_events = []
        self.rep_records = []
        self.log = []
        for i, s in (right_sizes or {}).items():
            self.g[1][i] = [(b"", 1)] * s
