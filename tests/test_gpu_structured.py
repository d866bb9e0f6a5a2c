"""GPU parity on isoform-like and repetitive reads (tests/structured_reads.py): gene families that share a core, isoforms that
share exons, truncated reads, tandem repeats — what synth.generate's independent uniform transcripts never produce.  Which
kernel path each fixed case reaches is asserted on the CPU, with the oracle alone, in tests/test_structured_host.py:
  family44 / family340   walks of more than IOC_WALK_SLOTS (32) / IOC_SCAN_ITEMS (256) cluster candidates (k_decide_scan's spill,
                         k_decide_pick's scan of the whole list)
  isoforms_trunc, repeat3, family44   bounds of totalMapped (k_gap_bounds, bound_rejects) within 20 % of the threshold on both sides
  repeat2 / repeat3      a read that repeats one minimizer value 100+ times (k_distinct_radix, Size per occurrence, first-hit Index,
                         k_eval's hit bitmap and previous-hit table), one posting list hit by every query
  family_ties            walks of more than 32 candidates that END in a join: dozens of passing candidates, ties at the winning Size
  family_aln             alignment verdicts on both sides of aligned_threshold; the bound rejecting inside undecided walks
and the extraction kernels on low-complexity sequence, where the leftmost-argmin rule of k_minimizers has ties to break."""
import ctypes as C
import functools

import numpy as np
import pytest

from isonclust2_amd import api, pipeline
from oracle import pyoracle as po
from tests import structured_reads as sr
from tests.bound_common import MappedBound, entry_cells, in_walk_rejections, single_batch_cells, size_floor
from tests.fuzz_cases import _with_sequences
from tests.helpers import compare_candidate_tables, oracle_entry_assignments, oracle_sorted_batch
from tests.test_gpu_merge import _batches, _same_index
from tests.test_structured_host import merge_traced, traced

pytestmark = pytest.mark.gpu

K, W = 11, 15


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def oracle_mode_run(name, mode):
    """the oracle's run of a case in an alignment mode: (view with sequences, cls, strand, stats); shared, read only"""
    rs = sr.case(name)
    B, view = oracle_sorted_batch(rs)
    ocl, ost, st = oracle_entry_assignments(B, view, mode=mode)
    return _with_sequences(rs, view), ocl, ost, st


class _Counted:
    """a MappedBound that counts how often the comparison consulted it (once per candidate of Size >= the Size rule's cut that the
    device exported as rejected), and a memo of the restated list cut per query"""

    def __init__(self, bound, view, p):
        self.bound, self.calls, self.view, self.p, self._floor, self.targets = bound, 0, view, p, {}, []

    def __call__(self, *a):
        self.calls += 1
        self.targets.append(int(a[1]))
        return self.bound(*a)

    def left_calls(self, L):
        """rejected candidates whose target is one of the L left clusters"""
        return sum(t < L for t in self.targets)

    def floor(self, q, need):
        if q not in self._floor:
            self._floor[q] = size_floor(self.view, q, self.p.k, self.p.w, need, _size_cut(self.p), self.p.min_prob_no_hits)
        return self._floor[q]

    def cut_rows(self, rows, thr, only=None):
        """the oracle's rows (of the mask `only`) that the list cut removes although the Size rule alone would keep them"""
        n = 0
        for i, (e, z) in enumerate(zip(rows["entry"].tolist(), rows["size"].tolist())):
            if only is None or only[i]:
                n += _size_cut(self.p) <= z < self.floor(e, api.host_min_total(int(self.view["hpc_len"][e]), thr))
        return n


def _size_cut(p):
    """The Size below which the Size rule alone excludes a candidate (ioc_set_params' `keep`): with the defaults int(5 * 0.8) = 4.
    A truncated read of a few dozen compressed bases has candidates of Size 1 - 3 whose totalMapped is the whole read (head + tail
    alone reach the threshold: isoforms_trunc, entry 149, Size 1, total 56 of 56); the device's list cut marks them rejected, the
    oracle never walks them, and compare_candidate_tables asserts exactly that for a Size below this."""
    return max(1, min(int(p.min_shared * p.min_fraction), p.min_shared))


# ---- candidate tables, totals, the bound ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sorted(sr.CASES) if n != "family340"])
def test_candidate_tables_totals_and_bound(ctx, name):
    """Every entry's candidate table and every evaluated totalMapped against the oracle's trace (as test_gpu_candidates.py), the
    assignments, and — new — the device's bound against the numpy restatement, both ways: what the device rejects the restatement
    rejects, and what the restated list cut and the restated bound inside an undecided walk reject the device rejects.  (On
    repeat2 and repeat3 neither side rejects a candidate of Size >= 4: there the tables and totals are the test.)"""
    rs, run = traced(name)
    view, rows, calls, entries = run["view"], run["rows"], run["calls"], run["entries"]
    p = api.default_params(K, W, "fast")
    cls, strand, st = ctx.cluster_batch(p, view)
    assert np.array_equal(cls, run["cls"]) and np.array_equal(strand, run["strand"])
    assert st["n_tie_replays"] >= run["stats"]["tie_reads"]
    tgt, _, _ = ctx.decisions()
    bound = _Counted(MappedBound(view, K, W, entry_cells(view), p.min_prob_no_hits), view, p)
    n_rows, n_walked, n_dev = compare_candidate_tables(ctx, view, rows, calls, entries, tgt, thr=p.mapped_threshold, bound=bound,
                                                       size_cut=_size_cut(p), size_rule=_size_cut(p), floor=bound.floor)
    assert n_rows == len(rows["entry"]) and n_rows > 10 * len(entries) // 4
    assert n_walked == int(np.isin(calls["entry"], entries).sum())        # every getMappedRatio call of the oracle was seen
    assert n_dev >= n_walked
    # What the device rejected: the rows the restated list cut removes (asserted one by one in compare_candidate_tables) and, in the
    # sweeps, with the TARGET's own error cell, the rows in reach of an undecided walk that the restated bound rejects.  The two
    # sets are disjoint.  test_structured_host.py: family_aln and family_ties have in-walk rejections; family44 and
    # isoforms_trunc list cuts only; on repeat2 and repeat3 the device rejects nothing of Size >= 4 (the shared block gives every
    # candidate in reach a Size of 100 or more), so there this check of the bound is idle and the tables and totals are the test.
    in_walk = in_walk_rejections(MappedBound(view, K, W, single_batch_cells(view, run["cls"]), p.min_prob_no_hits), view, rows, K, W)
    assert bound.calls >= bound.cut_rows(rows, p.mapped_threshold) + in_walk
    if name in ("family_aln", "family_ties"):
        assert in_walk >= 20


def test_bound_with_left_clusters_in_a_two_batch_merge(ctx):
    """The same comparison for `cluster -l -r` of family_aln in two batches: the targets are left clusters (their error cells:
    left_err) and the right representatives that opened a cluster before the query.  test_structured_host.py: dozens of
    candidates with a left target lie in reach of an undecided walk and are rejected by the bound of the left cluster's own cell."""
    rs = sr.case("family_aln")
    m = merge_traced("family_aln")
    obs, sbs, rows, calls = m["obs"], m["sbs"], m["rows"], m["calls"]
    p = api.default_params(K, W, "fast")
    left, right = (pipeline.cluster_single(ctx, p, sb) for sb in sbs)
    L, nR = left.n_clusters, right.n_clusters
    assert L == m["L"] and nR == m["nR"] and L > 20 and nR > 20
    entries = list(range(nR))
    rv = dict(right.rep_view)
    rv.update(n_members=np.bincount(right.member_cls, minlength=nR).astype(np.int32), depth=right.depth, min_cls_size=3)
    lv = dict(cls_hpc_err=left.rep_view["hpc_err"], keys=left.mindb[0], offs=left.mindb[1], postings=left.mindb[2])
    cls, strand, st = ctx.cluster_merge(p, lv, rv)
    tgt, _, _ = ctx.decisions()
    # the oracle's decisions: the left cluster every right cluster's members ended up in
    ocl, ost = obs[0].assignments(rs.n)
    first_member = np.array([right.member_read[np.nonzero(right.member_cls == c)[0][0]] for c in range(nR)])
    assert np.array_equal(cls, ocl[first_member])
    # device target -> cluster id: a left cluster is its own id, a right representative the id it was given when it opened one
    cid = np.concatenate([np.arange(L), np.where(tgt < 0, cls, -1)]).astype(np.int64)
    cells = np.concatenate([[api.host_err_cell(float(e)) for e in left.rep_view["hpc_err"]], entry_cells(rv)])
    bound = _Counted(MappedBound(rv, K, W, cells, p.min_prob_no_hits), rv, p)
    n_rows, n_walked, n_dev = compare_candidate_tables(ctx, rv, rows, calls, entries, tgt, thr=p.mapped_threshold, cid=cid,
                                                       bound=bound, size_cut=_size_cut(p), size_rule=_size_cut(p), floor=bound.floor)
    assert n_rows == len(rows["entry"]) and n_rows > 10 * nR // 4
    assert n_walked == int(np.isin(calls["entry"], entries).sum()) and n_dev >= n_walked
    assert int((rows["cls"] < L).sum()) > 100 and int((rows["cls"] >= L).sum()) > 100     # both kinds of target were compared
    # rejections inside undecided walks whose target is a LEFT cluster (a left cluster's id is its target number): left_err decided
    left_rows = rows["cls"] < L
    in_walk_left = in_walk_rejections(MappedBound(rv, K, W, cells, p.min_prob_no_hits), rv, rows, K, W, only=left_rows)
    assert in_walk_left >= 10
    assert bound.left_calls(L) >= bound.cut_rows(rows, p.mapped_threshold, only=left_rows) + in_walk_left
    assert bound.calls >= bound.cut_rows(rows, p.mapped_threshold) + in_walk_left


# ---- the resolve shortcuts where walks are long ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["family340", "family_ties"])
def test_resolve_shortcuts_on_walks_beyond_the_scan_items(ctx, monkeypatch, name):
    """family340: dozens of queries with more than 256 candidates in reach of the walk, none passing; family_ties: walks of more
    than 32 with dozens of passing candidates and ties at the winning Size.  With the bound and the list cut, without the cut,
    without both (every walk candidate is queued: on family340 the spill past IOC_SCAN_ITEMS), and with a queue of 64 items: the
    oracle's assignments every time, each shortcut only ever removes evaluations, and without them nothing the oracle evaluated
    is lost (an item dropped in the spill or at a full queue would be)."""
    _, run = traced(name)
    view = run["view"]
    p = api.default_params(K, W, "fast")
    evals = []
    for bound, keepq, cap in (("1", "1", None), ("1", "0", None), ("0", "0", None), ("1", "1", "64"), ("0", "0", "64")):
        monkeypatch.setenv("IOC_RESOLVE_BOUND", bound)
        monkeypatch.setenv("IOC_SCORE_KEEPQ", keepq)
        if cap:
            monkeypatch.setenv("IOC_QUEUE_CAP", cap)
        cls, strand, st = ctx.cluster_batch(p, view)
        assert np.array_equal(cls, run["cls"]) and np.array_equal(strand, run["strand"]), (bound, keepq, cap)
        assert st["n_tie_replays"] >= run["stats"]["tie_reads"]
        evals.append(int(ctx.timings()["n_mapped_evals"]))
    assert evals[0] <= evals[1] <= evals[2], evals
    # every getMappedRatio call of the oracle is a distinct (query, candidate) of some walk: with no shortcut the device evaluates it
    oracle_calls = int(run["rows"]["walked"].sum())
    assert oracle_calls == len(run["calls"]["entry"]) and oracle_calls > 256
    assert evals[2] >= oracle_calls and evals[4] >= oracle_calls, (evals, oracle_calls)


# ---- index builds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["repeat2", "family44"])
@pytest.mark.parametrize("switches", [{"IOC_POST16": "0"}, {"IOC_BUILD_SORT": "0"}, {"IOC_POST16": "0", "IOC_BUILD_SORT": "0"}],
                         ids=["post32", "hash_build", "post32_hash_build"])
def test_builds_and_posting_widths_on_repeats_and_families(ctx, monkeypatch, switches, name):
    rs, run = traced(name)
    B = run["batch"]
    sb = pipeline.SortedBatch(view=run["view"], read_ids=run["view"]["orig"].astype(np.int64), batch_nr=0, batch_start=0,
                              batch_end=rs.n - 1)
    for key, value in switches.items():
        monkeypatch.setenv(key, value)
    cb = pipeline.cluster_single(ctx, api.default_params(K, W, "fast"), sb)
    ocl, ost = B.assignments(rs.n)
    cls, strand = cb.assignments(rs.n)
    assert np.array_equal(cls, ocl) and np.array_equal(strand, ost)
    _same_index(cb, B)


@pytest.mark.parametrize("name,chunk", [("isoforms_trunc", None), ("repeat3", None), ("repeat3", "37")])
def test_three_batch_left_fold(ctx, monkeypatch, name, chunk):
    """((b0 + b1) + b2): assignments and MinDB after every step; once with the right batches run in chunks of 37 entries"""
    rs = sr.case(name)
    obs, sbs = _batches(rs, 3)
    p = api.default_params(K, W, "fast")
    if chunk:
        monkeypatch.setenv("IOC_MERGE_CHUNK", chunk)
    for B in obs:
        B.cluster(mode="fast")
    cbs = [pipeline.cluster_single(ctx, p, sb) for sb in sbs]
    for cb, B in zip(cbs, obs):
        _same_index(cb, B)
    left_o, left = obs[0], cbs[0]
    for b in (1, 2):
        left_o.cluster(right=obs[b], mode="fast")
        left = pipeline.cluster_merge(ctx, p, left, cbs[b])
        ocl, ost = left_o.assignments(rs.n)
        cls, strand = left.assignments(rs.n)
        bad = np.nonzero((cls != ocl) | (strand != ost))[0]
        assert len(bad) == 0, (b, len(bad), bad[:5], cls[bad[:5]], ocl[bad[:5]])
        assert left.n_clusters == left_o.n_clusters()
        _same_index(left, left_o)


# ---- alignment modes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode,host", [("family_aln", "sahlin", False), ("family_aln", "furious", False),
                                            ("isoforms_trunc", "sahlin", False), ("family_aln", "sahlin", True)])
def test_alignment_modes(ctx, monkeypatch, name, mode, host):
    """The fallback aligns members of one family (verdicts on both sides of aligned_threshold: verdict mode's early stop and the
    driver's speculative verdicts against the exact count) and truncated isoforms; once with the host aligner (IOC_ALIGN_HOST)."""
    v, ocl, ost, ostat = oracle_mode_run(name, mode)
    assert ostat["aln_invoked"] > 0
    if host:
        monkeypatch.setenv("IOC_ALIGN_HOST", "1")
    cls, strand, st = ctx.cluster_batch(api.default_params(K, W, mode), v)
    bad = np.nonzero((cls != ocl) | (strand != ost))[0]
    assert len(bad) == 0, (len(bad), bad[:5], cls[bad[:5]], ocl[bad[:5]])
    assert st["n_aln_invoked"] == ostat["aln_invoked"]


# ---- extraction on low-complexity sequence ---------------------------------------------------------------------------------------
def _stable(rng, n, not_first=None):
    """n random letters, no two neighbours equal (homopolymer compression leaves it alone); not_first: a letter to avoid at 0"""
    out = np.zeros(n, np.int64)
    for i in range(n):
        avoid = out[i - 1] if i else (b"ACGT".index(not_first) if not_first is not None else -1)
        out[i] = (avoid + rng.integers(1, 4)) % 4 if avoid >= 0 else rng.integers(0, 4)
    return bytes(b"ACGT"[int(x)] for x in out)


def _tandem(rng, period, n, not_first=None):
    while True:
        u = sr.repeat_unit(rng, period).tobytes()
        if not_first is None or u[0] != not_first:
            return (u * (n // period + 1))[:n]


def _two_letter(rng, hpc_len):
    """two letters in random runs of 1 - 2: `hpc_len` runs (its compressed form alternates)"""
    a, b = (b"ACGT"[int(x)] for x in rng.choice(4, 2, replace=False))
    return b"".join(bytes([a if i % 2 == 0 else b]) * int(rng.choice([1, 1, 2])) for i in range(hpc_len))


def extraction_reads(k, w, seed=0):
    """Reads for one (k, w): tandem repeats of eight periods, two-letter reads and mixtures of random and repeat at compressed
    lengths that give 255 .. 513 windows (the 256-window tile of k_minimizers and its edges), and reads at and one below the
    gates 2k and w."""
    rng = np.random.default_rng([seed, k, w])
    reads = []
    for nw in (255, 256, 257, 511, 512, 513):
        n = nw + w                                   # windows = compressed length - w
        for period in (2, 3, 4, 5, 7, 12, 30, 257):
            reads.append(_tandem(rng, period, n))
        reads.append(_two_letter(rng, n))
        a = _stable(rng, n // 3)
        b = _tandem(rng, int(rng.choice([2, 3])), n // 3, not_first=a[-1])
        reads.append(a + b + _stable(rng, n - len(a) - len(b), not_first=b[-1]))
    for n in sorted({2 * k - 1, 2 * k, w - 1, w, max(2 * k, w), max(2 * k, w) + 1}):
        reads += [_stable(rng, n), _tandem(rng, 3, n), _tandem(rng, 2, n)]
    quals = [bytes(rng.integers(34, 91, len(r)).astype(np.uint8)) for r in reads]
    return reads, quals


def check_extraction(ctx, reads, quals, k, w):
    """ioc_extract_minimizers of the reads against po.hpc / po.error_rate / po.kmer_encode / po.revcomp / po.minimizers, bit for
    bit: compressed strings and qualities, status, error rate, both strands' (value, position) lists.  Returns the statuses."""
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    ex = ctx.extract_minimizers(offs, np.frombuffer(b"".join(reads), np.uint8), np.frombuffer(b"".join(quals), np.uint8), k, w)
    mn, ps = ctx.extracted_download(int(ex["off_rev"][-1]))
    total = int(offs[-1])
    dseq, dqual = C.create_string_buffer(total), C.create_string_buffer(total)
    ctx._chk(ctx.L.ioc_extracted_hpc_download(ctx.h, dseq, dqual, total))
    for i, (s, q) in enumerate(zip(reads, quals)):
        hs, hq = po.hpc(s, q)
        assert ex["hpc_len"][i] == len(hs), (i, ex["hpc_len"][i], len(hs))
        a = int(offs[i])
        assert dqual.raw[a:a + len(hs)] == hq, i
        empty = ex["off_fwd"][i + 1] == ex["off_fwd"][i] and ex["off_rev"][i + 1] == ex["off_rev"][i]
        if any(c not in b"ACGT" for c in s):
            assert ex["status"][i] == 2 and empty, (i, ex["status"][i])
            continue
        assert dseq.raw[a:a + len(hs)] == hs, i
        if len(hs) < 2 * k or len(hs) < w:
            assert ex["status"][i] == 1 and empty, (i, len(hs), ex["status"][i])
            continue
        assert ex["status"][i] == 0, (i, len(hs))
        assert ex["hpc_err"][i] == po.error_rate(hq, nomin=True), i
        for strand, off in ((0, ex["off_fwd"]), (1, ex["off_rev"])):
            seq = hs if strand == 0 else po.revcomp(hs)
            emn, eps, _ = po.minimizers(po.kmer_encode(seq, k), k, w)
            lo, hi = int(off[i]), int(off[i + 1])
            assert hi - lo == len(emn), (i, strand, len(hs), hi - lo, len(emn))
            assert np.array_equal(mn[lo:hi], emn), (i, strand, len(hs))
            assert np.array_equal(ps[lo:hi], eps), (i, strand, len(hs))
    return ex["status"]


@pytest.mark.parametrize("k,w", [(11, 15), (10, 10), (11, 42), (15, 15), (16, 20), (16, 47), (17, 20), (32, 32), (32, 63)])
def test_extract_low_complexity_bitwise(ctx, k, w):
    """Ties inside a window are what the leftmost-argmin rule is for, and they arise only on low-complexity sequence: across the
    256-window tile edge, across a wave's first lane, at W = w - k + 1 = 32 (the widest the entry takes), at k = 16 and 32 (the
    mask and the 32-bit wrap of the k-mer value)."""
    reads, quals = extraction_reads(k, w)
    status = check_extraction(ctx, reads, quals, k, w)
    assert int((status == 0).sum()) >= 60 and int((status == 1).sum()) >= 3


def homopolymer_reads(seed=3):
    """Runs of 255, 256, 257 and 600 equal bases that start at offset 1, 255 and 256 of the read (k_hpc works in chunks of 256
    bases: the run's head in one chunk, its best quality chunks later, on its last base); a base outside ACGT as the last base,
    and one inside a run."""
    rng = np.random.default_rng(seed)
    reads, quals = [], []
    for run in (255, 256, 257, 600):
        for at in (1, 255, 256):
            base = b"ACGT"[int(rng.integers(0, 4))]
            pre = _stable(rng, at, not_first=base)[::-1]                   # (ends in a letter other than the run's)
            suf = _stable(rng, 60, not_first=base)
            reads.append(pre + bytes([base]) * run + suf)
            q = rng.integers(40, 61, len(reads[-1])).astype(np.uint8)
            q[at:at + run] = 35
            q[at + run - 1] = 93                                           # the run's highest quality: its last base
            quals.append(bytes(q))
    stable = _stable(rng, 80)
    reads += [stable + b"N", stable[:40] + b"AAAANAAAA" + _stable(rng, 40, not_first=ord("A"))]
    quals += [bytes(rng.integers(40, 61, len(r)).astype(np.uint8)) for r in reads[-2:]]
    return reads, quals


def test_extract_long_homopolymer_runs_and_foreign_bases(ctx):
    reads, quals = homopolymer_reads()
    for r, q in zip(reads[:12], quals[:12]):
        hs, hq = po.hpc(r, q)
        assert 93 in hq and len(hs) <= len(r) - 254          # (the case is what it says: a long run, its best quality kept)
    status = check_extraction(ctx, reads, quals, K, W)
    assert status.tolist() == [0] * 12 + [2, 2]


def qual_strings(k, seed=11):
    rng = np.random.default_rng([seed, k])
    out = []
    for n in (2 * k, 2 * k + 1, 2 * k + 2, 3 * k + 5, 700):
        plain = rng.integers(34, 127, n).astype(np.uint8)
        edge = plain.copy()
        u = rng.random(n)
        edge[u < 0.1] = ord("!")                        # the capped table entry (p = 1 -> 0.79433)
        edge[u > 0.9] = ord("~")
        head = plain.copy()
        head[:k] = ord("!")
        out += [bytes(plain), bytes(edge), bytes(head), b"!" * n, b"~" * n]
    return out


@pytest.mark.parametrize("k", [1, 32, 64, 65])
def test_qual_scores_edges_bitwise(ctx, k):
    """CalcQualScore / CalcErrorRate with `!` (the capped table entry) and `~`, at the length gate 2k and one above it, and with
    a first-k product that runs over more than one wave's worth of lanes (k = 64, 65)."""
    quals = qual_strings(k)
    offs = np.zeros(len(quals) + 1, np.int64)
    offs[1:] = np.cumsum([len(q) for q in quals])
    score, err = ctx.qual_scores(offs, np.frombuffer(b"".join(quals), np.uint8), k)
    for i, q in enumerate(quals):
        if len(q) > 2 * k:
            qs = po.qual_score(q, k)
            assert score[i] == (qs if qs > 0 else -1.0), (i, len(q), score[i], qs)
            assert err[i] == po.error_rate(q, nomin=True), (i, len(q))
        else:
            assert score[i] == -1.0 and err[i] == 1.0, (i, len(q))


def test_sort_stage_of_a_structured_set(ctx):
    """`sort` on the GPU (quality scores, order, extraction) of the truncated tandem-repeat reads equals the oracle's sorted batch"""
    rs, run = traced("repeat3")
    view = run["view"]
    sb, order = pipeline.sort_stage(ctx, rs, K, W)
    assert np.array_equal(order, view["orig"])
    for key in ("off_fwd", "off_rev", "min_val", "min_pos", "hpc_len"):
        assert np.array_equal(np.asarray(sb.view[key]), np.asarray(view[key])), key
