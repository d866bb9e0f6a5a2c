"""ioc_left_adopt: the clustering just resolved becomes the context's left state on the device — what ioc_index_export
followed by ioc_left_load would have loaded (the MinDB as CSR, the per-cluster value sets, the err cells), with no key and no
posting on the host.  Against the product's own export, and — through pipeline.cluster_stream, merges and ioc_index_update on
top of the adopted state — against the oracle's ClusterSortedReads (src/cluster.cpp:67-322) and UpdateMinDB
(src/minimizer.cpp:124-160)."""
import numpy as np
import pytest

from isonclust2_amd import api, pipeline, synth
from tests import adopt_common as ac
from tests.helpers import oracle_entry_assignments, oracle_sorted_batch, param_pair
from tests.test_gpu_parity import _concat
from tests.test_update_mindb import _rep_values

pytestmark = pytest.mark.gpu

CUTS = (0, 1, 64, 128, 193)      # slices of 1, 63, 64, 65 entries and the rest
IOC_ERR_STATE = -3


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _adopt_equals_export(ctx, n_clusters):
    """index_export, left_adopt, left_export: the same three arrays, the count returned; a second adoption has nothing to adopt."""
    exported = ctx.index_export()
    assert ctx.left_adopt() == n_clusters
    ac.same_mindb(ctx.left_export(), exported)
    with pytest.raises(api.IocError) as e:
        ctx.left_adopt()
    assert e.value.code == IOC_ERR_STATE
    return exported


@pytest.mark.parametrize("kw", [{}, {"k": 16, "w": 16}], ids=["k11_sorted_build", "k16_hash_build"])
def test_adopt_equals_export(ctx, kw):
    """One batch, fast mode; k = 16 takes the hash build with 32-bit values."""
    p, op = param_pair(kw)
    rs = synth.generate(300, 20, 400)
    B, view = oracle_sorted_batch(rs, op.k, op.w, op)
    ocl, ost, _ = oracle_entry_assignments(B, view)
    cls, strand, st = ctx.cluster_batch(p, view)
    assert np.array_equal(cls, ocl) and np.array_equal(strand, ost)
    assert st["n_clusters"] == B.n_clusters() > 1
    exported = _adopt_equals_export(ctx, st["n_clusters"])
    ac.same_mindb(exported, B.index())


def _read_sets():
    plain = synth.generate(300, 20, 400)
    # reads of 12 kb at Q6 score above every 400-base read and fail the quality gate (cluster.cpp:157): they head the sorted
    # batch; a 3 kb read at Q20 scores above them
    bad1, bad63 = synth.generate(1, 1, 12000, 5.5, 6.5, seed=11), synth.generate(63, 2, 12000, 5.5, 6.5, seed=12)
    top = synth.generate(1, 1, 3000, 20, 21, seed=13)
    return {"plain": plain, "gated_first_slice": _concat(synth.generate(299, 20, 400, seed=2), bad1),
            "gated_middle_slice": _concat(_concat(synth.generate(236, 20, 400, seed=3), bad63), top)}


@pytest.fixture(scope="module")
def stream_inputs():
    out = {}
    for name, rs in _read_sets().items():
        B, view = oracle_sorted_batch(rs)
        out[name] = (rs, ac.with_sequences(rs, view))
    return out


@pytest.mark.parametrize("name,mode", [("plain", "fast"), ("plain", "sahlin"), ("plain", "furious"), ("gated_first_slice", "fast"),
                                       ("gated_middle_slice", "fast"), ("gated_middle_slice", "sahlin")])
def test_stream_equals_whole(ctx, stream_inputs, name, mode):
    """One sorted batch in slices through cluster_stream: the oracle's clustering of the whole batch."""
    rs, view = stream_inputs[name]
    gated = ac.gate_mask(view)
    if name == "gated_first_slice":
        assert gated[0] and not gated[1:64].all()                     # adoption with L == 0 and no new cluster
    if name == "gated_middle_slice":
        assert not gated[0] and gated[1:64].all()                     # adoption that adds nothing to a left state of one cluster
    B, _ = oracle_sorted_batch(rs)
    ocl, ost, _ = oracle_entry_assignments(B, view, mode=mode)
    sb = ac.sorted_batch(view)
    cuts = CUTS + (rs.n,)
    slices = [pipeline.slice_sorted(sb, a, b, batch_nr=j) for j, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]
    cb = pipeline.cluster_stream(ctx, api.default_params(11, 15, mode), slices)
    acl, ast = cb.assignments(rs.n)
    assert np.array_equal(acl[view["orig"]], ocl) and np.array_equal(ast[view["orig"]], ost)
    assert cb.n_clusters == B.n_clusters() > 1
    ac.same_mindb(cb.mindb, B.index())
    opened = np.nonzero(ocl >= 0)[0][np.unique(ocl[ocl >= 0], return_index=True)[1]]
    assert np.array_equal(cb.rep_entry, opened)                       # the representatives the stream kept are the entries that opened clusters


def _adopt_then_merge(ctx, rs, kw):
    """Two consecutive batches: the first clustered and adopted (adopt-equals-export), the second merged against the adopted
    state — the oracle's Batch.cluster(right=...)."""
    p, op = param_pair(kw)
    obs, sbs = ac.two_batches(rs, op)
    for B in obs:
        B.cluster(mode="fast")
    right = pipeline.cluster_single(ctx, p, sbs[1])
    left = pipeline.cluster_single(ctx, p, sbs[0])
    assert left.n_clusters == obs[0].n_clusters() and right.n_clusters == obs[1].n_clusters()
    exported = _adopt_equals_export(ctx, left.n_clusters)
    ac.same_mindb(exported, obs[0].index())
    obs[0].cluster(right=obs[1], mode="fast")
    cls, strand, st = ac.merge_resident(ctx, p, left.rep_view["hpc_err"], right)
    ac.right_reads_equal_oracle(obs[0], right, cls, strand, rs.n)
    assert st["n_clusters"] == obs[0].n_clusters()
    ac.same_mindb(ctx.index_export(), obs[0].index())
    return left, exported


def test_long_posting_lists(ctx):
    """MappedThreshold 1.01: no read maps, every read opens a cluster.  A posting list holds at most one cluster per read of the
    transcript the key comes from, so lists longer than a 256-thread workgroup need more than 256 reads per transcript in the
    adopted batch: 2400 reads of 300 bases over 3 transcripts, 400 per transcript and batch (the oracle finds lists of 362
    clusters in the first batch and of 595 after the merge)."""
    left, exported = _adopt_then_merge(ctx, synth.generate(2400, 3, 300), {"mapped_threshold": 1.01})
    assert left.n_clusters == 1200 and int(np.diff(exported[1]).max()) > 256
    assert int(np.diff(ctx.index_export()[1]).max()) > 512


def test_long_value_set(ctx):
    """A 200 kb read among 50 ordinary ones opens a cluster: a value set of tens of thousands of values."""
    rs = _concat(synth.generate(50, 5, 1500, 10, 21, seed=71), synth.generate(1, 1, 200000, 12, 18, seed=72))
    left, exported = _adopt_then_merge(ctx, rs, {})
    assert int(np.bincount(exported[2]).max()) > 30000


def test_both_posting_widths(ctx):
    """A small slice (16-bit postings), then a slice padded with 70 000 gated entries (32-bit postings: L + n > 65 535)."""
    p, op = param_pair()
    rs = synth.generate(300, 20, 400)
    B, view = oracle_sorted_batch(rs)
    ocl, ost, _ = oracle_entry_assignments(B, view)
    sb = ac.sorted_batch(view)
    first, rest = pipeline.slice_sorted(sb, 0, 40), pipeline.slice_sorted(sb, 40, rs.n)
    plain = pipeline.cluster_stream(ctx, p, [first, rest])
    n_pad = 70000 + (rs.n - 40)
    pos = np.linspace(100, n_pad - 100, rs.n - 40).astype(np.int64)
    padded = pipeline.SortedBatch(view=ac.pad_view(rest.view, n_pad, pos), read_ids=np.full(n_pad, -1, np.int64))
    cls0, strand0, st0 = ctx.cluster_batch(p, first.view)
    assert ctx.left_adopt() == st0["n_clusters"] > 0
    cls1, strand1, st1 = ctx.cluster_merge(p, dict(resident=True, cls_hpc_err=plain.rep_view["hpc_err"][:st0["n_clusters"]]), padded.view)
    assert ctx.timings()["n_queries"] == n_pad
    real = np.zeros(n_pad, bool)
    real[pos] = True
    assert np.all(cls1[~real] == -1) and np.all(strand1[~real] == 0)
    cls, strand = np.concatenate([cls0, cls1[pos]]), np.concatenate([strand0, strand1[pos]])
    assert np.array_equal(cls, ocl) and np.array_equal(strand, ost)
    acl, ast = plain.assignments(rs.n)
    assert np.array_equal(cls, acl[view["orig"]]) and np.array_equal(strand, ast[view["orig"]])
    assert st1["n_clusters"] == B.n_clusters() == plain.n_clusters
    exported = _adopt_equals_export(ctx, st1["n_clusters"])           # (an adoption behind a pass on 32-bit postings)
    ac.same_mindb(exported, B.index())
    ac.same_mindb(exported, plain.mindb)


def test_edits_after_adoption(ctx):
    """ioc_index_update on the adopted state, for a cluster the adopted pass opened and for one that was left before it: pins
    the transposed value sets (the update refuses old minimizers that are not the cluster's set) and the slots.  Then a merge."""
    p, op = param_pair()
    rs = synth.generate_config("config1", seed=4)
    obs, sbs = ac.two_batches(rs, op)
    for B in obs:
        B.cluster(mode="fast")
    right = pipeline.cluster_single(ctx, p, sbs[1])
    n0 = len(sbs[0].view["hpc_len"])
    cut = n0 // 3
    left = pipeline.cluster_stream(ctx, p, [pipeline.slice_sorted(sbs[0], 0, cut), pipeline.slice_sorted(sbs[0], cut, n0)])
    ncl = left.n_clusters
    assert ncl == obs[0].n_clusters() and left.rep_entry[0] < cut <= left.rep_entry[ncl - 1]
    assert ctx.left_adopt() == ncl
    left_o = obs[0]
    for c, src in [(ncl - 1, 2), (0, 3), (1, 2)]:
        old, new = _rep_values(left_o, c), _rep_values(left_o, src)
        left_o.update_mindb(c, old, new)
        ctx.index_update(c, old, new)
    keys, offs, post = left_o.index()
    assert np.any(np.diff(offs) == 0), "a key whose list became empty stays"
    ac.same_mindb(ctx.left_export(), (keys, offs, post))
    with pytest.raises(Exception):       # (the sets are what the update checks its old minimizers against)
        ctx.index_update(3, _rep_values(left_o, 4), _rep_values(left_o, 3))
    left_o.cluster(right=obs[1], mode="fast")
    cls, strand, st = ac.merge_resident(ctx, p, left.rep_view["hpc_err"], right)
    ac.right_reads_equal_oracle(left_o, right, cls, strand, rs.n)
    assert st["n_clusters"] == left_o.n_clusters()


def test_after_a_chunked_call(ctx, monkeypatch):
    """ioc_cluster_merge in chunks of 37: the state it ends in is adopted like any other, and a chunked call may start from
    the resident left state."""
    p, op = param_pair()
    rs = synth.generate(600, 40, 400)
    obs, sbs = ac.two_batches(rs, op)
    for B in obs:
        B.cluster(mode="fast")
    assert len(sbs[0].view["hpc_len"]) == 300
    right = pipeline.cluster_single(ctx, p, sbs[1])
    monkeypatch.setenv("IOC_MERGE_CHUNK", "37")
    cls, strand, st = ctx.cluster_batch(p, sbs[0].view)
    assert st["n_clusters"] == obs[0].n_clusters()
    exported = _adopt_equals_export(ctx, st["n_clusters"])
    ac.same_mindb(exported, obs[0].index())
    left = pipeline.cluster_single(ctx, p, sbs[0])
    assert ctx.left_adopt() == left.n_clusters
    monkeypatch.setenv("IOC_MERGE_CHUNK", "7")
    assert right.n_clusters > 3 * 7
    obs[0].cluster(right=obs[1], mode="fast")
    cls, strand, st = ac.merge_resident(ctx, p, left.rep_view["hpc_err"], right)
    ac.right_reads_equal_oracle(obs[0], right, cls, strand, rs.n)
    assert st["n_clusters"] == obs[0].n_clusters()
    ac.same_mindb(ctx.index_export(), obs[0].index())
