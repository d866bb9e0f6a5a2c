"""ioc_align_pairs_blocks_correct: ioc_align_pairs_blocks with the slot, length and position planes projected beside the base
plane, and k_group_pile and the kernels of ioc_iso_correct.hip over the planes behind the block kernels, with the block stage's
group as the groups.  Everything align_pairs_blocks returns must equal that call's own result on the same pairs, as bytes; every
pair's corrected bytes and record must equal the stand-alone call's, ioc_planes_correct_groups on planes projected on the host from
ioc_align_pairs_ops' bytes, as bytes.

The planted case (iso_correct_common.planted_isoforms, built with tests/structured_reads.py; seed 3): a representative of 400 bases,
12 reads of it, 4 reads of an isoform that skips 20 rows of it — at most max_run 24, and 4 < need(19) = 5, so a correction against the
whole cluster pastes the exon back — and 3 reads that carry an exon of 40 bases the representative lacks.  On the CPU restatement
alone (test_the_two_conditions_on_the_cpu), host aligner and host projections: the rule of ioc_align_pairs_correct fills 21, 18, 23
and 20 rows into the four minority reads and the exon is back in all four; held against their own isoform's table they keep lacking
it.  The summed edit distance of the 19 corrected reads to what each was read from is 185 under ioc_align_pairs_correct's rule (60 in
the four minority reads, 120 in the three carriers, whose exon the slot planes cut to six bases) and 6 under the new one (334 before
any correction)."""
import numpy as np
import pytest

from isonclust2_amd import api
from tests import blocks_common as bc
from tests import correct_common as cc
from tests import iso_correct_common as ic
from tests import polish_common as pc

N_MAJOR, N_MINOR, N_CARRY = ic.PLANTED_SIZES
MINOR = range(N_MAJOR, N_MAJOR + N_MINOR)
CARRY = range(N_MAJOR + N_MINOR, N_MAJOR + N_MINOR + N_CARRY)
BLOCKS = {**bc.DEFAULT, **ic.PLANTED_BLOCKS}
CORRECT = {"correct_" + k: v for k, v in ic.PLANTED_RULE.items()}


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


@pytest.fixture(scope="module")
def case():
    T, reads, truths = ic.planted_isoforms()
    n = len(reads)
    return dict(T=T, reads=reads, truths=truths, n=n, seqs=[T] + reads, pairs=[(1 + i, 0, 0, 0.1) for i in range(n)], segs=[(0, 0)], sop=[0] * n)


def _planes(T, reads, opss):
    planes = [ic.project_all(ops, rd, len(T)) for ops, rd in zip(opss, reads)]
    return tuple([p[x] for p in planes] for x in range(4))


def _distances(case, opss, seqs):
    return [pc.distance(ic.whole_read(case["reads"][i], opss[i], seqs[i]), case["truths"][i]) for i in range(case["n"])]


def test_the_two_conditions_on_the_cpu(case):
    """established on the restatement alone, before anything runs on the device: the host aligner, the host projections, the block
    search's definition, and py_correct_groups with every pair in no group (today's rule; its planes cut to six bases a run, as
    ioc_align_pairs_correct has them) and with the block search's groups (the new one)"""
    T, reads, n = case["T"], case["reads"], case["n"]
    opss = [api.host_align_ops(rd, T, gap_open=pc.gap_open(0.1))[0] for rd in reads]
    base, slots, ilen, qpos = _planes(T, reads, opss)
    blk = api.planes_blocks(np.array(base, np.uint8), **BLOCKS)
    group, ng = blk["reads"]["group"].tolist(), int(blk["seg"]["n_groups"])
    assert ng == 2 and group == [0] * N_MAJOR + [1] * N_MINOR + [0] * N_CARRY
    assert [(int(b["first"]), int(b["end"])) for b in blk["blocks"]] == [ic.EXON]
    short = [np.minimum(l, ic.SLOTS).astype(np.uint8) for l in ilen]
    old = ic.py_correct_groups([T], case["sop"], [-1] * n, [ng], reads, base, slots, short, qpos, **ic.PLANTED_RULE)
    new = ic.py_correct_groups([T], case["sop"], group, [ng], reads, base, slots, ilen, qpos, **ic.PLANTED_RULE)
    assert [o == c for o, c in zip(old[0], [cc.py_correct(b, s, *_whole_tables(T, base, slots), T, **ic.PLANTED_RULE)[0] for b, s in zip(base, slots)])] == [True] * n
    d_old, d_new = _distances(case, opss, old[0]), _distances(case, opss, new[0])
    for i in MINOR:   # today's rule fills the skipped exon in — the read is now nearer to T than to what it was read from —, the new one does not
        assert _nearer_to_the_representative(case, opss, i, old[0][i]) and not _nearer_to_the_representative(case, opss, i, new[0][i])
        assert old[2][i]["n_fill"] >= 18 and d_old[i] >= 14 and new[2][i]["n_fill"] <= 8 and d_new[i] == 0
        assert new[2][i]["table"] == 1 and new[2][i]["n_guarded"] == 0
    print("summed distance to the truth: today's rule", sum(d_old), "by isoform", sum(d_new), "uncorrected", sum(pc.distance(r, t) for r, t in zip(reads, case["truths"])))
    assert (sum(d_old), sum(d_new)) == (185, 6)   # (the sums in the docstring and in DESIGN.md)
    assert sum(d_new) <= sum(d_old)


def _nearer_to_the_representative(case, opss, i, corrected):
    whole = ic.whole_read(case["reads"][i], opss[i], corrected)
    return pc.distance(whole, case["T"]) < pc.distance(whole, case["truths"][i])


def _whole_tables(T, base, slots):
    cols, ins = np.zeros(len(T) + 1, api.PILEUP_DTYPE), np.zeros(len(T) + 1, api.PILEUP_INS_DTYPE)
    for b, s in zip(base, slots):
        api.planes_pile(b, s, cols=cols, ins=ins)
    return cols, ins


BLOCK_KEYS = ("score", "windows", "ratio", "block_off", "reads", "seg", "stats", "cols", "row0")


@pytest.fixture(scope="module")
def fused(ctx, case):
    ctx.align_set_pool(case["seqs"])
    got = ctx.align_pairs_blocks_correct(case["pairs"], 11, case["segs"], case["sop"], tables=True, stats=True, **CORRECT, **ic.PLANTED_BLOCKS)
    opss = ctx.align_pairs_ops(case["pairs"], 11)[3]
    return got, opss


@pytest.mark.gpu
def test_the_block_outputs_are_the_blocks_call_s(ctx, case, fused):
    got, _ = fused
    plain = ctx.align_pairs_blocks(case["pairs"], 11, case["segs"], case["sop"], tables=True, stats=True, **ic.PLANTED_BLOCKS)
    for f in BLOCK_KEYS:
        assert np.asarray(got[f]).tobytes() == np.asarray(plain[f]).tobytes(), f
    for f in ("blocks", "rows"):
        assert len(got[f]) == len(plain[f]) and all(a.tobytes() == b.tobytes() for a, b in zip(got[f], plain[f])), f


@pytest.mark.gpu
def test_against_the_stand_alone_call_on_host_planes(ctx, case, fused):
    got, opss = fused
    T, reads, n = case["T"], case["reads"], case["n"]
    base, slots, ilen, qpos = _planes(T, reads, opss)
    group, ng = got["reads"]["group"].tolist(), [int(got["seg"]["n_groups"][0])]
    seqs, quals, recs = ctx.planes_correct_groups([T], case["sop"], group, ng, [p[0] for p in case["pairs"]], base, slots, ilen, qpos, **ic.PLANTED_RULE)
    assert got["seq"] == seqs and got["qual"] == quals
    assert got["correct"].dtype == api.ISO_CORRECT_STATS_DTYPE and got["correct"].tobytes() == recs.tobytes()
    # ... and both against the definition restated in Python
    want = ic.py_correct_groups([T], case["sop"], group, ng, reads, base, slots, ilen, qpos, **ic.PLANTED_RULE)
    assert seqs == want[0] and quals == want[1] and ic.stats_dicts(recs) == want[2]


@pytest.mark.gpu
def test_the_planted_case(ctx, case, fused):
    """the minority keeps lacking its exon, the carriers keep theirs with their flanks corrected, and the corrected reads are no
    further from what they were read from than under ioc_align_pairs_correct's rule"""
    got, opss = fused
    T, reads, n = case["T"], case["reads"], case["n"]
    assert got["reads"]["group"].tolist() == [0] * N_MAJOR + [1] * N_MINOR + [0] * N_CARRY and not got["correct"]["flags"].any()
    assert got["correct"]["table"].tolist() == [0] * N_MAJOR + [1] * N_MINOR + [0] * N_CARRY
    ctx.align_set_pool(case["seqs"])
    old = ctx.align_pairs_correct(case["pairs"], 11, case["segs"], case["sop"], **ic.PLANTED_RULE)
    for i in MINOR:
        assert _nearer_to_the_representative(case, opss, i, old["seq"][i]) and not _nearer_to_the_representative(case, opss, i, got["seq"][i])
    d_raw = [pc.distance(r, t) for r, t in zip(reads, case["truths"])]
    d_old, d_new = _distances(case, opss, old["seq"]), _distances(case, opss, got["seq"])
    print("summed distance to the truth: ioc_align_pairs_correct", sum(d_old), "ioc_align_pairs_blocks_correct", sum(d_new), "uncorrected", sum(d_raw))
    assert sum(d_new) <= sum(d_old)
    base, slots, ilen, qpos = _planes(T, reads, opss)
    for i in CARRY:   # the exon as the read has it, at quality 0, and the rest of the read corrected
        rec = got["correct"][i]
        p = int(np.argmax(ilen[i]))
        run = reads[i][int(qpos[i][p]):int(qpos[i][p]) + int(ilen[i][p])]
        assert int(ilen[i][p]) > 20 and rec["n_long_runs"] >= 1 and rec["n_long_bases"] >= len(run)
        at = got["seq"][i].find(run)
        assert at >= 0 and got["qual"][i][at:at + len(run)] == b"!" * len(run)
        assert d_new[i] < d_raw[i] and d_new[i] <= 6
        assert d_old[i] >= 30   # (today's rule cuts the exon to the six bases the slot planes hold)


@pytest.mark.gpu
def test_the_refusals_write_nothing(ctx, case):
    ctx.align_set_pool(case["seqs"])
    bound = sum(api.pileup_call_bound(len(case["T"])) + len(r) for r in case["reads"])
    for bad, code in ((dict(correct_cap=bound - 1), -4), (dict(correct_min_depth=0), -1), (dict(correct_max_run=65), -1), (dict(min_gap=0), -1)):
        with pytest.raises(api.IocError) as e:
            ctx.align_pairs_blocks_correct(case["pairs"], 11, case["segs"], case["sop"], **{**CORRECT, **ic.PLANTED_BLOCKS, **bad})
        assert e.value.code == code, bad
    ok = ctx.align_pairs_blocks_correct(case["pairs"], 11, case["segs"], case["sop"], correct_cap=bound, **CORRECT, **ic.PLANTED_BLOCKS)
    assert sum(len(s) for s in ok["seq"]) <= bound
    empty = ctx.align_pairs_blocks_correct([], 11, [], [], **CORRECT)
    assert empty["seq"] == [] and len(empty["correct"]) == 0
