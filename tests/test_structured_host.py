"""Preconditions of the structured read sets (tests/structured_reads.CASES), checked on the CPU with the oracle alone: every
case really reaches the kernel path it is there for, so that tests/test_gpu_structured.py cannot quietly stop exercising it.
These are conditions, not measurements; the counts observed when the seeds were chosen stand next to each one.

The bound of totalMapped (tests/bound_common.py, restated from the header comment of ioc_resolve.hip) is checked against the
oracle's exact totals here: the formula itself; the device's arithmetic is compared with this restatement on the GPU."""
import functools

import numpy as np
import pytest

from isonclust2_amd import api
from tests import structured_reads as sr
from tests.bound_common import (MappedBound, in_walk_rejections, single_batch_cells, size_floor, slack_counts, strand_bound_terms,
                                 subset_view)
from tests.helpers import oracle_entry_assignments, oracle_sorted_batch, oracle_traced_run, walk_lengths

IOC_WALK_SLOTS, IOC_SCAN_ITEMS = 32, 256       # ioc_kernels.h


@functools.lru_cache(maxsize=None)
def traced(name):
    """the oracle's fast-mode run of a case with every entry traced (shared by the tests of this module; read only)"""
    rs = sr.case(name)
    return rs, oracle_traced_run(rs)


@functools.lru_cache(maxsize=None)
def merge_traced(name):
    """the oracle's `cluster -l -r` of a case cut into two batches, every right cluster traced (shared, read only): dict(obs, sbs,
    L, nR, rows, calls, left_rep, right_rep) — *_rep: the entry of its batch that represents every cluster (fast mode: its opener)"""
    from oracle import pyoracle as po
    from tests.test_gpu_merge import _batches
    obs, sbs = _batches(sr.case(name), 2)
    reps = []
    for B, sb in zip(obs, sbs):
        B.cluster(mode="fast")
        cls, orig, _, is_rep = B.members()
        at = {int(r): i for i, r in enumerate(sb.read_ids)}
        rep = np.full(B.n_clusters(), -1, np.int64)
        rep[cls[is_rep != 0]] = [at[int(o)] for o in orig[is_rep != 0]]
        reps.append(rep)
    L, nR = obs[0].n_clusters(), obs[1].n_clusters()
    po.trace_set(list(range(nR)), mapped_calls=True)
    try:
        obs[0].cluster(right=obs[1], mode="fast")
        rows, calls = po.trace_rows(), po.trace_mapped_calls()
    finally:
        po.trace_set(())
    return dict(obs=obs, sbs=sbs, L=L, nR=nR, rows=rows, calls=calls, left_rep=reps[0], right_rep=reps[1])


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_generator_is_deterministic_and_within_the_size_limits(name):
    a, b = sr.case(name), sr.case(name)
    assert a.seq.tobytes() == b.seq.tobytes() and a.qual.tobytes() == b.qual.tobytes()
    assert np.array_equal(a.offs, b.offs) and np.array_equal(a.transcript, b.transcript) and np.array_equal(a.strand, b.strand)
    other = sr.case(name, seed=sr.CASES[name]["seed"] + 1)
    assert other.seq.tobytes() != a.seq.tobytes()
    assert a.n <= 360 and int(np.diff(a.offs).max()) <= 900
    assert set(np.unique(a.seq).tolist()) <= set(b"ACGT")
    # the first pass: read i comes from transcript i
    g = int(a.transcript.max()) + 1
    assert np.array_equal(a.transcript[:min(g, a.n)], np.arange(min(g, a.n)))


def test_repeat_units_survive_homopolymer_compression():
    from oracle import pyoracle as po
    rng = np.random.default_rng(5)
    for period in (2, 3, 4, 5, 7, 12, 30, 257):
        u = sr.repeat_unit(rng, period)
        block = np.tile(u, 3).tobytes()
        assert len(u) == period and po.hpc(block, b"5" * len(block))[0] == block


def test_truncation_takes_a_prefix_suffix_or_infix_of_at_least_30_percent():
    rng = np.random.default_rng(9)
    src = np.arange(200, dtype=np.uint8)
    kinds = set()
    for _ in range(200):
        t = sr._truncate(rng, src)
        assert 60 <= len(t) <= 200 and np.array_equal(t, src[t[0]:t[0] + len(t)])
        kinds.add((t[0] == 0, t[-1] == 199))
    assert {(True, False), (False, True), (False, False)} <= kinds


def test_family44_walks_exceed_the_walk_slots():
    """observed (seed 1): 7 entries with more than 32 candidates in reach of the walk, the longest 44"""
    rs, run = traced("family44")
    walks = walk_lengths(run["rows"], rs.n)
    assert int((walks > IOC_WALK_SLOTS).sum()) >= 3, walks.max()


def test_family340_walks_exceed_the_scan_items():
    """observed (seed 1): 30 entries with more than 256 candidates in reach of the walk (306 with more than 32), the longest 299"""
    rs, run = traced("family340")
    walks = walk_lengths(run["rows"], rs.n)
    assert int((walks > IOC_SCAN_ITEMS).sum()) >= 10, walks.max()


def test_family_ties_long_walks_end_in_joins():
    """observed (seed 2): 46 entries with more than 32 candidates in reach of the walk, 37 of them with a passing candidate (up
    to 52 passing ones), 31 reads whose passing candidates tie at the winning Size — the long walks of family44 and family340
    all end in "nothing passes", which a scan of part of the list answers as well"""
    rs, run = traced("family_ties")
    rows, view = run["rows"], run["view"]
    walks = walk_lengths(rows, rs.n)
    need = np.array([api.host_min_total(int(h), 0.65) for h in view["hpc_len"]], np.int64)
    passing = np.bincount(rows["entry"][rows["total_mapped"] >= need[rows["entry"]]], minlength=rs.n)
    assert int(((walks > IOC_WALK_SLOTS) & (passing > 0)).sum()) >= 10
    assert int(((walks > IOC_WALK_SLOTS) & (passing > IOC_WALK_SLOTS)).sum()) >= 3      # (the winner may lie past the slots)
    assert run["stats"]["tie_reads"] >= 5


def test_bound_terms_by_hand():
    # positions 0 10 25 27 60, length 70; lim 2: the widest span of two steps is 25 -> 60, the head pos[1], the tail 70 - 27
    assert strand_bound_terms([0, 10, 25, 27, 60], 70, 2) == (35, 10 + 43)
    assert strand_bound_terms([0, 10, 25, 27, 60], 70, 1) == (33, 0 + 10)
    assert strand_bound_terms([0, 10, 25, 27, 60], 70, 9) == (60, 60 + 70)      # a limit beyond the list: all of it
    assert strand_bound_terms([0, 10, 25, 27, 60], 70, 0) == (0, 0)             # no gap passes at all
    assert strand_bound_terms([], 70, 3) == (0, 0)


# observed when the seeds were chosen: (rows, rows above the bound, rejected with bound >= 0.8 need, unrejected failing with
# bound < 1.25 need)
#   family44 (6967, 0, 17, 101)   isoforms_trunc (1850, 0, 43, 32)   repeat3 (2524, 0, 28, 34)   repeat2 (867, 0, 0, 0)
#   family_aln (2155, 0, 383, 200)   family340 (66400, 0, 5, 134)   family_ties (6949, 0, 553, 1650)
@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_bound_is_sound_and_decides_close_to_the_threshold(name):
    rs, run = traced(name)
    view = run["view"]
    bound = MappedBound(view, 11, 15, single_batch_cells(view, run["cls"]))
    n_rows, unsound, near_rejected, near_unrejected = slack_counts(bound, view, run["rows"])
    assert n_rows > 500
    assert unsound == 0                        # the formula: never below the oracle's exact totalMapped
    if name in ("family44", "isoforms_trunc", "repeat3"):
        assert near_rejected >= 5 and near_unrejected >= 5, (near_rejected, near_unrejected)


# The rows above are all trace rows.  The device consults the bound for fewer: the list cut (keep_q: the minimum over the 15
# target cells, test_list_cut_removes_candidates_the_size_rule_keeps below) and, in the sweeps, the candidates in reach of a walk
# that is not decided at its top Size.  Only the latter use the target's own error cell.  observed: family_aln 196,
# family_ties 63; family44, family340, isoforms_trunc, repeat2 and repeat3 0 (there the device's rejections are list cuts only)
@pytest.mark.parametrize("name", ["family_aln", "family_ties"])
def test_bound_rejects_inside_the_walk(name):
    rs, run = traced(name)
    view = run["view"]
    bound = MappedBound(view, 11, 15, single_batch_cells(view, run["cls"]))
    assert in_walk_rejections(bound, view, run["rows"], 11, 15) >= 20


def test_bound_rejects_left_targets_inside_the_walk_of_a_merge():
    """observed (family_aln in two batches, 26 left and 36 right clusters): 43 candidates with a LEFT target in reach of an
    undecided walk that the bound rejects — where the left clusters' error cells (left_err) decide on the device"""
    m = merge_traced("family_aln")
    rv = subset_view(m["sbs"][1].view, m["right_rep"])
    rows, L = m["rows"], m["L"]
    cells = np.ones(max(L, int(rows["cls"].max()) + 1), np.int64)
    cells[:L] = [api.host_err_cell(float(m["sbs"][0].view["hpc_err"][e])) for e in m["left_rep"]]
    bound = MappedBound(rv, 11, 15, cells)
    assert in_walk_rejections(bound, rv, rows, 11, 15, only=rows["cls"] < L) >= 10
    assert int((rows["cls"] < L).sum()) > 100 and int((rows["cls"] >= L).sum()) > 100


def test_truncated_reads_pass_the_threshold_below_the_size_rule():
    """observed (isoforms_trunc, seed 1): 2 candidates of Size < int(MinShared * MinFraction) = 4 whose exact totalMapped reaches
    the threshold (a read of a few dozen compressed bases: head + tail alone cover it), none of them walked — the rows for which
    compare_candidate_tables needs its size_cut; no other case has one"""
    _, run = traced("isoforms_trunc")
    rows, view = run["rows"], run["view"]
    need = np.array([api.host_min_total(int(h), 0.65) for h in view["hpc_len"]], np.int64)
    short = (rows["size"] < 4) & (rows["total_mapped"] >= need[rows["entry"]])
    assert int(short.sum()) >= 1 and not rows["walked"][short].any()


# observed: family44 5, family_aln 101, isoforms_trunc 7, repeat2 0, repeat3 0 (the shared block gives every candidate of a read
# that holds it a Size of 100 or more, and a read cut short of it has its few small candidates below the Size rule)
@pytest.mark.parametrize("name", ["family44", "family_aln", "isoforms_trunc"])
def test_list_cut_removes_candidates_the_size_rule_keeps(name):
    """the per-query cut of the candidate lists (k_gap_bounds' keep_q, restated in bound_common.size_floor) decides: some rows
    have int(MinShared * MinFraction) = 4 <= Size < the cut; none of them reaches the threshold on the oracle's exact total"""
    _, run = traced(name)
    rows, view = run["rows"], run["view"]
    need = [api.host_min_total(int(h), 0.65) for h in view["hpc_len"]]
    floor = np.array([size_floor(view, q, 11, 15, need[q], 4) for q in range(len(need))], np.int64)
    cut = (rows["size"] >= 4) & (rows["size"] < floor[rows["entry"]])
    assert int(cut.sum()) >= 3
    assert (rows["total_mapped"][cut] < np.array(need, np.int64)[rows["entry"][cut]]).all()


@pytest.mark.parametrize("name", ["repeat2", "repeat3"])
def test_repeat_reads_repeat_a_minimizer_value(name):
    """observed: repeat2 194 duplicate minimizer values in one read's list, repeat3 129"""
    _, run = traced(name)
    v = run["view"]
    most = 0
    for off in (v["off_fwd"], v["off_rev"]):
        for e in range(len(off) - 1):
            vals = v["min_val"][int(off[e]):int(off[e + 1])]
            most = max(most, len(vals) - len(np.unique(vals)))
    assert most >= 100, most


def test_family_aln_fallback_joins_and_refuses():
    """observed (seed 1): 58 clusters in fast mode, 18 in sahlin mode, 67 entries sent to the alignment fallback"""
    rs, run = traced("family_aln")
    fast = int(run["cls"].max()) + 1
    B, view = oracle_sorted_batch(rs)
    ocl, _, st = oracle_entry_assignments(B, view, mode="sahlin")
    sahlin = int(ocl.max()) + 1
    assert st["aln_invoked"] > 0
    assert fast - sahlin >= 5          # the fallback joins
    assert sahlin >= 6                 # and refuses: 24 transcripts do not collapse into a few clusters
    assert api.default_params(11, 15, "sahlin").aligned_threshold == 0.2


def test_fuzz_shapes_build_their_reads():
    """fuzz_cases.parity_reads: a case without a `shape` key is a `random` one (old reproducers replay the reads they always
    did), the draw of the shape leaves the generator it is handed alone, and every structured shape clusters on the oracle."""
    from isonclust2_amd import synth
    from tests import fuzz_cases as fz
    rng, twin = np.random.default_rng(77), np.random.default_rng(77)
    seen = set()
    for i in range(60):
        c = fz.draw_parity(rng, None if i % 4 else "sahlin")
        # the stream of draws is the one from before the key existed: the same calls on a twin generator stay in step
        n, g = int(twin.integers(1, 260)), int(twin.integers(1, 24))
        twin.choice([120, 200, 350, 600, 900, 1500, 2500]), twin.choice([7, 9, 11, 14]), twin.choice([4, 8, 12])
        twin.choice([0, 0, 2, 3]), twin.choice([0.0, 0.0, 0.3]), twin.integers(0, 5)
        assert int(twin.integers(0, 1 << 30)) == c["seed"] and g == c["g"] and (n == c["n"] or c["mode"] != "fast")
        if c["shape"] in seen or c["n"] < 20:
            continue
        seen.add(c["shape"])
        rs = fz.parity_reads(c)
        assert rs.n == c["n"] and rs.seq.tobytes() == fz.parity_reads(dict(c)).seq.tobytes()
        if c["shape"] == "random":
            old = {k: v for k, v in c.items() if k not in ("shape", "sargs")}
            ref = synth.generate(c["n"], c["g"], c["ln"], c["qlo"], c["qhi"], seed=c["seed"], dup_every=c["dup"], len_jitter=c["jit"])
            assert fz.parity_reads(old).seq.tobytes() == ref.seq.tobytes() == rs.seq.tobytes()
        else:
            B, view = oracle_sorted_batch(rs, c["k"], c["w"])
            ocl, _, _ = oracle_entry_assignments(B, view)
            assert int(ocl.max()) >= 0
    assert seen == {"random", "family", "isoforms", "repeat"}, seen
