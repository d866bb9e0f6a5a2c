"""CPU-only checks of ioc_host_read_correct, the definition k_read_correct is tested against: against tables and planes spelled
out by hand, against the plain-Python restatement of tests/correct_common.py on inputs no aligner would produce, its refusals, and
the property the rule exists for on two haplotypes and an isoform that lacks 40 bases."""
import numpy as np
import pytest

from isonclust2_amd import api
from tests import correct_common as cc
from tests import polish_common as pc
from tests import sites_common as sc


@pytest.mark.parametrize("case", cc.HAND, ids=[c[0] for c in cc.HAND])
def test_hand_tables(case):
    frame, base, slots, cols, ins, rule, seq, qual, st = cc.hand_case(case)
    assert cc.py_correct(base, slots, cols, ins, frame, **rule) == (seq, qual, st)  # (the witness itself, against the hand)
    assert api.read_correct(base, slots, cols, ins, frame, **rule) == (seq, qual, st)


@pytest.mark.parametrize("max_run", [0, 1, 9, 10, 63, 64])
@pytest.mark.parametrize("kind", ["fill", "remove"])
def test_runs_at_and_above_max_run(kind, max_run):
    """Runs of exactly max_run and of max_run + 1 rows between two rows that are kept, max_run 0 and 64 included."""
    for run in (max_run, max_run + 1):
        rlen = run + 2
        frame = b"A" * rlen
        base = np.array([0] + [cc.DEL if kind == "fill" else 1] * run + [0, cc.NONE], np.uint8)
        cols = pc.table([cc.A10] + [cc.A10 if kind == "fill" else (0, 1, 0, 0, 0, 9)] * run + [cc.A10, cc.Z])
        ins = pc.ins_table(rlen + 1, {})
        seq, qual, st = api.read_correct(base, cc.slots_of(rlen + 1), cols, ins, frame, min_depth=3, min_alt=3, min_pct=25, max_run=max_run)
        applied = run <= max_run
        assert st["n_guarded"] == (0 if applied else run) and st["n_" + kind] == (run if applied else 0)
        assert seq == (b"A" * (rlen if kind == "fill" else 2) if applied else b"A" + (b"" if kind == "fill" else b"C" * run) + b"A")
        assert (seq, qual, st) == cc.py_correct(base, cc.slots_of(rlen + 1), cols, ins, frame, 3, 3, 25, max_run)


def test_refusals_write_nothing():
    frame, base, slots, cols, ins, rule, *_ = cc.hand_case(cc.HAND[0])
    L = api._lib.load()
    import ctypes as C
    for bad in (dict(min_depth=0), dict(min_alt=0), dict(min_pct=0), dict(min_pct=51), dict(max_run=-1), dict(max_run=65)):
        with pytest.raises(api.IocError) as e:
            api.read_correct(base, slots, cols, ins, frame, **{**rule, **bad})
        assert e.value.code == -1  # IOC_ERR_ARG
    with pytest.raises(api.IocError) as e:
        api.read_correct(base, slots, cols, ins, frame, cap=api.pileup_call_bound(1) - 1, **rule)
    assert e.value.code == -4  # IOC_ERR_CAPACITY
    seq, qual, st = C.create_string_buffer(b"\xEE" * 16, 16), C.create_string_buffer(b"\xEE" * 16, 16), api._lib.CorrectStats(*([-7] * 8))
    args = (base.ctypes.data, slots.ctypes.data, 1, cols.ctypes.data, ins.ctypes.data, frame)
    assert L.ioc_host_read_correct(*args, 3, 3, 25, 65, seq, qual, 16, C.byref(st)) == -1
    assert L.ioc_host_read_correct(*args, 3, 3, 25, 10, seq, qual, 6, C.byref(st)) == -4
    assert L.ioc_host_read_correct(*args, 3, 3, 25, 10, None, qual, 16, C.byref(st)) == -1
    assert L.ioc_host_read_correct(None, *args[1:], 3, 3, 25, 10, seq, qual, 16, C.byref(st)) == -1
    assert L.ioc_host_read_correct(*args[:2], -1, *args[3:], 3, 3, 25, 10, seq, qual, 16, C.byref(st)) == -1
    assert seq.raw == b"\xEE" * 16 and qual.raw == b"\xEE" * 16 and all(getattr(st, f) == -7 for f in cc.FIELDS)
    assert L.ioc_host_read_correct(*args, 3, 3, 25, 10, seq, qual, 16, None) == 1  # (the record is optional)


def test_random_inputs_against_the_restatement():
    """200 cases no aligner would produce; between them every counter of the record is exercised and runs of both kinds are longer
    than 64 rows."""
    rng = np.random.default_rng(20)
    seen, longest = dict.fromkeys(cc.FIELDS, 0), {"fill": 0, "remove": 0}
    for t in range(200):
        rlen = int(rng.integers(0, 200))
        frame, base, slots, cols, ins = cc.random_case(rng, rlen)
        rule = dict(min_depth=int(rng.integers(1, 5)), min_alt=int(rng.integers(1, 5)), min_pct=int(rng.integers(1, 51)),
                    max_run=int(rng.choice([0, 1, 2, 3, 10, 64])))
        got = api.read_correct(base, slots, cols, ins, frame, **rule)
        assert got == cc.py_correct(base, slots, cols, ins, frame, **rule), (t, rlen, rule)
        assert len(got[0]) == len(got[1]) == got[2]["out_len"] <= api.pileup_call_bound(rlen)
        for f in cc.FIELDS:
            seen[f] += got[2][f]
        dec = cc.py_decisions(base, cols, frame, rule["min_depth"], rule["min_alt"], rule["min_pct"])
        for kind in longest:
            longest[kind] = max([longest[kind]] + [n for _, n in cc.runs(dec, kind)])
    assert all(seen.values()), seen
    assert min(longest.values()) > 64, longest   # (runs of either kind that cross the 64-row steps)


def test_counters_near_2_32():
    rng = np.random.default_rng(21)
    for t in range(20):
        frame, base, slots, cols, ins = cc.random_case(rng, 40, values=(0, 1, 3, 2**31, pc.M32))
        assert api.read_correct(base, slots, cols, ins, frame) == cc.py_correct(base, slots, cols, ins, frame)


def test_haplotypes_and_an_isoform_keep_what_is_theirs():
    """20 noisy reads of T, 15 of its haplotype B and 2 of an isoform without T[150:190] (seed cc.SEED = 1638, 8 % errors), aligned
    against T by the host aligner and corrected by the host definition at the default rule.  Summed edit distance of the aligned
    parts of the reads to what they were mutated from: 784 before, 7 after (87 with max_run 64, which fills the isoform's exon
    in).  Every B read shows B's allele at every site of SITES_ON_T before the correction (what the seed was chosen for) and
    after it; both isoform reads hold 40 rows back."""
    T, reads, truths = cc.isoform_case(cc.SEED)
    B = sc.haplotypes()[1]
    seqs, quals, recs, (cols, ins, bases, slots, ops) = cc.host_correct_all(T, reads)
    before = sum(pc.distance(cc.aligned_part(r, o), tr) for r, o, tr in zip(reads, ops, truths))
    after = sum(pc.distance(s, tr) for s, tr in zip(seqs, truths))
    print(f"summed edit distance: {before} before, {after} after")
    assert after < before
    assert (before, after) == (784, 7)
    for i in range(20, 35):
        assert cc.shows_b_alleles(reads[i], T, B), i   # (the seed's choice)
        assert cc.shows_b_alleles(seqs[i], T, B), i
    assert not any(cc.shows_b_alleles(seqs[i], T, B) for i in range(20))   # (and no read of T was pulled over)
    gap = cc.CUT[1] - cc.CUT[0]
    long_seqs, _, long_recs, _ = cc.host_correct_all(T, reads, max_run=64)
    for i in (35, 36):
        assert recs[i]["n_guarded"] >= gap, recs[i]
        assert pc.distance(seqs[i], truths[i]) < pc.distance(cc.aligned_part(reads[i], ops[i]), truths[i])
        assert len(long_seqs[i]) > len(seqs[i]) and long_recs[i]["n_fill"] >= gap
    assert sum(pc.distance(s, tr) for s, tr in zip(long_seqs, truths)) == 87


def test_the_planted_case_has_the_runs_it_claims():
    """The shapes of tests/test_gpu_planes_correct.py, measured on the restatement so that they cannot decay unnoticed: of "fill"
    and of "remove" alike there are maximal runs of exactly 10, 11, 64, 65 and 130 rows, runs that start at rows 0, 62, 63, 64 and
    127, a run that ends at row rlen - 1, and a run that covers a whole step of 64 rows and reaches into both its neighbours."""
    case = cc.planted_case()
    for kind in ("fill", "remove"):
        found = cc.planted_runs(case, kind)
        assert cc.RUN_LENGTHS <= {n for _, _, n in found}, kind
        assert cc.RUN_STARTS <= {a for _, a, _ in found}, kind
        assert any(a + n == rlen for rlen, a, n in found), kind
        assert any(a < 64 * c and a + n > 64 * (c + 1) for _, a, n in found for c in range(1, 9)), kind
