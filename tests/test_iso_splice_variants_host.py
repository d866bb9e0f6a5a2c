"""The full-length sequence of an isoform by variant, on the host alone: ioc_host_isoform_splice_variants against the restatement of
splice_variants_common (py_splice_variants: ioc_host_isoform_splice's own restatement over the key with every 2 turned into 1, tlen
replaced and the chosen slot as the window), the planted cases where the choice of the slot bites, its refusals, what the functions
that existed still return, and the property case of variants_common carried on to the four isoforms' transcripts."""
import ctypes as C

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import iso_polish_common as ipc
from tests import polish_common as pc
from tests import splice_common as sc
from tests import splice_variants_common as svc
from tests import variants_common as vc

A, B, LACK, NONE = api.INS_CARRY, api.INS_CARRY_B, api.INS_LACK, api.INS_NONE


def _case(rng, rlen, values=(0, 1, 2, 3, 5)):
    cols, ins = pc.random_tables(rng, rlen + 1, values=values)
    return cols, ins, bytes(b"ACGTN"[x] for x in rng.integers(0, 5, rlen))


def test_the_symbols_and_the_record_sizes():
    L = _lib.load()
    for name in ("ioc_host_isoform_splice_variants", "ioc_planes_isoforms_full_variants", "ioc_align_pairs_isoforms_full_variants"):
        assert hasattr(L, name), name
    assert api.WINDOW_VARIANT_DTYPE.itemsize == 32 and api.INSERT_WINDOW_DTYPE.itemsize == 32
    assert api.SPLICE_SITE_DTYPE.itemsize == 16 and api.SPLICE_STATS_DTYPE.itemsize == 32 == C.sizeof(_lib.SpliceStats)
    assert (A, B) == (1, 2) and api.READ_VARIANTS_DTYPE.itemsize == 16


@pytest.mark.parametrize("rlen", [2, 63, 64, 65, 300])
def test_random_tables_and_plans_against_the_restatement(rlen):
    rng = np.random.default_rng(100 + rlen)
    states, picked = set(), set()
    for ns in (0, 1, 5, 32):
        for _ in range(12):
            cols, ins, frame = _case(rng, rlen)
            key, win, var, slots = svc.random_plan(rng, rlen, ns)
            md = int(rng.integers(1, 6))
            got = api.isoform_splice_variants(cols, ins, frame, key, win, var, slots, md)
            sc.same_splice(got, svc.py_splice_variants(cols, ins, frame, key, win, var, slots, md))
            assert (got[3]["reserved"] == 0).all()
            states |= set(got[3]["state"].tolist())
            picked |= {((key >> (2 * b)) & 3, int(var[b]["split"])) for b in range(ns) if int(got[3][b]["state"]) == sc.DONE}
    assert states == {sc.LACK, sc.DONE, sc.UNCALLED, sc.OVERLAP}
    # a DONE site took A, split or not, and B only where the site splits.  At rlen 2 every window is [1, 2): one site an isoform is
    # DONE, and the draws reach what they reach of the three
    every = {(A, 0), (A, 1), (B, 1)}
    assert picked <= every and len(picked) >= 1 and (rlen == 2 or picked == every)


def test_carry_b_at_a_site_that_did_not_split_is_uncalled():
    rng = np.random.default_rng(7)
    cols, ins, frame = _case(rng, 40)
    win, var = sc.windows([(5, 9), (20, 25)], tlen=[6, 6]), svc.variants([0, 1], [0, 4])
    slots = [(b"ACGT", b"IIII"), (b"", b""), (b"GG", b"II"), (b"TTT", b"III")]
    seq, qual, st, sites, ss = api.isoform_splice_variants(cols, ins, frame, sc.key_of([B, B]), win, var, slots, 2)
    assert sites["state"].tolist() == [sc.UNCALLED, sc.DONE] and ss == dict(n_done=1, n_uncalled=1, n_overlap=0, rows_replaced=5, spliced_bytes=3)
    assert seq[int(sites[1]["at"]):int(sites[1]["at"]) + 3] == b"TTT" and int(sites[1]["len"]) == 3 and int(sites[0]["at"]) == -1
    # a stray tlen_b where nothing split does not call the site either, and B bytes that stand there are not read
    var2, slots2 = svc.variants([0, 1], [9, 4]), [slots[0], (b"CC", b"II")] + slots[2:]
    assert api.isoform_splice_variants(cols, ins, frame, sc.key_of([B, B]), win, var2, slots2, 2)[0] == seq
    # a split site whose B template has no length: UNCALLED as a window with tlen 0 is
    assert api.isoform_splice_variants(cols, ins, frame, sc.key_of([B, B]), win, svc.variants([0, 1], [0, 0]), slots, 2)[3]["state"].tolist() == [sc.UNCALLED] * 2


def test_the_earlier_site_wins_across_variants():
    rng = np.random.default_rng(8)
    cols, ins, frame = _case(rng, 60)
    win, var = sc.windows([(10, 22), (20, 30), (30, 34)], tlen=[7, 7, 7]), svc.variants([1, 1, 0], [7, 7, 0])
    slots = [sc.random_string(rng, k) for k in (8, 40, 1, 8, 3, 0)]
    for k0 in (A, B):
        for k1 in (A, B):
            got = api.isoform_splice_variants(cols, ins, frame, sc.key_of([k0, k1, A]), win, var, slots, 2)
            sc.same_splice(got, svc.py_splice_variants(cols, ins, frame, sc.key_of([k0, k1, A]), win, var, slots, 2))
            assert got[3]["state"].tolist() == [sc.DONE, sc.OVERLAP, sc.DONE]   # lo and hi are the site's: either variant of site 0 shuts site 1 out
            assert int(got[3][0]["len"]) == (8 if k0 == A else 40)
    # where site 0 is not DONE, site 1 is, with the slot its own state takes
    got = api.isoform_splice_variants(cols, ins, frame, sc.key_of([LACK, B, A]), win, var, slots, 2)
    assert got[3]["state"].tolist() == [sc.LACK, sc.DONE, sc.DONE] and int(got[3][1]["len"]) == 8 and slots[3][0] in got[0]


def test_a_key_without_a_2_over_slots_that_hold_the_windows_is_the_parent_byte_for_byte():
    rng = np.random.default_rng(9)
    for _ in range(60):
        rlen, ns = int(rng.integers(2, 120)), int(rng.integers(0, 12))
        cols, ins, frame = _case(rng, rlen)
        key, win, var, slots = svc.random_plan(rng, rlen, ns)
        key = sc.key_of([s if s != B else (A, LACK, NONE)[b % 3] for b, s in enumerate((key >> (2 * b)) & 3 for b in range(ns))])
        sc.same_splice(api.isoform_splice_variants(cols, ins, frame, key, win, var, slots, 2), api.isoform_splice(cols, ins, frame, key, win, slots[0::2], 2))


def test_an_isoform_without_a_done_site_is_the_call():
    rng = np.random.default_rng(10)
    for t in range(60):
        rlen = int(rng.integers(2, 90))
        cols, ins, frame = _case(rng, rlen)
        key, win, var, slots = svc.random_plan(rng, rlen, int(rng.integers(0, 6)))
        if t % 3 == 0:
            key = sc.key_of([(LACK, NONE)[b % 2] for b in range(len(win))])    # no site carried
        elif t % 3 == 1:
            key, var = sc.key_of([B] * len(win)), svc.variants([0] * len(win))   # B claimed everywhere, nothing split
        else:
            win["tlen"], var["tlen_b"] = 0, 0                                    # none called
        seq, qual, st, sites, ss = api.isoform_splice_variants(cols, ins, frame, key, win, var, slots, 2)
        assert (seq, qual, st) == api.pileup_call(cols, ins, frame, 2)
        assert ss["n_done"] == ss["rows_replaced"] == ss["spliced_bytes"] == 0 and (sites["at"] == -1).all() and (sites["len"] == 0).all()
    empty = api.isoform_splice_variants(*_case(rng, 0), 6, sc.windows([]), svc.variants([]), [], 1)
    assert empty[:3] == (b"", b"", dict(out_len=0, n_sub=0, n_del=0, n_ins=0, n_low=0))


def _raw(cols, ins, frame, md, key, win, var, ns, sseq, squal, soff, cap, seq=True, sites=True):
    """the C function itself, every output filled with a mark first: (status, anything written)"""
    out_s, out_q = np.full(4096, 0xEE, np.uint8), np.full(4096, 0xEE, np.uint8)
    rec = np.full(40, -7, api.SPLICE_SITE_DTYPE)
    st, ss = _lib.PolishStats(), _lib.SpliceStats()
    st.out_len = ss.n_done = -7
    soff = np.asarray(soff, np.int64)
    rc = _lib.load().ioc_host_isoform_splice_variants(cols.ctypes.data if cols is not None else None, ins.ctypes.data if ins is not None else None, frame, len(frame), md,
                                                      key, win.ctypes.data if win is not None else None, var.ctypes.data if var is not None else None, ns, sseq, squal,
                                                      soff.ctypes.data, out_s.ctypes.data if seq else None, out_q.ctypes.data, cap, st,
                                                      rec.ctypes.data if sites else None, ss)
    written = (out_s != 0xEE).any() or (out_q != 0xEE).any() or (rec["state"] != -7).any() or st.out_len != -7 or ss.n_done != -7
    return rc, written


def test_refusals_write_nothing():
    rng = np.random.default_rng(6)
    cols, ins, frame = _case(rng, 30)
    win, var = sc.windows([(5, 9), (12, 20)]), svc.variants([1, 0])
    ok = dict(cols=cols, ins=ins, frame=frame, md=2, key=sc.key_of([B, A]), win=win, var=var, ns=2, sseq=b"ACGTACGT", squal=b"IIIIIIII", soff=[0, 2, 5, 8, 8],
              cap=api.isoform_splice_bound(30, 8))
    rc, written = _raw(**ok)
    assert rc > 0 and written   # (the call itself goes through)
    ARG, CAP = -1, -4
    bad = lambda **kw: _raw(**{**ok, **kw})
    # what ioc_host_isoform_splice refuses
    assert bad(md=0) == (ARG, False) and bad(cols=None) == (ARG, False) and bad(ins=None) == (ARG, False) and bad(seq=False) == (ARG, False)
    assert bad(ns=-1) == (ARG, False) and bad(ns=33) == (ARG, False) and bad(win=None) == (ARG, False) and bad(sites=False) == (ARG, False)
    for lo, hi in ((0, 4), (5, 5), (9, 5), (5, 31), (31, 32)):   # outside 1 <= lo < hi <= rlen
        assert bad(win=sc.windows([(lo, hi), (12, 20)])) == (ARG, False), (lo, hi)
    assert bad(win=sc.windows([(5, 9), (12, 20)], tlen=[1, -1])) == (ARG, False)
    assert bad(sseq=None) == (ARG, False) and bad(squal=None) == (ARG, False)
    # what is new: no variant records, a slot_off that does not ascend — at an A slot, at a B slot, at the last —, a split that is no flag, a negative tlen_b
    assert bad(var=None) == (ARG, False)
    for soff in ([3, 2, 5, 8, 8], [0, 6, 5, 8, 8], [0, 2, 9, 8, 8], [0, 2, 5, 8, 7]):
        assert bad(soff=soff) == (ARG, False), soff
    assert bad(var=svc.variants([2, 0], [1, 0])) == (ARG, False) and bad(var=svc.variants([-1, 0], [1, 0])) == (ARG, False)
    assert bad(var=svc.variants([1, 0], [-1, 0])) == (ARG, False) and bad(var=svc.variants([1, 0], [1, -1])) == (ARG, False)
    # capacity: the call's bound plus the bytes of ALL slots, whatever the key takes; exactly the bound goes through
    assert bad(cap=ok["cap"] - 1) == (CAP, False) and bad(cap=ok["cap"] - 1, key=0) == (CAP, False)
    assert bad(soff=[4, 5, 6, 7, 8], cap=api.pileup_call_bound(30) + 4)[0] > 0   # (slot_off need not begin at 0: the bound counts its span)
    assert bad(soff=[4, 5, 6, 7, 8], cap=api.pileup_call_bound(30) + 3) == (CAP, False)
    with pytest.raises(api.IocError):
        api.isoform_splice_variants(cols, ins, frame, 6, win, var, [(b"AC", b"II"), (b"ACG", b"III"), (b"ACG", b"III"), (b"", b"")], 2, cap=ok["cap"] - 1)
    assert len(api.isoform_splice_variants(cols, ins, frame, 6, win, var, [(b"AC", b"II"), (b"ACG", b"III"), (b"ACG", b"III"), (b"", b"")], 2, cap=ok["cap"])[0]) > 0


def test_the_functions_that_existed_return_what_they_returned():
    rng = np.random.default_rng(11)
    for _ in range(40):
        rlen, ns = int(rng.integers(2, 100)), int(rng.integers(1, 9))
        cols, ins, frame = _case(rng, rlen)
        key, win, ws = sc.random_plan(rng, rlen, ns)   # (draws state 2 as well)
        got = api.isoform_splice(cols, ins, frame, key, win, ws, 2)
        sc.same_splice(got, sc.py_splice(cols, ins, frame, key, win, ws, 2))
        assert all(int(got[3][b]["state"]) == sc.LACK for b in range(ns) if (key >> (2 * b)) & 3 == B)
    cols, ins, frame = _case(rng, 30)
    got = api.isoform_splice(cols, ins, frame, sc.key_of([B]), sc.windows([(5, 9)]), [(b"ACGT", b"IIII")], 2)
    assert got[3]["state"].tolist() == [sc.LACK] and got[:3] == api.pileup_call(cols, ins, frame, 2)


@pytest.fixture(scope="module")
def measured():
    return svc.host_measure()


def test_the_property_on_the_host_path(measured):
    case, iso, m = measured
    assert vc.SEED == 0 and len(case["reads"]) == sum(vc.SIZES)
    print(m)
    assert int(case["ins"]["seg"]["n_groups"]) == 3 and case["n_groups"] == 4   # three isoforms to the insert stage, four counted again
    four, nearer, gained, over_parent = svc.property_holds(m)
    assert four and nearer and gained and over_parent
    assert m == svc.PINNED
    # the states behind it: a DONE site is an exon the isoform carries, nothing overlaps, nothing stays uncalled, and the slot a site
    # took is the one its key2 names
    var = case["var"]
    slot_exon = vc.slot_exons(var, case["planted"])
    for (key2, _, x, _, _, _), ((seq, _, sites, ss), _, _) in zip(m, iso):
        assert int(ss["n_overlap"]) == int(ss["n_uncalled"]) == 0
        for b in range(len(sites)):
            s = (key2 >> (2 * b)) & 3
            assert (int(sites[b]["state"]) == sc.DONE) == (s in (A, B))
            if s in (A, B):
                at, n = int(sites[b]["at"]), int(sites[b]["len"])
                assert seq[at:at + n] == var["seq"][2 * b + (s == B)] and n > 0
        exon = lambda b: vc.EXONS[slot_exon[((key2 >> (2 * b)) & 3) == B]] if b == 0 else svc.SECOND   # (site 0: the planted exon its slot stands for)
        assert sum(exon(b) for b in range(len(sites)) if int(sites[b]["state"]) == sc.DONE) == svc.carried(x)


def test_the_parent_loses_the_exon_the_variant_splice_keeps(measured):
    case, iso, m = measured
    h = [x for x, r in enumerate(m) if r[0] & 3 == B]
    assert len(h) == 1
    key2, _, x, d, p, u = m[h[0]]
    assert p[x] - d[x] >= min(vc.EXONS) / 2 and p[x] >= min(vc.EXONS)   # the parent's sequence lacks the whole exon
    # ... and what the insert stage's three isoforms give under the parent's splice holds the 60-base exon's transcript nowhere
    ins, win = case["ins"], case["win"]
    keys = sc.group_keys(1, [0] * len(case["reads"]), ins["reads"], [3])
    full = sc.host_isoforms_full([case["frame"]], [0] * len(case["reads"]), ins["reads"]["group"].tolist(), [3], case["base"], case["slots"], keys, [win["win"]],
                                 [win["seq"]], [win["qual"]], 3)
    true = svc.true_transcripts()
    dist = [tuple(ipc.edit_distance(s, t) for t in true) for s in full["gseq"][0]]
    print(dist)
    assert dist == [(180, 165, 120, 0), (60, 45, 0, 120), (33, 4, 47, 167)]
    b_true = vc.slot_exons(case["var"], case["planted"])[1]   # the planted exon variant B stands for: the 60-base one
    assert vc.EXONS[b_true] == 60 and x == b_true
    assert min(d[b_true] for d in dist) >= min(vc.EXONS) / 2
