"""The full-length sequence of an isoform, on the host alone: ioc_host_isoform_splice against the plain-Python restatement of
splice_common (py_splice, built from a per-row restatement of the call), its refusals, the two identities that state the rule without
py_splice, and the property cases A and B through the host aligner, the host projections and the definitions."""
import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import polish_common as pc
from tests import splice_common as sc


def _case(rng, rlen, values=(0, 1, 2, 3, 5)):
    cols, ins = pc.random_tables(rng, rlen + 1, values=values)
    return cols, ins, bytes(b"ACGTN"[x] for x in rng.integers(0, 5, rlen))


def test_the_rows_of_py_row_add_up_to_the_call():
    rng = np.random.default_rng(5)
    for _ in range(40):
        cols, ins, frame = _case(rng, int(rng.integers(0, 70)), values=(0, 1, 2, 3, 2**31, pc.M32))
        md = int(rng.integers(1, 5))
        rows = [sc.py_row(cols, ins, frame, p, md) for p in range(len(frame) + 1)]
        seq, qual, st = pc.py_call(cols, ins, frame, md)
        assert (b"".join(r[0] for r in rows), b"".join(r[1] for r in rows)) == (seq, qual)
        assert all(sum(r[2][f] for r in rows) == st[f] for f in sc.STAT_KEYS)


def test_random_tables_and_plans_against_the_restatement():
    rng = np.random.default_rng(1)
    seen = set()
    for _ in range(300):
        rlen, ns = int(rng.integers(2, 120)), int(rng.integers(0, 12))
        cols, ins, frame = _case(rng, rlen)
        key, win, ws = sc.random_plan(rng, rlen, ns)
        md = int(rng.integers(1, 6))
        got = api.isoform_splice(cols, ins, frame, key, win, ws, md)
        sc.same_splice(got, sc.py_splice(cols, ins, frame, key, win, ws, md))
        seen |= set(got[3]["state"].tolist())
    assert seen == {sc.LACK, sc.DONE, sc.UNCALLED, sc.OVERLAP}


def test_thirty_two_sites_and_the_highest_bits_of_the_key():
    rng = np.random.default_rng(2)
    cols, ins, frame = _case(rng, 100)
    win = sc.windows([(1 + 3 * b, 4 + 3 * b) for b in range(32)])
    ws = [sc.random_string(rng, int(rng.integers(0, 9))) for _ in range(32)]
    for key in (sc.key_of([sc.CARRY] * 32), sc.key_of([api.INS_LACK] * 31 + [sc.CARRY]), sc.key_of([api.INS_NONE] * 31 + [sc.CARRY]), 2**64 - 1):
        got = api.isoform_splice(cols, ins, frame, key, win, ws, 2)
        sc.same_splice(got, sc.py_splice(cols, ins, frame, key, win, ws, 2))
    assert got[4]["n_done"] == 0 and api.isoform_splice(cols, ins, frame, sc.key_of([sc.CARRY] * 32), win, ws, 2)[4]["rows_replaced"] == 96


def test_an_isoform_without_a_done_site_is_the_call():
    rng = np.random.default_rng(3)
    for _ in range(60):
        rlen = int(rng.integers(2, 90))
        cols, ins, frame = _case(rng, rlen)
        key, win, ws = sc.random_plan(rng, rlen, int(rng.integers(0, 6)))
        if _ % 2:
            key = sc.key_of([(api.INS_LACK, api.INS_NONE, 2)[b % 3] for b in range(len(win))])   # no site carried
        else:
            win["tlen"] = 0                                                                       # none called
            ws = [(b"", b"")] * len(win)
        seq, qual, st, sites, ss = api.isoform_splice(cols, ins, frame, key, win, ws, 2)
        assert (seq, qual, st) == api.pileup_call(cols, ins, frame, 2)
        assert ss["n_done"] == ss["rows_replaced"] == ss["spliced_bytes"] == 0 and (sites["at"] == -1).all() and (sites["len"] == 0).all()
    assert api.isoform_splice(*_case(rng, 0), 5, sc.windows([]), [], 1)[:3] == (b"", b"", dict(out_len=0, n_sub=0, n_del=0, n_ins=0, n_low=0))


def _cut_call(cols, ins, frame, b, min_depth):
    """api.pileup_call over the rows [0, b) of the tables alone: the cut tables end with an empty row, which emits nothing"""
    c, i = np.zeros(b + 1, api.PILEUP_DTYPE), np.zeros(b + 1, api.PILEUP_INS_DTYPE)
    c[:b], i[:b] = cols[:b], ins[:b]
    return api.pileup_call(c, i, frame[:b], min_depth)


def test_a_done_site_is_the_call_of_the_rows_before_the_window_and_the_walk_from_hi():
    rng = np.random.default_rng(4)
    for _ in range(80):
        rlen = int(rng.integers(2, 120))
        cols, ins, frame = _case(rng, rlen)
        lo = int(rng.integers(1, rlen))
        hi = int(rng.integers(lo + 1, rlen + 1)) if _ % 4 else rlen
        w = sc.random_string(rng, int(rng.choice([0, 1, 8, 50])))
        seq, qual, st, sites, ss = api.isoform_splice(cols, ins, frame, sc.CARRY, sc.windows([(lo, hi)]), [w], 2)
        head = _cut_call(cols, ins, frame, lo, 2)
        whole = api.pileup_call(cols, ins, frame, 2)
        upto = _cut_call(cols, ins, frame, hi, 2)                  # rows [0, hi) without the insertions in front of hi ...
        rest = whole[0][len(upto[0]):], whole[1][len(upto[1]):]    # ... so what follows them in the whole call is the walk from hi on
        assert seq == head[0] + w[0] + rest[0] and qual == head[1] + w[1] + rest[1]
        assert int(sites[0]["at"]) == len(head[0]) and int(sites[0]["len"]) == len(w[0]) and int(sites[0]["state"]) == sc.DONE
        assert all(st[f] == head[2][f] + whole[2][f] - upto[2][f] for f in sc.STAT_KEYS) and st["out_len"] == len(seq)
        assert ss == dict(n_done=1, n_uncalled=0, n_overlap=0, rows_replaced=hi - lo, spliced_bytes=len(w[0]))


def _raw(cols, ins, frame, md, key, win, ns, wseq, wqual, woff, cap, seq=True, sites=True):
    """the C function itself, every output filled with a mark first: (status, anything written)"""
    out_s, out_q = np.full(4096, 0xEE, np.uint8), np.full(4096, 0xEE, np.uint8)
    rec = np.full(40, -7, api.SPLICE_SITE_DTYPE)
    st, ss = _lib.PolishStats(), _lib.SpliceStats()
    st.out_len = ss.n_done = -7
    woff = np.asarray(woff, np.int64)
    rc = _lib.load().ioc_host_isoform_splice(cols.ctypes.data if cols is not None else None, ins.ctypes.data if ins is not None else None, frame, len(frame), md, key,
                                             win.ctypes.data if win is not None else None, ns, wseq, wqual, woff.ctypes.data, out_s.ctypes.data if seq else None,
                                             out_q.ctypes.data, cap, st, rec.ctypes.data if sites else None, ss)
    written = (out_s != 0xEE).any() or (out_q != 0xEE).any() or (rec["state"] != -7).any() or st.out_len != -7 or ss.n_done != -7
    return rc, written


def test_refusals_write_nothing():
    rng = np.random.default_rng(6)
    cols, ins, frame = _case(rng, 30)
    win = sc.windows([(5, 9), (12, 20)])
    ok = dict(cols=cols, ins=ins, frame=frame, md=2, key=5, win=win, ns=2, wseq=b"ACGTAC", wqual=b"IIIIII", woff=[0, 2, 6], cap=api.isoform_splice_bound(30, 6))
    rc, written = _raw(**ok)
    assert rc > 0 and written   # (the call itself goes through)
    ARG, CAP = -1, -4
    bad = lambda **kw: _raw(**{**ok, **kw})
    # what the call refuses
    assert bad(md=0) == (ARG, False) and bad(cols=None) == (ARG, False) and bad(ins=None) == (ARG, False) and bad(seq=False) == (ARG, False)
    # what the windows' definition refuses about the count, and the records
    assert bad(ns=-1) == (ARG, False) and bad(ns=33) == (ARG, False) and bad(win=None) == (ARG, False) and bad(sites=False) == (ARG, False)
    for lo, hi in ((0, 4), (5, 5), (9, 5), (5, 31), (31, 32)):   # outside 1 <= lo < hi <= rlen
        assert bad(win=sc.windows([(lo, hi), (12, 20)])) == (ARG, False), (lo, hi)
    assert bad(win=sc.windows([(5, 9), (12, 20)], tlen=[1, -1])) == (ARG, False)
    assert bad(woff=[0, 7, 6]) == (ARG, False) and bad(woff=[3, 2, 6]) == (ARG, False)   # does not ascend
    assert bad(wseq=None) == (ARG, False) and bad(wqual=None) == (ARG, False)
    # capacity: the call's bound plus the windows' bytes, whatever the key carries
    assert bad(cap=ok["cap"] - 1) == (CAP, False) and bad(cap=ok["cap"] - 1, key=0) == (CAP, False)
    assert bad(woff=[4, 5, 6], cap=api.pileup_call_bound(30) + 2)[0] > 0   # (win_off need not begin at 0: the bound counts its span)
    with pytest.raises(api.IocError):
        api.isoform_splice(cols, ins, frame, 5, win, [(b"AC", b"II"), (b"ACGT", b"IIII")], 2, cap=ok["cap"] - 1)


@pytest.mark.parametrize("which", ["A", "B"])
def test_the_property_on_the_host_path(which):
    seed, tried, pinned = (sc.SEED_A, sc.SEEDS_TRIED_A, sc.PINNED_A) if which == "A" else (sc.SEED_B, sc.SEEDS_TRIED_B, sc.PINNED_B)
    assert tried == seed + 1 <= 6
    for s in range(seed):   # (no earlier seed holds: the seed is the first)
        assert not sc.property_holds(which, sc.host_measure(which, s)[2])
    case, iso, measured = sc.host_measure(which, seed)
    print(which, measured)
    assert sc.property_holds(which, measured)
    assert measured == pinned
    # the states behind it: an isoform's DONE sites are the exons it carries, nothing overlaps and nothing stays uncalled
    for (x, _, _), (_, _, sites, ss, _) in zip(measured, iso):
        assert int(ss["n_overlap"]) == int(ss["n_uncalled"]) == 0
        assert sum(sc.EXONS[which][b] for b in range(len(sites)) if int(sites[b]["state"]) == sc.DONE) == sc.carried(which, x)
