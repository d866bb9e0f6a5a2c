"""CPU-only checks of ioc_host_read_correct_long, the definition the kernels of ioc_iso_correct.hip are tested against: the C
function against the plain-Python restatement (tests/iso_correct_common.py) on hand planes with long rows at the 64-row steps and
on random tables; with no long row it is ioc_host_read_correct, byte for byte; every way a pair is unresolved; every refusal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import correct_common as cc
from tests import iso_correct_common as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(got, want):
    assert got[0] == want[0] and got[1] == want[1]
    assert got[2] == want[2]


def test_the_symbols_and_the_record():
    txt = open(os.path.join(ROOT, "include", "isonclust2_hip.h")).read()
    L = _lib.load()
    for name in ("ioc_host_read_correct_long", "ioc_planes_correct_groups", "ioc_align_pairs_blocks_correct"):
        assert re.search(r"\b%s\s*\(" % name, txt) and hasattr(L, name) and name in _lib.SYMBOLS
    assert C.sizeof(_lib.IsoCorrectStats) == 48 and api.ISO_CORRECT_STATS_DTYPE.itemsize == 48
    assert api.ISO_CORRECT_STATS_FIELDS == ic.FIELDS
    assert re.search(r"#define\s+IOC_ISOC_UNRESOLVED\s+1\b", txt) and _lib.ISOC_UNRESOLVED == ic.UNRESOLVED == 1


@pytest.mark.parametrize("case", cc.HAND, ids=[c[0] for c in cc.HAND])
def test_without_a_long_row_it_is_read_correct_on_the_hand_cases(case):
    frame, base, slots, cols, ins, rule, seq, qual, st = cc.hand_case(case)
    rows = len(frame) + 1
    ilen = np.minimum((slots != 0).sum(axis=0), ic.SLOTS).astype(np.uint8)   # (what a run of at most six leaves in the length plane)
    qpos = np.arange(rows, dtype=np.uint32)
    got = api.read_correct_long(base, slots, ilen, qpos, cols, ins, frame, b"", **rule)
    assert (got[0], got[1]) == (seq, qual)
    assert {f: got[2][f] for f in cc.FIELDS} == st
    assert got[2]["table"] == got[2]["n_long_runs"] == got[2]["n_long_bases"] == got[2]["flags"] == 0
    _same(got, ic.py_correct_long(base, slots, ilen, qpos, cols, ins, frame, b"", **rule))


@pytest.mark.parametrize("rlen", [0, 1, 63, 64, 65, 130, 300])
def test_without_a_long_row_it_is_read_correct_on_random_tables(rlen):
    rng = np.random.default_rng(400 + rlen)
    for _ in range(6):
        frame, base, slots, cols, ins = cc.random_case(rng, rlen)
        ilen = rng.integers(0, ic.SLOTS + 1, rlen + 1).astype(np.uint8)   # (any value up to six: not a long row)
        qpos = rng.integers(0, 1000, rlen + 1).astype(np.uint32)
        rule = dict(min_depth=int(rng.integers(1, 5)), min_alt=int(rng.integers(1, 4)), min_pct=int(rng.integers(1, 51)), max_run=int(rng.integers(0, 65)))
        s, q, st = api.read_correct(base, slots, cols, ins, frame, **rule)
        got = api.read_correct_long(base, slots, ilen, qpos, cols, ins, frame, b"ACGT", **rule)
        assert (got[0], got[1]) == (s, q) and {f: got[2][f] for f in cc.FIELDS} == st
        _same(got, ic.py_correct_long(base, slots, ilen, qpos, cols, ins, frame, b"ACGT", **rule))
        assert ic.py_correct_long(base, slots, ilen, qpos, cols, ins, frame, b"ACGT", **rule)[:2] == cc.py_correct(base, slots, cols, ins, frame, **rule)[:2]


@pytest.mark.parametrize("case", ic.HAND_LONG, ids=[c[0] for c in ic.HAND_LONG])
def test_long_rows_at_the_steps(case):
    _, rlen, long_rows = case
    frame, base, slots, ilen, qpos, cols, ins, query, _ = ic.hand_read(rlen, long_rows, seed=rlen)
    got = api.read_correct_long(base, slots, ilen, qpos, cols, ins, frame, query)
    _same(got, ic.py_correct_long(base, slots, ilen, qpos, cols, ins, frame, query))
    kept = {p: n for p, n in long_rows.items() if n > ic.SLOTS}
    assert got[2]["n_long_runs"] == len(kept) and got[2]["n_long_bases"] == sum(kept.values()) and got[2]["flags"] == 0
    if len(kept) == len(long_rows):   # the read comes back as it is: its bases at 40, its runs at 0
        assert got[0] == query
        want_q = bytearray()
        for p in range(rlen + 1):
            want_q += b"!" * long_rows.get(p, 0) + (b"I" if p < rlen else b"")
        assert got[1] == bytes(want_q)
    else:   # a run of six is the slot rule's: nobody else has it, it is dropped
        assert got[2]["n_ins_drop"] == sum(n for n in long_rows.values() if n <= ic.SLOTS)


@pytest.mark.parametrize("rlen", [1, 64, 129, 260])
def test_long_rows_on_random_tables(rlen):
    """the long rows among everything else the rule does: a long row's base is decided, guarded and written like any other"""
    rng = np.random.default_rng(900 + rlen)
    resolved = 0
    for _ in range(8):
        frame, base, slots, cols, ins = cc.random_case(rng, rlen, p_bad=0.0)
        base[base == ic.NONE] = ic.DEL   # (spanned throughout: no long row is unresolved here)
        ilen = np.where(rng.random(rlen + 1) < 0.04, rng.integers(7, 255, rlen + 1), rng.integers(0, 7, rlen + 1)).astype(np.uint8)
        query = bytes(rng.choice(list(b"ACGTN"), 1800).tolist())   # (at 260 rows now and then shorter than the runs together)
        qpos = np.array([int(rng.integers(0, len(query) - int(n) + 1)) for n in ilen], np.uint32)
        rule = dict(min_depth=int(rng.integers(1, 5)), min_alt=int(rng.integers(1, 4)), min_pct=int(rng.integers(1, 51)), max_run=int(rng.integers(0, 65)))
        got = api.read_correct_long(base, slots, ilen, qpos, cols, ins, frame, query, **rule)
        _same(got, ic.py_correct_long(base, slots, ilen, qpos, cols, ins, frame, query, **rule))
        if got[2]["flags"] == 0:
            resolved += 1
            assert got[2]["n_long_runs"] == int((ilen > ic.SLOTS).sum()) and got[2]["n_long_bases"] == int(ilen[ilen > ic.SLOTS].sum())
        else:
            assert int(ilen[ilen > ic.SLOTS].sum()) > len(query)
    assert resolved >= 3


def test_every_unresolved_case():
    frame, base, slots, ilen, qpos, cols, ins, query, _ = ic.hand_read(130, {64: 20}, seed=3)
    empty = dict.fromkeys(ic.FIELDS, 0)
    empty["flags"] = ic.UNRESOLVED
    ok = api.read_correct_long(base, slots, ilen, qpos, cols, ins, frame, query)
    assert ok[0] == query and ok[2]["flags"] == 0
    # the plane's cap, at a long row and at any other
    for p in (64, 5, 130):
        capped = ilen.copy()
        capped[p] = 255
        assert api.read_correct_long(base, slots, capped, qpos, cols, ins, frame, query) == (b"", b"", empty)
        assert ic.py_correct_long(base, slots, capped, qpos, cols, ins, frame, query) == (b"", b"", empty)
    # a run that leaves the read: by one byte, and a position plane of another read
    assert api.read_correct_long(base, slots, ilen, qpos, cols, ins, frame, query[:int(qpos[64]) + 19]) == (b"", b"", empty)
    exact = api.read_correct_long(base, slots, ilen, qpos, cols, ins, frame, query[:int(qpos[64]) + 20])
    assert exact[2]["flags"] == 0 and exact[2]["n_long_bases"] == 20
    far = qpos.copy()
    far[64] = 2**32 - 1
    assert api.read_correct_long(base, slots, ilen, far, cols, ins, frame, query) == (b"", b"", empty)
    assert ic.py_correct_long(base, slots, ilen, far, cols, ins, frame, query) == (b"", b"", empty)
    # a long row the read does not span: its own row, and row rlen behind an uncovered last row
    gone = base.copy()
    gone[64] = ic.NONE
    assert api.read_correct_long(gone, slots, ilen, qpos, cols, ins, frame, query) == (b"", b"", empty)
    f2, b2, s2, l2, q2, c2, i2, query2, _ = ic.hand_read(64, {64: 9}, seed=4)
    assert api.read_correct_long(b2, s2, l2, q2, c2, i2, f2, query2)[2]["flags"] == 0
    b2[63] = ic.NONE
    assert api.read_correct_long(b2, s2, l2, q2, c2, i2, f2, query2) == (b"", b"", empty)
    assert ic.py_correct_long(b2, s2, l2, q2, c2, i2, f2, query2) == (b"", b"", empty)
    # runs that together are longer than the read: they overlap, and the bound on cap does not hold them
    f3, b3, s3, l3, q3, c3, i3, query3, _ = ic.hand_read(20, {4: 100, 9: 100}, seed=6)
    assert api.read_correct_long(b3, s3, l3, q3, c3, i3, f3, query3)[0] == query3
    short = query3[:199]
    q3[4], q3[9] = 0, 99
    assert api.read_correct_long(b3, s3, l3, q3, c3, i3, f3, short) == (b"", b"", empty)
    assert ic.py_correct_long(b3, s3, l3, q3, c3, i3, f3, short) == (b"", b"", empty)
    # rlen 0: row 0 is spanned by nothing
    z = api.read_correct_long(np.array([ic.NONE], np.uint8), np.zeros((6, 1), np.uint8), np.array([9], np.uint8), np.zeros(1, np.uint32),
                              np.zeros(1, api.PILEUP_DTYPE), np.zeros(1, api.PILEUP_INS_DTYPE), b"", b"ACGTACGTACGT")
    assert z == (b"", b"", empty)


def test_every_refusal():
    frame, base, slots, ilen, qpos, cols, ins, query, _ = ic.hand_read(10, {3: 8}, seed=5)
    for bad in (dict(min_depth=0), dict(min_alt=0), dict(min_pct=0), dict(min_pct=51), dict(max_run=-1), dict(max_run=65)):
        with pytest.raises(api.IocError) as e:
            api.read_correct_long(base, slots, ilen, qpos, cols, ins, frame, query, **bad)
        assert e.value.code == -1
    bound = api.read_correct_long_bound(10, len(query))
    assert bound == 10 + 6 * 11 + len(query)
    with pytest.raises(api.IocError) as e:
        api.read_correct_long(base, slots, ilen, qpos, cols, ins, frame, query, cap=bound - 1)
    assert e.value.code == -4  # IOC_ERR_CAPACITY
    assert api.read_correct_long(base, slots, ilen, qpos, cols, ins, frame, query, cap=bound)[0] == query
    # NULL arrays, a negative length: IOC_ERR_ARG, and nothing is written
    L = _lib.load()
    seq, qual, st = C.create_string_buffer(b"\x55" * bound, bound), C.create_string_buffer(b"\x55" * bound, bound), _lib.IsoCorrectStats()
    st.out_len = 77
    args = [base.ctypes.data, slots.ctypes.data, ilen.ctypes.data, qpos.ctypes.data, 10, cols.ctypes.data, ins.ctypes.data, frame, query, len(query), 3, 3, 25, 10,
            seq, qual, bound, C.byref(st)]
    for k in (0, 1, 2, 3, 5, 6, 7, 8, 14, 15):
        a = list(args)
        a[k] = None
        assert L.ioc_host_read_correct_long(*a) == -1, k
    for k, v in ((4, -1), (9, -1)):
        a = list(args)
        a[k] = v
        assert L.ioc_host_read_correct_long(*a) == -1
    a = list(args)
    a[16] = bound - 1
    assert L.ioc_host_read_correct_long(*a) == -4
    assert seq.raw == b"\x55" * bound and qual.raw == b"\x55" * bound and st.out_len == 77
    assert L.ioc_host_read_correct_long(*args) == len(query) and st.out_len == len(query)
