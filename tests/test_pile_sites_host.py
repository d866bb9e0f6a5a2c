"""The host definitions of the variable sites — ioc_host_ops_project, ioc_host_pileup_sites, ioc_host_site_alleles — against their
plain-Python restatements (tests/sites_common.py): tables worked out by hand, tables no aligner would produce, random strings;
that the projections of many reads sum to their pileup; the refusals; and the two-haplotype case, whose sites and allele vectors
are known in closed form, exact and under 8 % noise.  Bytes and integers only.  No GPU."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import polish_common as pc
from tests import sites_common as sc


@pytest.mark.parametrize("case", sc.HAND_SITES, ids=lambda c: c[0])
def test_hand_tables(case):
    name, rows, (md, ma, mp, mx), want, n_found = case
    cols = sc.table(rows)
    assert sc.py_sites(cols, md, ma, mp, mx) == (want, n_found), "the restatement itself"
    got, found = api.pileup_sites(cols, md, ma, mp, mx)
    assert (sc.as_tuples(got), found) == (want, n_found)


def test_random_tables_against_the_restatement():
    rng = np.random.default_rng(5)
    for trial in range(60):
        n_rows = int(rng.integers(1, 40))
        values = [(0, 1, 2, 3, 2**31, sc.M32), (0, 1, 2, 3, 4, 5, 6, 7), (0, 3, 10, 11, 40)][trial % 3]
        cols, _ = pc.random_tables(rng, n_rows, values=values)
        md, ma, mp = int(rng.integers(1, 12)), int(rng.integers(1, 6)), int(rng.choice([1, 10, 25, 33, 50]))
        for mx in (1, 3, 4096):
            got, found = api.pileup_sites(cols, md, ma, mp, mx)
            assert (sc.as_tuples(got), found) == sc.py_sites(cols, md, ma, mp, mx), (trial, mx)
    assert any(api.pileup_sites(pc.random_tables(rng, 30, values=(0, 3, 10, 11, 40))[0], 3, 3, 25)[1] > 5 for _ in range(3))


def test_hand_projection_and_alleles():
    ops, query, rlen, base, insf = sc.HAND_PROJECTION
    assert sc.py_project(ops, query, rlen) == (base, insf)
    b, i = api.ops_project(ops, query, rlen)
    assert (b.tolist(), i.tolist()) == (base, insf)
    sites = np.zeros(len(sc.HAND_ALLELES), api.PILE_SITE_DTYPE)
    for s, ((row, kind), _) in zip(sites, sc.HAND_ALLELES):
        s["row"], s["kind"] = row, kind
    want = [a for _, a in sc.HAND_ALLELES]
    assert sc.py_alleles(base, insf, [(r, k) for (r, k), _ in sc.HAND_ALLELES]) == want
    assert api.site_alleles(b, i, sites).tolist() == want
    # rlen 0: one row, nothing covered
    b0, i0 = api.ops_project(b"iI", b"AC", 0)
    assert (b0.tolist(), i0.tolist()) == ([sc.NONE], [1]) == sc.py_project(b"iI", b"AC", 0)
    s0 = np.zeros(1, api.PILE_SITE_DTYPE)
    s0["kind"] = sc.INS
    assert api.site_alleles(b0, i0, s0).tolist() == [sc.NONE]


def test_random_strings_and_the_sum_of_projections_is_the_pileup():
    rng = random.Random(9)
    for trial in range(40):
        # reads of one reference length: random bytes with the reference consumption fixed
        rlen = rng.randint(0, 60)
        cols = np.zeros(rlen + 1, api.PILEUP_DTYPE)
        summed = np.zeros((rlen + 1, 7), np.int64)
        projections = []
        for _ in range(rng.randint(1, 12)):
            ref_ops = [rng.choice(b"===XDd") for _ in range(rlen)]
            ops = bytearray()
            for op in ref_ops + [None]:
                ops += bytes([rng.choice(b"IIi")]) * rng.choice((0, 0, 0, 1, 2, 9))   # (one run in front of a row, as an aligner has it)
                if op is not None:
                    ops.append(op)
            ops = bytes(ops)
            query = bytes(rng.choice(b"ACGTACGTNn") for _ in range(sum(ops.count(c) for c in b"=XIi")))
            base, insf = api.ops_project(ops, query, rlen)
            assert (base.tolist(), insf.tolist()) == sc.py_project(ops, query, rlen)
            api.ops_pileup(ops, query, rlen, cols=cols)
            for ch in range(6):
                summed[:, ch] += base == ch
            summed[:, 6] += insf
            assert set(base.tolist()) <= {0, 1, 2, 3, 4, sc.DEL, sc.NONE} and set(insf.tolist()) <= {0, 1}
            projections.append((base, insf))
        for ch, f in enumerate(sc.COUNTERS + ("ins_runs",)):
            assert np.array_equal(summed[:, ch], cols[f]), (trial, f)
        sites, _ = api.pileup_sites(cols, 1, 1, 10)
        for base, insf in projections:
            assert api.site_alleles(base, insf, sites).tolist() == sc.py_alleles(base.tolist(), insf.tolist(), sc.as_tuples(sites))
    for trial in range(40):   # bytes in any order
        ops, query, rlen = sc.random_ops(rng, rng.randint(0, 300))
        base, insf = api.ops_project(ops, query, rlen)
        assert (base.tolist(), insf.tolist()) == sc.py_project(ops, query, rlen)


def test_refusals_leave_the_outputs_untouched():
    L = _lib.load()
    base, insf = np.full(8, 0xA5, np.uint8), np.full(8, 0xA5, np.uint8)
    def project(ops, query, rlen, n=None, b=base, i=insf):
        return L.ioc_host_ops_project(ops, len(ops) if n is None else n, query, len(query), rlen, b.ctypes.data if b is not None else None,
                                      i.ctypes.data if i is not None else None)
    assert project(b"==Z", b"ACG", 3) == -1                       # a byte that is no operation
    assert project(b"==\0", b"ACG", 3) == -1
    assert project(b"===", b"AC", 3) == -1 and project(b"===", b"ACG", 4) == -1 and project(b"==I", b"ACG", 3) == -1  # wrong consumption
    assert project(b"===", b"ACG", 3, n=2**31) == -1              # len >= 2^31 (refused before a byte is read)
    assert project(b"===", b"ACG", 3, n=-1) == -1 and project(b"===", b"ACG", -1) == -1
    assert project(b"===", b"ACG", 3, b=None) == -1 and project(b"===", b"ACG", 3, i=None) == -1
    assert (base == 0xA5).all() and (insf == 0xA5).all()
    assert project(b"===", b"ACG", 3) == 0 and base[:4].tolist() == [0, 1, 2, sc.NONE] and (base[4:] == 0xA5).all() and insf[:4].tolist() == [0] * 4
    with pytest.raises(ValueError):
        api.ops_project(b"=", b"AC", 1)

    cols = sc.table([(6, 4, 0, 0, 0, 0, 5), sc.Z])
    out, found = np.full(4 * 8, -9, np.int32), C.c_int64(-9)
    def sites(md=3, ma=3, mp=25, mx=4, rlen=1, c=cols, o=out):
        return L.ioc_host_pileup_sites(c.ctypes.data if c is not None else None, rlen, md, ma, mp, mx, o.ctypes.data if o is not None else None,
                                       C.byref(found))
    assert sites(md=0) == -1 and sites(ma=0) == -1 and sites(mp=0) == -1 and sites(mp=51) == -1 and sites(mx=0) == -1 and sites(rlen=-1) == -1
    assert sites(c=None) == -1 and sites(o=None) == -1
    assert (out == -9).all() and found.value == -9
    assert sites() == 2 and found.value == 2 and sites(mp=1) == 2 and sites(mp=50) == 1
    assert L.ioc_host_pileup_sites(cols.ctypes.data, 1, 3, 3, 25, 4, out.ctypes.data, None) == 2   # n_found may be NULL
    for bad in (dict(min_depth=0), dict(min_alt=0), dict(min_pct=0), dict(min_pct=51), dict(max_sites=0)):
        with pytest.raises(api.IocError) as e:
            api.pileup_sites(cols, **bad)
        assert e.value.code == -1

    b, i = api.ops_project(b"===", b"ACG", 3)
    alle = np.full(2, 0xA5, np.uint8)
    s = np.zeros(2, api.PILE_SITE_DTYPE)
    def alleles(rlen=3, n=2):
        return L.ioc_host_site_alleles(b.ctypes.data, i.ctypes.data, rlen, s.ctypes.data, n, alle.ctypes.data)
    s["row"] = [1, 4]
    assert alleles() == -1                                         # a row outside 0 .. rlen
    s["row"] = [1, -1]
    assert alleles() == -1
    s["row"], s["kind"] = [1, 3], [0, 0]
    assert alleles() == -1                                         # a base site at row rlen
    s["kind"] = [0, 2]
    assert alleles() == -1 and alleles(n=-1) == -1 and alleles(rlen=-1) == -1
    assert (alle == 0xA5).all()
    s["kind"] = [0, 1]
    assert alleles() == 0 and alle.tolist() == [1, 0]


def _check_haplotypes(frame, reads, n_first, want_sites, e):
    cols, sites, found, alleles = sc.host_sites_and_alleles(frame, reads, e=e)
    assert [(int(s["row"]), int(s["kind"])) for s in sites] == want_sites and found == len(want_sites)
    return sites, [a.tolist() for a in alleles]


@pytest.mark.parametrize("on", ["T", "B"])
def test_two_haplotypes_closed_form(on):
    """6 reads equal to T and 5 equal to B, piled on T and on B: exactly the substitution, the deleted rows and the insertion;
    the two groups have one allele vector each, and the two differ at every site."""
    T, B, reads = sc.haplotypes()
    assert len(B) == len(T) - 1 and sum(a != b for a, b in zip(T[:120], B[:120])) == 1
    sites, alleles = _check_haplotypes(T if on == "T" else B, reads, 6, sc.SITES_ON_T if on == "T" else sc.SITES_ON_B, 0.1)
    first, second = alleles[0], alleles[6]
    assert alleles[:6] == [first] * 6 and alleles[6:] == [second] * 5
    assert all(a != b for a, b in zip(first, second)) and sc.NONE not in first + second
    # the majority (6 reads) is the major allele everywhere, the 5 the minor
    assert first == [int(s["major"]) for s in sites] and second == [int(s["minor"]) for s in sites]
    assert all((int(s["depth"]), int(s["n_major"]), int(s["n_minor"])) == (11, 6, 5) for s in sites)
    if on == "T":
        assert second[1:4] == [sc.DEL] * 3 and (first[4], second[4]) == (0, 1) and first[0] == pc.CH[T[40]] and second[0] == pc.CH[B[40]]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_two_haplotypes_under_noise(seed):
    """20 + 15 reads mutated at 8 %, aligned with the gap open of e = 0.2, on T: the same five sites and no other."""
    T, reads = sc.noisy_haplotypes(seed)
    sites, alleles = _check_haplotypes(T, reads, 20, sc.SITES_ON_T, 0.2)
    # most reads of each group carry their haplotype's allele at the substitution
    sub = [a[0] for a in alleles]
    assert sum(a == int(sites["major"][0]) for a in sub[:20]) >= 15 and sum(a == int(sites["minor"][0]) for a in sub[20:]) >= 10
