"""ioc_host_align_ops / ioc_host_ops_to_cigar: the host aligner returning the alignment itself — one operation byte per column
of the comparison string ('=' 'X' 'I' 'D', free end gaps 'i' 'd').  The string must be consistent with its sequences, re-score
to the score, and reduce to exactly what ioc_host_align and the oracle's aligner return as `comp`."""
import ctypes as C
import random
import re

import pytest

from isonclust2_amd import _lib, api
from oracle import pyoracle as po
from tests.align_ops_checks import check_ops, ops_to_comp

# an error sum for every class of setGapOpen (src/cluster.cpp:425-440): gap open 5, 4, 3, 2
E_OF_GAP_OPEN = {5: 0.005, 4: 0.03, 3: 0.08, 2: 0.2}


def _mutate(rng, s, rate):
    out = bytearray()
    for ch in s:
        x = rng.random()
        if x < rate / 3:
            out.append(rng.choice(b"ACGT"))
        elif x < 2 * rate / 3:
            continue
        elif x < rate:
            out.append(ch)
            out.append(rng.choice(b"ACGT"))
        else:
            out.append(ch)
    return bytes(out)


def _pairs():
    """A few hundred seeded pairs of 0 .. 400 bases."""
    rng = random.Random(20240)
    rnd = lambda n, alphabet=b"ACGT": bytes(rng.choice(alphabet) for _ in range(n))
    out = []
    for rate in (0.02, 0.1, 0.3):                        # mutated copies
        for _ in range(40):
            base = rnd(rng.randint(1, 400))
            out.append((_mutate(rng, base, rate)[:400], _mutate(rng, base, rate)[:400]))
    for _ in range(40):                                  # unrelated
        out.append((rnd(rng.randint(1, 400)), rnd(rng.randint(1, 400))))
    for _ in range(30):                                  # a read inside a longer reference, and the reverse
        base = rnd(rng.randint(120, 400))
        a = rng.randint(0, len(base) // 2)
        inner = _mutate(rng, base[a:a + rng.randint(20, len(base) // 2)], 0.08)
        out += [(inner, base), (base, inner)]
    for _ in range(40):                                  # overlapping ends
        base = rnd(rng.randint(100, 400))
        a, b = rng.randint(1, len(base) - 1), rng.randint(1, len(base) - 1)
        out.append((_mutate(rng, base[min(a, b):], 0.06), _mutate(rng, base[:max(a, b)], 0.06)))
    for n, m in ((0, 0), (0, 1), (1, 0), (0, 57), (57, 0), (1, 1), (3, 200), (200, 3), (10, 10), (5, 9)):   # empty, shorter than k
        out.append((rnd(n), rnd(m)))
    for _ in range(30):                                  # bytes other than A C G T
        base = rnd(rng.randint(30, 300), b"ACGTNacgt-*")
        out.append((_mutate(rng, base, 0.1), _mutate(rng, base, 0.1)))
    out.append((b"A" * 90, b"A" * 70))                   # ties everywhere
    out.append((b"AC" * 60, b"CA" * 61))
    return out


def _host_comp(L, q, r, go):
    comp, sc = C.create_string_buffer(len(q) + len(r) + 1), C.c_int32()
    n = L.ioc_host_align(q, len(q), r, len(r), 2, -2, go, 1, comp, len(q) + len(r) + 1, C.byref(sc))
    assert n >= 0
    return comp.raw[:n], sc.value


@pytest.mark.parametrize("gap_open", [2, 3, 4, 5])
def test_ops_are_consistent_rescore_and_reduce_to_comp(gap_open):
    """Checks 1 - 6 for every pair.  Check 4 (the string re-scores to the score) relies on gap open > gap extend, which every
    class of ioc_host_gap_open satisfies with gap extend 1: see check_ops."""
    L = _lib.load()
    e = E_OF_GAP_OPEN[gap_open]
    assert L.ioc_host_gap_open(e) == gap_open
    pairs = _pairs()
    assert len(pairs) >= 300
    for t, (q, r) in enumerate(pairs):
        ops, score = api.host_align_ops(q, r, gap_open=gap_open)
        check_ops(ops, q, r, score, gap_open, tag=(t, len(q), len(r)))                       # 1 - 4
        comp, hs = _host_comp(L, q, r, gap_open)                                             # 5
        assert ops_to_comp(ops) == comp == api.ops_to_comp(ops) and score == hs, t
        os_, ocomp, oratio = po.align(q, r, e, 11)
        assert comp == ocomp and score == os_, t
        assert L.ioc_host_aln_ratio(ops_to_comp(ops), len(ops), e, max(len(q), 1), 11) == L.ioc_host_aln_ratio(comp, len(comp), e, max(len(q), 1), 11)
        if len(q):
            assert L.ioc_host_aln_ratio(ops_to_comp(ops), len(ops), e, len(q), 11) == oratio, t
        cigar = api.ops_to_cigar(ops)                                                        # 6
        assert re.fullmatch(r"(\d+[=XIDid])*", cigar)
        back = b"".join(op.encode() * int(n) for n, op in re.findall(r"(\d+)([=XIDid])", cigar))
        assert back == ops, t
        assert not re.search(r"(\D)\d+\1", "#" + cigar), (t, "adjacent runs of one operation")


def test_reference_aln_ratio_vector(kat):
    """AlnRatioTest (test/isONclust2_test.cpp:137-181), through the operation string."""
    L = _lib.load()
    ref, read = kat["min_match"]["ref"].encode(), kat["min_match"]["read"].encode()
    e = po.error_rate(b"I" * len(ref), nomin=False) + po.error_rate(b"I" * len(read), nomin=False)
    go = L.ioc_host_gap_open(e)
    ops, score = api.host_align_ops(ref, read, gap_open=go)          # the test aligns (ref, read) in that order
    check_ops(ops, ref, read, score, go)
    comp, hs = _host_comp(L, ref, read, go)
    assert ops_to_comp(ops) == comp and score == hs
    ratio = L.ioc_host_aln_ratio(ops_to_comp(ops), len(ops), e, len(read), kat["aln_ratio"]["k"])
    assert abs(ratio - kat["aln_ratio"]["expected_double_eq"]) < 1e-15


def test_end_gap_order_and_letters():
    """Leading i, leading d, the walk, trailing i, trailing d; upper case inside the walk only."""
    assert api.host_align_ops(b"", b"")[0] == b""
    assert api.host_align_ops(b"ACG", b"")[0] == b"iii" and api.host_align_ops(b"", b"ACGT")[0] == b"dddd"
    ops, score = api.host_align_ops(b"ACGTACGTAC", b"TTTTTACGTACGTAC")                  # query = the reference's suffix
    assert ops == b"ddddd" + b"=" * 10 and score == 20
    ops, score = api.host_align_ops(b"GGGGACGTACGTAC", b"ACGTACGTACTTT")                # overlap: query tail on reference head
    assert ops == b"iiii" + b"=" * 10 + b"ddd" and score == 20
    ops, score = api.host_align_ops(b"ACGTACGTACGTACGTAAAACCCCGGGGTTTT", b"ACGTACGTACGTACGTCCCCGGGGTTTT", gap_open=3)
    assert ops == b"=" * 16 + b"IIII" + b"=" * 12 and score == 2 * 28 - (3 + 3)   # one gap of four: open + 3 x extend


def test_cigar_errors_and_capacity():
    L = _lib.load()
    assert api.ops_to_cigar(b"") == "" and api.ops_to_cigar(b"ii==X=IIDd") == "2i2=1X1=2I1D1d"
    with pytest.raises(ValueError):
        api.ops_to_cigar(b"==M=")
    out = C.create_string_buffer(4)
    assert L.ioc_host_ops_to_cigar(b"==X", 3, out, 4) == -4                                       # IOC_ERR_CAPACITY
    out = C.create_string_buffer(5)
    assert L.ioc_host_ops_to_cigar(b"==X", 3, out, 5) == 4 and out.value == b"2=1X"
    buf, sc = C.create_string_buffer(8), C.c_int32()
    assert L.ioc_host_align_ops(b"ACGT", 4, b"ACGT", 4, 2, -2, 3, 1, buf, 8, C.byref(sc)) < 0    # needs qlen + rlen + 1
