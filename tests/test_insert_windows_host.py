"""The sequence of an inserted exon, on the host alone: ioc_host_ops_project_qpos, ioc_host_align_global_ops and
ioc_host_insert_windows against the plain-Python restatements of windows_common, and the property case — the consensus of the
carriers' windows at both sites of representative A through the host aligner, the host projections and the definitions."""
import numpy as np
import pytest

from isonclust2_amd import api
from tests import inserts_common as ic
from tests import windows_common as wc

# three of the scoring sets of test_align_params_host.py as (match, mismatch, gap): tie-rich, tie-rich with odd and even scores, and a
# negative match
PARAMS = [(2, -2, 2), (1, -1, 1), (5, -4, 2), (-7, -8, 1)]


def _rand(rng, n):
    return bytes(b"ACGT"[x] for x in rng.integers(0, 4, n))


def _mutate(rng, s, rate):
    out = bytearray()
    for c in s:
        u = rng.random()
        if u < rate / 3:
            continue
        out.append(b"ACGT"[int(rng.integers(0, 4))] if u < 2 * rate / 3 else c)
        if u > 1 - rate / 3:
            out.append(b"ACGT"[int(rng.integers(0, 4))])
    return bytes(out)


QPOS_CASES = [
    (b"", 0), (b"====", 4), (b"ii==dd", 4), (b"dd==ii", 4), (b"i" * 5, 0), (b"d" * 5, 5), (b"D" * 7, 7), (b"III==", 2), (b"==III", 2),
    (b"=" * 10 + b"I" * 300 + b"=" * 10, 20), (b"iiIII=X=DD=III" + b"i" * 4, 6), (b"I" * 300, 0), (b"dI=Id", 3), (b"=iD", 2),
]


@pytest.mark.parametrize("ops,rlen", QPOS_CASES)
def test_the_position_plane_of_chosen_strings(ops, rlen):
    got, want = api.ops_project_qpos(ops, rlen), wc.py_qpos(ops, rlen)
    assert got.dtype == np.uint32 and got.tobytes() == want.tobytes(), (ops, got, want)
    assert got[0] == 0 and (np.diff(got.astype(np.int64)) >= 0).all()


def test_the_position_plane_of_random_strings_and_where_a_run_begins():
    rng = np.random.default_rng(3)
    for _ in range(300):
        n = int(rng.integers(0, 400))
        body = bytes(rng.choice(np.frombuffer(b"=XID", np.uint8), n, p=[.7, .1, .12, .08]))
        ops = b"i" * int(rng.integers(0, 4)) + b"d" * int(rng.integers(0, 3)) + body + b"d" * int(rng.integers(0, 3)) + b"i" * int(rng.integers(0, 4))
        rlen = sum(o in b"=XDd" for o in ops)
        got = api.ops_project_qpos(ops, rlen)
        assert got.tobytes() == wc.py_qpos(ops, rlen).tobytes(), ops
        q = r = 0
        for a, o in enumerate(ops):   # the run of 'I' in front of row r begins at query[qpos[r]]
            if o == 73 and (a == 0 or ops[a - 1] != 73) and r > 0:
                assert int(got[r]) == q, (ops, r)
            q += o in b"=XIi"
            r += o in b"=XDd"


def test_the_position_plane_refuses_what_the_length_plane_refuses():
    for ops, rlen in ((b"==Z=", 3), (b"===", 2), (b"===", 4), (b"=\0=", 2), (b"DD", 1)):
        assert wc.py_qpos(ops, rlen) is None
        with pytest.raises(ValueError):
            api.ops_project_qpos(ops, rlen)
        with pytest.raises(ValueError):
            api.ops_project_ilen(ops, rlen)
    L = api._lib.load()
    plane = np.full(4, 0xA5A5A5A5, np.uint32)
    assert L.ioc_host_ops_project_qpos(b"==", -1, 2, plane.ctypes.data) == -1 and L.ioc_host_ops_project_qpos(b"==", 2, -1, plane.ctypes.data) == -1
    assert L.ioc_host_ops_project_qpos(b"==", 2, 2, None) == -1 and L.ioc_host_ops_project_qpos(b"=Z", 2, 2, plane.ctypes.data) == -1
    assert (plane == 0xA5A5A5A5).all()   # nothing was written


def _same_alignment(q, r, match, mismatch, gap):
    got, score = api.align_global_ops(q, r, match, mismatch, gap)
    want, wscore = wc.py_global(q, r, match, mismatch, gap)
    assert (got, score) == (want, wscore), (q, r, got, want)
    assert score == wc.ops_score(got, match, mismatch, gap)
    assert sum(o in b"=XI" for o in got) == len(q) and sum(o in b"=XD" for o in got) == len(r)
    return got


@pytest.mark.parametrize("match,mismatch,gap", PARAMS)
def test_the_global_alignment_of_chosen_strings(match, mismatch, gap):
    rng = np.random.default_rng(5)
    one, long = b"G", _rand(rng, 200)
    for q, r in ((b"", b""), (b"", b"ACGT"), (b"ACGT", b""), (one, long), (long, one), (long, long), (b"AAAA", b"AAA"), (b"AAA", b"AAAA"), (b"ACGT", b"TGCA")):
        _same_alignment(q, r, match, mismatch, gap)
    if match > 0:   # (under a negative match two gaps beat a match: identical strings are not all '=' there)
        assert api.align_global_ops(long, long, match, mismatch, gap)[0] == b"=" * 200


def test_the_tie_order_is_pinned():
    # one base too many on either side: every place of the gap scores the same; the walk back prefers the diagonal, so the gap
    # stands at the front
    assert api.align_global_ops(b"AAAA", b"AAA") == (b"I===", 4) and api.align_global_ops(b"AAA", b"AAAA") == (b"D===", 4)
    # 'D' before 'I' where both give the cell: the walk back meets 'D' first, so in forward order 'I' stands in front of 'D'
    assert api.align_global_ops(b"A", b"C", match=2, mismatch=-9, gap=1) == (b"ID", -2)


@pytest.mark.parametrize("match,mismatch,gap", PARAMS)
def test_the_global_alignment_of_random_pairs(match, mismatch, gap):
    rng = np.random.default_rng(17 + match)
    for _ in range(40):
        r = _rand(rng, int(rng.integers(1, 90)))
        _same_alignment(_mutate(rng, r, 0.08), r, match, mismatch, gap)


def test_the_global_alignment_refuses():
    for bad in (dict(gap=-1), dict(gap=(1 << 20) + 1), dict(match=(1 << 20) + 1), dict(mismatch=-(1 << 20) - 1)):
        with pytest.raises(api.IocError) as e:
            api.align_global_ops(b"ACGT", b"ACGT", **bad)
        assert e.value.code == -1, bad
    L = api._lib.load()
    ops = np.full(8, 0xA5, np.uint8)
    assert L.ioc_host_align_global_ops(b"ACGT", 4, b"ACGT", 4, 2, -2, 2, ops.ctypes.data, 7, None) == -4   # cap below qlen + rlen
    assert L.ioc_host_align_global_ops(b"ACGT", -1, b"ACGT", 4, 2, -2, 2, ops.ctypes.data, 8, None) == -1
    assert L.ioc_host_align_global_ops(None, 4, b"ACGT", 4, 2, -2, 2, ops.ctypes.data, 8, None) == -1
    assert (ops == 0xA5).all()


def test_window_bounds_voters_and_the_template():
    reads, base, qpos, sites, keys, extra = wc.planted_segment(max_win=40)
    qlen = [len(r) for r in reads]
    got = api.insert_windows(base, qpos, qlen, sites, keys, slack=8, max_win=40)
    want = wc.py_windows(base, qpos, qlen, sites, keys, 8, 40)
    for a, b in zip((got["win"], got["cls"], got["start"], got["len"]), want):
        assert a.tobytes() == b.tobytes()
    w = got["win"]
    assert (int(w[0]["lo"]), int(w[0]["hi"])) == (1, 11) and (int(w[2]["lo"]), int(w[2]["hi"])) == (190, 200)          # the clamps bite
    assert tuple(w[0][["template_pair", "tlen", "n_voters"]]) == (1, 15, 4)                                            # equal lengths, an even number: the index decides
    assert tuple(w[1][["template_pair", "tlen", "n_voters", "n_short", "n_long"]]) == (1, 25, 5, 1, 1)                 # 21 25 25 30 40: the lower median is read 1
    assert tuple(w[2][["template_pair", "tlen", "n_voters"]]) == (-1, 0, 0)                                            # no voter: not called
    assert got["cls"][:, 1].tolist() == [1, 1, 1, 1, 1, api.WIN_LONG, api.WIN_SHORT, api.WIN_NONE] and got["len"][4, 1] == 40
    for i in range(5):   # a voter's window is the insertion and its read's bases on the window rows
        s, n = int(got["start"][i, 1]), int(got["len"][i, 1])
        assert n == extra[i] and s == 92 + (5 if i < 4 else 0)   # (reads 0 .. 3 hold five inserted bases in front of row 2)
    wide = api.insert_windows(base, qpos, qlen, sites, keys, slack=8, max_win=41)
    assert int(wide["win"][1]["n_long"]) == 0 and int(wide["win"][1]["n_voters"]) == 6
    for slack in (0, 3, 32):
        g = api.insert_windows(base, qpos, qlen, sites, keys, slack=slack, max_win=100)
        for a, b in zip((g["win"], g["cls"], g["start"], g["len"]), wc.py_windows(base, qpos, qlen, sites, keys, slack, 100)):
            assert a.tobytes() == b.tobytes(), slack
    stolen = [10] + qlen[1:]   # a plane that is not this read's: the window leaves the read
    assert api.insert_windows(base, qpos, stolen, sites, keys, slack=8, max_win=40)["cls"][0].tolist() == [api.WIN_LONG, api.WIN_LONG, api.WIN_NONE]


def test_the_windows_refuse():
    reads, base, qpos, sites, keys, _ = wc.planted_segment()
    qlen = [len(r) for r in reads]
    bad_site = sites.copy()
    bad_site[2]["end"] = 201
    zero = sites.copy()
    zero[0]["first"] = 0
    for kw, st in ((dict(slack=-1), sites), (dict(slack=33), sites), (dict(max_win=0), sites), (dict(max_win=513), sites), ({}, bad_site), ({}, zero),
                   ({}, np.zeros(33, api.PILE_INSERT_DTYPE))):
        with pytest.raises(api.IocError) as e:
            api.insert_windows(base, qpos, qlen, st, keys, **kw)
        assert e.value.code == -1, kw
    none = api.insert_windows(base, qpos, qlen, sites[:0], keys)
    assert len(none["win"]) == 0


@pytest.fixture(scope="module")
def prop():
    return wc.host_property()


def test_the_consensus_of_a_site_holds_the_exon(prop):
    T, frame, reads, base, qpos, ins, got = prop
    assert all(ic.property_a_holds(ins)) and (wc.SEED, wc.SEEDS_TRIED) == (ic.SEED_A, ic.SEEDS_TRIED_A)
    dist = wc.distances(T, frame, got["win"], got["seq"])
    print("sites", ins["sites"], "windows", got["win"], "(to the true window, to the representative's rows, length)", dist)
    for k in range(2):
        assert dist[k][1] - dist[k][0] >= wc.MARGIN[k], (k, dist[k])   # nearer to the window with the exon by half the exon's length
        assert int(got["win"][k]["n_voters"]) == int(ins["sites"][k]["n_carry"]) and len(got["qual"][k]) == len(got["seq"][k])
    assert dist == wc.PINNED   # the host path's figures, pinned as equalities


def test_the_template_aligned_to_itself_is_all_matches(prop):
    _, _, reads, _, _, _, got = prop
    w = got["win"][0]
    t = reads[int(w["template_pair"])]
    assert api.align_global_ops(t[:int(w["tlen"])], t[:int(w["tlen"])])[0] == b"=" * int(w["tlen"])
