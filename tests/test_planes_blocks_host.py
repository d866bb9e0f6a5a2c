"""ioc_host_planes_blocks, the definition of the exon blocks of a cluster and every read's isoform: against a plain restatement in
Python (blocks_common.py_blocks) on the planted planes of the GPU test and on random planes, as bytes; what it refuses, and that a
refusal writes nothing; what the planted planes are there for, measured; and the property case through the host aligner and
ioc_host_ops_project alone."""
import ctypes as C

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import blocks_common as bc


@pytest.fixture(scope="module")
def planted():
    case = bc.planted_case()
    return case, bc.host_segments(case)


def _planes(rlen, p):
    return p if len(p) else np.zeros((0, rlen + 1), np.uint8)


@pytest.mark.parametrize("rule", [{}, bc.SECOND, dict(max_blocks=1)], ids=["default", "second", "one_block"])
def test_planted_planes_against_python(rule):
    for rlen, p in bc.planted_case():
        bc.same_as_py(api.planes_blocks(_planes(rlen, p), **rule), _planes(rlen, p), **rule)


def test_random_planes_against_python():
    rng = np.random.default_rng(1)
    hows = set()
    for _ in range(60):
        n, rlen = int(rng.integers(0, 40)), int(rng.integers(0, 400))
        rule = dict(min_gap=int(rng.integers(1, 25)), min_depth=int(rng.integers(1, 5)), min_alt=int(rng.integers(1, 4)), min_pct=int(rng.integers(1, 51)),
                    min_block=int(rng.integers(1, 12)), max_blocks=int(rng.integers(1, 33)))
        p = bc.random_planes(rng, n, rlen)
        got = api.planes_blocks(p, **rule)
        bc.same_as_py(got, p, **rule)
        lean = api.planes_blocks(p, rows=False, **rule)
        assert "rows" not in lean and lean["reads"].tobytes() == got["reads"].tobytes()
        hows |= set(got["reads"]["how"].tolist())
    assert hows == {0, 1, 2, 3}


def test_what_the_planted_planes_are_there_for(planted):
    case, want = planted
    by = {rlen: w for (rlen, _), w in zip(case, want)}
    spans = lambda w: [(int(b["first"]), int(b["end"])) for b in w["blocks"]]
    gaps = lambda rlen, i: (int(by[rlen]["reads"][i]["n_gaps"]), int(by[rlen]["reads"][i]["gap_rows"]))
    assert gaps(19, 0) == (0, 0) and gaps(20, 0) == (1, 20) and tuple(by[20]["reads"][1][["first_row", "end_row"]]) == (0, 0)
    assert gaps(63, 0) == (1, 20) and gaps(63, 1) == (0, 0) and spans(by[63]) == []                     # min_gap and one fewer; min_block - 1
    assert spans(by[64]) == [(15, 25), (44, 64)]                                                        # min_block; a block that ends at rlen
    assert spans(by[127]) == [(58, 80)] and gaps(127, 0) == (1, 64) and gaps(127, 1) == (1, 64)         # across 63 | 64
    assert gaps(128, 0) == (1, 64) and gaps(128, 1) == (1, 65) and gaps(128, 2) == (2, 63)              # 0xEE cuts a gap: 36 + 27 rows
    assert gaps(129, 0) == (2, 60) and spans(by[129]) == [(64, 129)]
    assert spans(by[4200]) == [(50, 4150)] and gaps(4200, 0) == (1, 4100) and gaps(4200, 30) == (1, 130) and gaps(4200, 31) == (1, 300)
    assert gaps(4200, 32) == (2, 59) and gaps(4200, 33) == (1, 64)
    assert tuple(by[2000]["seg"][["n_blocks", "n_found", "n_groups"]]) == (32, 35, 3)
    keys = sorted({int(k) for k in by[2000]["reads"]["key"]})
    assert keys[1] ^ keys[2] == 3 << 62 and keys[2] >= 2**63                                            # block 31 alone, and bit 63
    assert [int(by[2000]["reads"][i]["group"]) for i in (40, 0, 20)] == [0, 1, 2]
    big = by[600]
    assert spans(big) == [(100, 140), (300, 420)]
    st = bc.states(big["reads"], 2)
    assert st[120] == [bc.SKIP, bc.KEEP] and st[121] == [bc.PART, bc.SKIP] and st[122] == [bc.KEEP, bc.KEEP] and st[123] == [bc.PART, bc.PART]
    assert st[124] == [bc.KEEP, bc.SKIP] and st[125] == [bc.SKIP, bc.PART] and st[126] == [bc.KEEP, bc.KEEP] and st[127] == [bc.SKIP, bc.PART]
    assert st[128] == [bc.NOT, bc.PART] and st[112] == st[113] == [bc.NOT, bc.NOT] and st[39] == [bc.NOT, bc.KEEP]
    how = big["reads"]["how"].tolist()
    assert [how[i] for i in (115, 118, 128, 129, 114, 113, 112)] == [api.ISO_DIRECT, api.ISO_RARE, api.ISO_ASSIGNED, api.ISO_AMBIGUOUS, api.ISO_AMBIGUOUS,
                                                                    api.ISO_AMBIGUOUS, api.ISO_AMBIGUOUS]
    assert int((big["reads"]["key"] == big["reads"]["key"][115]).sum()) == 3 and int(big["reads"]["group"][128]) == int(big["reads"]["group"][115])
    assert int((big["reads"]["key"] == big["reads"]["key"][118]).sum()) == 2 and st[118] == [bc.PART, bc.KEEP]   # min_alt - 1 carriers
    every = np.concatenate([w["reads"] for w in want])
    assert set(every["how"].tolist()) == {0, 1, 2, 3}
    assert {s for w in want for row in bc.states(w["reads"], len(w["blocks"])) for s in row} == {0, 1, 2, 3}
    assert any(len(w["blocks"]) == 0 and len(w["reads"]) for w in want)
    one = api.planes_blocks(dict(case)[2000], max_blocks=1)
    assert tuple(one["seg"][["n_blocks", "n_found"]]) == (1, 35)


def test_refusals_write_nothing():
    L = _lib.load()
    p = bc.planted_case()[5][1]
    n, rlen = p.shape[0], p.shape[1] - 1
    good = [20, 3, 3, 25, 10, 32]
    fill = lambda dt, k: np.frombuffer(bytes([0xA5]) * (dt.itemsize * k), dt).copy()

    def call(rule, n_reads=n, length=rlen, base=p.ctypes.data, blocks=True, reads=True, seg=True):
        out = fill(api.BLOCK_ROW_DTYPE, rlen + 1), fill(api.PILE_BLOCK_DTYPE, 32), fill(api.READ_BLOCKS_DTYPE, n), fill(api.BLOCKS_SEG_DTYPE, 1)
        before = [o.tobytes() for o in out]
        rc = L.ioc_host_planes_blocks(base, n_reads, length, *rule, out[0].ctypes.data, out[1].ctypes.data if blocks else None,
                                      out[2].ctypes.data if reads else None, out[3].ctypes.data if seg else None)
        return rc, [o.tobytes() for o in out] == before

    assert call(good) == (0, False)
    for at, bad in ((0, 0), (1, 0), (2, 0), (3, 0), (3, 51), (4, 0), (5, 0), (5, 33), (0, -1)):
        rule = list(good)
        rule[at] = bad
        assert call(rule) == (-1, True), (at, bad)
    for kw in (dict(n_reads=-1), dict(length=-1), dict(base=None), dict(blocks=False), dict(reads=False), dict(seg=False)):
        assert call(good, **kw) == (-1, True), kw
    with pytest.raises(api.IocError):
        api.planes_blocks(p, min_pct=51)
    with pytest.raises(TypeError):
        api.planes_blocks(p, max_run=3)


def test_four_isoforms_and_three_truncated_reads():
    """The property case: T of 1000 random bases; 12 reads of T, 10 without [150, 190), 10 without that and [400, 520), 6 without
    [400, 520) alone, and T[:300], the third isoform from 250 on and T[100:450]; every read mutated at 8 %, aligned by the host
    aligner at gap_open(0.1) and projected.  (The flanks have to be this long: on a 600-base T the 80 bases behind the 120-row gap
    cannot pay for it, and the aligner leaves them as a free end.)  The seed is the first of 0, 1, 2, .. at which all four
    conditions hold: blocks_common.SEEDS_TRIED seeds were tried."""
    assert bc.find_seed(bc.SEED + 1) == (bc.SEED, bc.SEEDS_TRIED)
    T, reads, true = bc.property_case(bc.SEED)
    planes = bc.host_base_planes(T, reads)
    got = api.planes_blocks(planes)
    bc.same_as_py(got, planes)
    two, near, right, four = bc.property_holds(got, true)
    print("blocks", [(int(b["first"]), int(b["end"])) for b in got["blocks"]], "record", got["seg"])
    assert two and near and right and four
    direct = [int(((got["reads"]["group"] == g) & (got["reads"]["how"] == api.ISO_DIRECT)).sum()) for g in range(4)]
    st = bc.states(got["reads"], 2)
    order = sorted(range(4), key=lambda x: [(bc.KEEP, bc.KEEP), (bc.SKIP, bc.KEEP), (bc.SKIP, bc.SKIP), (bc.KEEP, bc.SKIP)][x][0] + 4 * [(0, 0), (1, 0), (1, 1), (0, 1)][x][1])
    assert [direct[order.index(x)] for x in range(4)] == list(bc.SIZES)
    assert int(got["seg"]["n_direct"]) == sum(bc.SIZES) and int(got["seg"]["n_reads"]) == 41
    for i, tr in enumerate(true[sum(bc.SIZES):], sum(bc.SIZES)):   # a truncated read has no state where it does not reach
        assert all(t is None and s == bc.NOT or t == s for s, t in zip(st[i], tr)), (i, st[i], tr)
