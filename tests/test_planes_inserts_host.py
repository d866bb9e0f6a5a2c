"""ioc_host_ops_project_ilen and ioc_host_planes_inserts, the definitions of the length plane and of the insertion sites of a
cluster with every read's combined isoform: the length plane against a plain loop on hand-written strings; the sites against a
plain restatement in Python (inserts_common.py_inserts) on the planted planes of the GPU test and on random planes, as bytes; what
both refuse, and that a refusal writes nothing; what the planted planes are there for, measured; and the two property cases through
the host aligner and the host projections alone."""
import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import blocks_common as bc
from tests import inserts_common as ic


def plain_ilen(ops, rlen):
    out, r, run = [0] * (rlen + 1), 0, 0
    for op in ops + "$":
        if op == "I":
            run += 1
            continue
        if run:
            out[r], run = min(run, 255), 0
        r += op in "=XDd"
    return out


STRINGS = ["", "=", "I", "i", "I=", "=I", "II=I=", "iI==Ii", "iiIII=D=IIIIdd", "=X" + "I" * 254 + "D" + "I" * 255 + "=" + "I" * 256 + "X" + "I" * 300,
           "I" * 300, "d" + "I" * 3 + "=" * 5 + "I" * 2, "i" * 4 + "=" + "I" * 7 + "i" * 3, "==DD" + "I" * 19 + "X" + "I" * 14 + "=="]


@pytest.mark.parametrize("ops", STRINGS, ids=[str(i) for i in range(len(STRINGS))])
def test_the_length_plane_against_a_plain_loop(ops):
    rlen = sum(c in "=XDd" for c in ops)
    got = api.ops_project_ilen(ops.encode(), rlen)
    assert got.tolist() == plain_ilen(ops, rlen), ops[:40]


def test_the_length_plane_on_the_runs_that_matter():
    ops = "=X" + "I" * 254 + "D" + "I" * 255 + "=" + "I" * 256 + "X" + "I" * 300
    assert api.ops_project_ilen(ops.encode(), 5).tolist() == [0, 0, 254, 255, 255, 255]        # 254, 255, 256 and 300: the last in front of row rlen
    assert api.ops_project_ilen(b"I" * 1 + b"=", 1).tolist() == [1, 0]                       # a run of 1 in front of row 0
    assert api.ops_project_ilen(b"iI==Ii", 2).tolist() == [1, 0, 1]                          # an 'I' run beside 'i' on either side
    assert api.ops_project_ilen(b"", 0).tolist() == [0]
    L = _lib.load()
    out = np.full(8, 0xA5, np.uint8)
    for ops, ln, rlen, ptr in ((b"==", 2, 3, True), (b"==", 2, 1, True), (b"=Q", 2, 2, True), (b"==", -1, 2, True), (b"==", 2, -1, True), (b"==", 2, 2, False),
                               (None, 2, 2, True)):
        assert L.ioc_host_ops_project_ilen(ops, ln, rlen, out.ctypes.data if ptr else None) == -1
        assert out.tolist() == [0xA5] * 8
    with pytest.raises(ValueError):
        api.ops_project_ilen(b"=I=", 3)


def _shape(r, b, l):
    return b.reshape(-1, r + 1), l.reshape(-1, r + 1)


@pytest.mark.parametrize("rule", [{}, dict(slack=0), dict(slack=32), dict(max_sites=1), dict(min_ins=41, min_depth=2, min_alt=2, min_pct=10, slack=3)],
                         ids=["default", "slack0", "slack32", "one_site", "second"])
def test_planted_planes_against_python(rule):
    for r, b, l, pre in ic.planted_case():
        b, l = _shape(r, b, l)
        ic.same_as_py(api.planes_inserts(b, l, pre_key=pre[0], pre_mask=pre[1], pre_full=pre[2], **rule), b, l, pre, **rule)
        if r in (600, 127):
            ic.same_as_py(api.planes_inserts(b, l, **rule), b, l, None, **rule)   # the stage on its own


def test_random_planes_against_python():
    rng = np.random.default_rng(11)
    hows, sts = set(), set()
    for t in range(60):
        n, rlen = int(rng.integers(0, 40)), int(rng.integers(0, 300))
        rule = dict(min_ins=int(rng.choice([1, 3, 20, 40, 255])), slack=int(rng.choice([0, 1, 8, 31, 32])), min_depth=int(rng.integers(1, 5)),
                    min_alt=int(rng.integers(1, 4)), min_pct=int(rng.integers(1, 51)), max_sites=int(rng.integers(1, 33)))
        b, l = ic.random_planes(rng, n, rlen)
        pre = ic.random_pre(rng, n) if t % 3 else None
        kw = dict(pre_key=pre[0], pre_mask=pre[1], pre_full=pre[2]) if pre else {}
        got = api.planes_inserts(b, l, **kw, **rule)
        ic.same_as_py(got, b, l, pre, **rule)
        lean = api.planes_inserts(b, l, rows=False, **kw, **rule)
        assert "rows" not in lean and lean["reads"].tobytes() == got["reads"].tobytes()
        hows |= set(got["reads"]["how"].tolist())
        sts |= {s for row in ic.states(got["reads"], len(got["sites"])) for s in row}
    assert hows == {0, 1, 2, 3} and sts == {ic.LACK, ic.CARRY, ic.NOT}


def test_what_the_planted_planes_are_there_for():
    case = ic.planted_case()
    assert sorted({len(b) for _, b, _, _ in case}) == [0, 1, 3, 6, 64, 65, 130]
    by = {slack: {r: w for (r, _, _, _), w in zip(case, ic.host_segments(case, slack=slack))} for slack in (0, 8, 32)}
    spans = lambda w: [(int(s["first"]), int(s["end"])) for s in w["sites"]]
    lens = lambda w: [(int(s["len_min"]), int(s["len_max"])) for s in w["sites"]]
    d = by[8]
    assert spans(d[0]) == spans(d[1]) == spans(d[65]) == [] and spans(d[2]) == [(1, 2)]                     # no junction; a site at 1 that ends at rlen - 1
    assert spans(d[63]) == [(1, 9), (55, 63)] and spans(by[0][63]) == [] and spans(by[32][63]) == [(1, 63)]  # rows 0 and rlen are seen through the window only
    assert spans(d[64]) == [(1, 64)] and lens(by[32][64]) == [(65 * 255, 65 * 255)] and lens(d[64]) == [(17 * 255, 17 * 255)]
    assert spans(d[127]) == [(58, 69)] and lens(d[127]) == [(24, 24)] and spans(by[0][127]) == []           # 12 + 12 across 63 | 64: no single run
    assert spans(by[32][127]) == [(34, 93)]
    assert int(d[127]["reads"][30]["ins_bases"]) == 0 and int(d[127]["reads"][0]["ins_bases"]) == 24        # a byte at a junction not spanned
    assert int(d[127]["rows"][70]["span"]) == 63 and int(d[127]["rows"][71]["span"]) == 62 and int(d[127]["rows"][72]["span"]) == 63   # 6 and 0xEE
    assert int(d[127]["rows"][100]["in_ins"]) == 3                                                          # min_alt carriers are not need(64)
    assert spans(by[0][128]) == [(64, 65)] and int(by[0][128]["sites"][0]["n_carry"]) == 20                 # exactly min_ins, and one fewer
    assert spans(d[129]) == [(120, 129)] and tuple(d[129]["sites"][0][["n_carry", "n_lack"]]) == (80, 50)
    assert spans(d[4200]) == [(1992, 2009), (4092, 4099)] and spans(by[0][4200]) == [(2000, 2001)]          # across 4095 | 4096
    assert tuple(d[2000]["seg"][["n_sites", "n_found", "n_groups"]]) == (32, 35, 3)
    keys = sorted({int(k) for k in d[2000]["reads"]["key"][:63]})
    assert keys[1] ^ keys[2] == 1 << 62 and int(d[2000]["reads"]["key"][63]) == 3 << 62                      # site 31 alone; no state there: bit 63
    assert tuple(d[2000]["reads"][63][["group", "how"]]) == (0, api.ISO_ASSIGNED)
    big = d[600]
    assert spans(big) == [(92, 109), (292, 309)] and int(big["seg"]["n_groups"]) == 6
    rd = big["reads"]
    group = lambda i: int(rd[i]["group"])
    assert [group(i) for i in (112, 0, 40, 100, 70, 20)] == [0, 1, 2, 3, 4, 5]      # (Z, 00) (Y, 00) (Y, A) (Y, B) (Y, AB) (X, 00): X last, unsigned
    assert [int(rd[i]["how"]) for i in (112, 115, 117, 118, 119, 120, 121, 122, 123)] == [
        api.ISO_DIRECT, api.ISO_RARE, api.ISO_AMBIGUOUS, api.ISO_AMBIGUOUS, api.ISO_ASSIGNED, api.ISO_ASSIGNED, api.ISO_AMBIGUOUS, api.ISO_AMBIGUOUS, api.ISO_ASSIGNED]
    assert group(119) == group(123) == 5 and group(120) == 2
    alone = api.planes_inserts(*_shape(600, case[9][1], case[9][2]))
    assert int(alone["seg"]["n_groups"]) == 4 and alone["sites"].tobytes() == big["sites"].tobytes()
    every = np.concatenate([w["reads"] for w in d.values()])
    assert set(every["how"].tolist()) == {0, 1, 2, 3}


def test_refusals_write_nothing():
    L = _lib.load()
    _, b, l, _ = ic.planted_case()[4]
    n, rlen = b.shape[0], b.shape[1] - 1
    pk, pm = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    good = [20, 8, 3, 3, 25, 32]
    fill = lambda dt, k: np.frombuffer(bytes([0xA5]) * (dt.itemsize * k), dt).copy()

    def call(rule, n_reads=n, length=rlen, base=b.ctypes.data, ilen=l.ctypes.data, key=None, mask=None, sites=True, reads=True, seg=True):
        out = fill(api.INSERT_ROW_DTYPE, rlen + 1), fill(api.PILE_INSERT_DTYPE, 32), fill(api.READ_INSERTS_DTYPE, n), fill(api.INSERTS_SEG_DTYPE, 1)
        before = [o.tobytes() for o in out]
        rc = L.ioc_host_planes_inserts(base, ilen, n_reads, length, *rule, key, mask, 0, out[0].ctypes.data, out[1].ctypes.data if sites else None,
                                       out[2].ctypes.data if reads else None, out[3].ctypes.data if seg else None)
        return rc, [o.tobytes() for o in out] == before

    assert call(good) == (0, False) and call(good, key=pk.ctypes.data, mask=pm.ctypes.data) == (0, False)
    for at, bad in ((0, 0), (0, 256), (1, -1), (1, 33), (2, 0), (3, 0), (4, 0), (4, 51), (5, 0), (5, 33)):
        rule = list(good)
        rule[at] = bad
        assert call(rule) == (-1, True), (at, bad)
    for kw in (dict(n_reads=-1), dict(length=-1), dict(base=None), dict(ilen=None), dict(sites=False), dict(reads=False), dict(seg=False),
               dict(key=pk.ctypes.data), dict(mask=pm.ctypes.data)):
        assert call(good, **kw) == (-1, True), kw
    with pytest.raises(api.IocError):
        api.planes_inserts(b, l, min_ins=256)
    with pytest.raises(TypeError):
        api.planes_inserts(b, l, min_gap=3)


def test_property_a_both_exons_are_insertions():
    """The reads of blocks_common.property_case — four isoforms of a 1000-base transcript, 8 % errors — aligned by the host aligner
    against the isoform that lacks [150, 190) and [400, 520): at the default rule exactly two sites, each holding its planted
    junction (150 and 360), the true state of all 38 complete reads, four isoforms.  The seed is the first from 0 at which this
    holds: inserts_common.SEEDS_TRIED_A seeds were tried."""
    assert ic.find_seeds()[0] == (ic.SEED_A, ic.SEEDS_TRIED_A)
    base, ilen, got = ic.run_a(ic.SEED_A)
    ic.same_as_py(got, base, ilen)
    print("sites", got["sites"], "record", got["seg"])
    assert all(ic.property_a_holds(got))
    whole = got["reads"][:sum(bc.SIZES)]   # (T[100:450] ends 50 bases into the second exon: what it says there is not held against anything)
    direct = [int(((whole["group"] == g) & (whole["how"] == api.ISO_DIRECT)).sum()) for g in range(4)]
    order = sorted(range(4), key=lambda x: ic.TRUE_A[x][0] + 4 * ic.TRUE_A[x][1])   # the key of each isoform, ascending
    assert [direct[order.index(x)] for x in range(4)] == list(bc.SIZES)
    st = ic.states(got["reads"], 2)
    assert st[38][0] == ic.CARRY and st[40][0] == ic.CARRY and st[39][1] == ic.LACK   # the truncated reads, where they reach across


def test_property_b_a_block_and_an_insertion():
    """The same reads against the isoform that lacks [150, 190) only: the block stage alone reports 2 isoforms, blocks and sites
    together the true 4, with every complete read in its own.  inserts_common.SEEDS_TRIED_B seeds were tried."""
    assert ic.find_seeds()[1] == (ic.SEED_B, ic.SEEDS_TRIED_B)
    base, ilen, blocks, pre, got = ic.run_b(ic.SEED_B)
    ic.same_as_py(got, base, ilen, pre)
    print("blocks", blocks["blocks"], "sites", got["sites"], "record", got["seg"])
    assert all(ic.property_b_holds(blocks, got))
    assert int(got["sites"][0]["first"]) <= 150 < int(got["sites"][0]["end"])
    assert int(api.planes_inserts(base, ilen)["seg"]["n_groups"]) == 2   # the sites alone see two as well


def test_one_run_of_min_ins_is_not_the_rule():
    """A documented fact about py_inserts, so that nobody simplifies the window away: at slack 0 — W(p) is then the one run in front
    of p — property A fails on seeds 0 .. 5 (measured: on all six; the aligner breaks a 40-base exon into runs of 19 + 14 or 22 +
    10 a few rows apart)."""
    failed = [s for s in range(6) if not all(ic.property_a_holds(ic.run_a(s, py=True, slack=0)[2]))]
    print("property A at slack 0 fails on seeds", failed)
    assert failed
    assert all(all(ic.property_a_holds(ic.run_a(s, py=True)[2])) for s in failed[:2])   # ... where the window holds
