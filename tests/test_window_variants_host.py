"""The definitions of the variants of an insertion site on the host, without a GPU: ioc_host_ops_agreement against a plain loop;
ioc_host_key_isoforms against a restatement and against ioc_host_planes_inserts itself; ioc_host_insert_window_variants against
variants_common.py_variants on planted segments, where every rule of the decision bites; what it refuses, against canaries; that the
definitions that existed return what they returned; and the property case."""
import ctypes as C

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import inserts_common as ic
from tests import variants_common as vc
from tests import windows_common as wc

A, B, OTHER, NONE = vc.A, vc.B, vc.OTHER, vc.NONE


def test_the_symbols_and_the_records():
    L = _lib.load()
    for s in ("ioc_host_ops_agreement", "ioc_host_key_isoforms", "ioc_host_insert_window_variants", "ioc_planes_insert_window_variants"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
    assert api.WINDOW_VARIANT_DTYPE.itemsize == 32 and api.READ_VARIANTS_DTYPE.itemsize == 16 and api.VARIANTS_SEG_DTYPE.itemsize == 32
    assert (api.INS_LACK, api.INS_CARRY, api.INS_CARRY_B, api.INS_NONE) == (0, 1, 2, 3) and api.VARIANTS_RULE["min_agree"] == 45


def test_the_agreement_against_a_plain_loop():
    rng = np.random.default_rng(1)
    chosen = [b"", b"=", b"X", b"D", b"I", b"i=d", b"====XXDI", b"=" * 600, b"I" * 513 + b"D" * 512, b"XDI" * 100]
    for ops in chosen + [bytes(b"=XIDid"[x] for x in rng.integers(0, 6, int(rng.integers(1, 300)))) for _ in range(200)]:
        assert api.ops_agreement(ops) == vc.py_agreement(ops), ops
    for bad in (b"=M", b"=\0=", b"N"):
        with pytest.raises(ValueError):
            api.ops_agreement(bad)
    for q, t in ((b"ACGTTGCAAC", b"ACGTAGCAAC"), (b"ACGT", b"ACGTTTTTACGT"), (b"AAAA", b"CCCC"), (b"G", b"G")):   # the global aligner's own bytes
        assert api.ops_agreement(api.align_global_ops(q, t)[0]) == vc.py_agreement(wc.py_global(q, t)[0])


@pytest.fixture(scope="module")
def planted():
    seg = vc.planted_segment()
    reads, base, qpos, sites, keys = seg
    return seg, api.insert_window_variants(base, qpos, [len(r) for r in reads], sites, keys, reads, **vc.PLANT)


def test_the_planted_segment_against_the_restatement(planted):
    (reads, base, qpos, sites, keys), got = planted
    vc.same_as_py(got, vc.py_variants(reads, base, qpos, sites, keys, **vc.PLANT))
    for rule in (dict(min_agree=1), dict(min_agree=100), dict(min_agree=30, min_alt=1, min_pct=1), dict(min_alt=6), dict(min_pct=50), dict(match=1, mismatch=-3, gap=1),
                 dict(slack=0), dict(slack=32)):
        r = {**vc.PLANT, **rule}
        vc.same_as_py(api.insert_window_variants(base, qpos, [len(x) for x in reads], sites, keys, reads, **r), vc.py_variants(reads, base, qpos, sites, keys, **r))


def test_what_each_planted_site_is_there_for(planted):
    (reads, base, qpos, sites, keys), got = planted
    var, variant, win = got["var"], got["variant"], got["win"]
    old = wc.host_windows(reads, base, qpos, sites, keys, **{k: v for k, v in vc.PLANT.items()})
    assert got["win"].tobytes() == old["win"].tobytes()   # round A's template, lo and hi are the window stage's
    # site 0 splits 6 / 5; the template is its own voter, near itself with its length; of five equal lengths the third index is template B
    assert [int(var[0][f]) for f in ("split", "template_pair_b", "tlen_b", "n_a", "n_b", "n_other", "n_far")] == [1, 5, 41, 6, 5, 0, 5]
    assert variant[:, 0].tolist() == [A, B] * 5 + [A] + [NONE] * 4
    t = int(win[0]["template_pair"])
    assert got["agree"][t, 0, 0] == int(win[0]["tlen"]) and got["agree"][5, 0, 1] == 41 and got["agree"][t, 0, 1] == vc.NO
    assert int(win[0]["n_short"]) == 1 and int(win[0]["n_long"]) == 1
    state = lambda i, k: (int(got["key2"][i]) >> (2 * k)) & 3
    assert [state(i, 0) for i in (11, 12)] == [vc.NOT, vc.NOT] and [(int(keys[i]) & 3) for i in (11, 12)] == [vc.CARRY, vc.CARRY]   # SHORT and LONG: re-keyed
    assert [state(i, 0) for i in range(11)] == [vc.CARRY, vc.CARRY_B] * 5 + [vc.CARRY]
    # site 1: n_far < need, round B does not run
    assert [int(var[1][f]) for f in ("split", "template_pair_b", "tlen_b", "n_a", "n_b", "n_other", "n_far")] == [0, -1, 0, 11, 0, 0, 2]
    assert (got["agree"][:, 1, 1] == vc.NO).all()
    # site 2: round B runs, n_b < need: today's consensus byte for byte, the far voters voting
    assert [int(var[2][f]) for f in ("split", "n_a", "n_b", "n_other", "n_far")] == [0, 11, 1, 4, 5] and int(var[2]["template_pair_b"]) >= 0
    # site 3: an OTHER voter, re-keyed to NONE
    assert [int(var[3][f]) for f in ("split", "n_a", "n_b", "n_other", "n_far")] == [1, 6, 4, 1, 5] and variant[10, 3] == OTHER and state(10, 3) == vc.NOT
    assert int(var[4]["n_far"]) == 0 and int(var[4]["split"]) == 0
    for k in (1, 2, 4):
        assert (got["seq"][2 * k], got["qual"][2 * k]) == (old["seq"][k], old["qual"][k]) and got["seq"][2 * k + 1] == b"", k
        assert all(state(i, k) == (int(keys[i]) >> (2 * k)) & 3 for i in range(len(reads))), k
    for k in (0, 3):
        assert got["seq"][2 * k] != old["seq"][k] or got["seq"][2 * k + 1] != b""
        assert len(got["seq"][2 * k + 1]) > 0
    mask = [sum(3 << (2 * k) for k in range(5) if state(i, k) != vc.NOT) for i in range(len(reads))]
    assert got["mask2"].tolist() == mask


def test_a_segment_where_nothing_splits_is_the_window_stage():
    reads, base, qpos, sites, keys = vc.quiet_segment()
    got = api.insert_window_variants(base, qpos, [len(r) for r in reads], sites, keys, reads, **vc.PLANT)
    old = wc.host_windows(reads, base, qpos, sites, keys, **vc.PLANT)
    assert got["win"].tobytes() == old["win"].tobytes() and got["key2"].tobytes() == keys.tobytes()
    assert got["seq"] == [old["seq"][0], b"", old["seq"][1], b""] and got["qual"] == [old["qual"][0], b"", old["qual"][1], b""]
    assert (got["var"]["split"] == 0).all() and (got["var"]["n_far"] == 0).all() and (got["var"]["template_pair_b"] == -1).all()
    vc.same_as_py(got, vc.py_variants(reads, base, qpos, sites, keys, **vc.PLANT))


def test_the_recount_against_the_restatement_and_the_insert_stage():
    rng = np.random.default_rng(9)
    for trial in range(60):
        n, S = int(rng.integers(0, 40)), int(rng.integers(0, 5))
        full = (1 << (2 * S)) - 1
        key = np.array([int(x) & full for x in rng.integers(0, 1 << 8, n)], np.uint64)
        mask = np.array([sum(3 << (2 * k) for k in range(S) if (int(x) >> (2 * k)) & 3 != 3) for x in key], np.uint64)
        pre = ic.random_pre(rng, n) if trial % 2 else None
        kw = dict(pre_key=pre[0], pre_mask=pre[1], pre_full=pre[2]) if pre else {}
        for min_alt in (1, 3):
            g, h, c = api.key_isoforms(key, mask, full, min_alt, **kw)
            wg, wh, wc_ = vc.py_key_isoforms(key, mask, full, min_alt, **kw)
            assert g.tolist() == wg.tolist() and h.tolist() == wh.tolist() and c == wc_, trial
    # ioc_host_planes_inserts itself: its group and how are the recount of its own keys, with and without the block words
    for rlen, b, l, (pk, pm, pf) in ic.planted_case():
        b, l = b.reshape(-1, rlen + 1), l.reshape(-1, rlen + 1)
        for kw in ({}, dict(pre_key=pk, pre_mask=pm, pre_full=pf)):
            got = api.planes_inserts(b, l, **kw)
            S = len(got["sites"])
            key = got["reads"]["key"]
            mask = np.array([sum(3 << (2 * k) for k in range(S) if (int(x) >> (2 * k)) & 3 != 3) for x in key], np.uint64)
            g, h, c = api.key_isoforms(key, mask, (1 << (2 * S)) - 1, ic.DEFAULT["min_alt"], **kw)
            assert g.tolist() == got["reads"]["group"].tolist() and h.tolist() == got["reads"]["how"].tolist(), rlen
            assert [c[f] for f in ("n_groups", "n_direct", "n_assigned", "n_rare", "n_ambiguous")] == [int(got["seg"][f]) for f in
                                                                                                    ("n_groups", "n_direct", "n_assigned", "n_rare", "n_ambiguous")]


def test_the_definitions_that_existed_return_what_they_returned():
    for rlen, b, l, pre in ic.planted_case():
        b, l = b.reshape(-1, rlen + 1), l.reshape(-1, rlen + 1)
        ic.same_as_py(api.planes_inserts(b, l), b, l)
        ic.same_as_py(api.planes_inserts(b, l, pre_key=pre[0], pre_mask=pre[1], pre_full=pre[2]), b, l, pre=pre)
    reads, base, qpos, sites, keys, _ = wc.planted_segment(max_win=40)
    got = api.insert_windows(base, qpos, [len(r) for r in reads], sites, keys, max_win=40)
    win, cls, start, ln = wc.py_windows(base, qpos, [len(r) for r in reads], sites, keys, max_win=40)
    assert got["win"].tobytes() == win.tobytes() and got["cls"].tobytes() == cls.tobytes() and got["start"].tobytes() == start.tobytes() and got["len"].tobytes() == ln.tobytes()


def test_refusals_against_canaries():
    reads, base, qpos, sites, keys = vc.quiet_segment()
    L = _lib.load()
    n, S, rlen = len(reads), len(sites), base.shape[1] - 1
    ql = np.array([len(r) for r in reads], np.int32)
    blob, roff = b"".join(reads), np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    bound = 2 * S * (7 * 80 + 6)

    def call(**kw):
        a = dict(slack=8, max_win=80, match=2, mismatch=-2, gap=2, depth=3, min_agree=45, min_alt=3, min_pct=25, cap=bound, roff=roff, sites=sites, n_sites=S)
        a.update(kw)
        outs = [np.full(m, 0xA5, np.uint8) for m in (S * 32, S * 32, n * S, n * S * 8, bound, bound, (2 * S + 1) * 8, 2 * S * 32, n * 8, n * 8)]
        rc = L.ioc_host_insert_window_variants(base.ctypes.data, qpos.ctypes.data, ql.ctypes.data, n, rlen, a["sites"].ctypes.data, a["n_sites"], keys.ctypes.data, blob,
                                               a["roff"].ctypes.data, a["slack"], a["max_win"], a["match"], a["mismatch"], a["gap"], a["depth"], a["min_agree"],
                                               a["min_alt"], a["min_pct"], *(o.ctypes.data for o in outs[:6]), a["cap"], *(o.ctypes.data for o in outs[6:]))
        return rc, all((o == 0xA5).all() for o in outs)

    assert call() == (0, False)
    outside = sites.copy()
    outside[1]["end"] = rlen + 1
    wrong = roff.copy()
    wrong[3] += 1
    for bad in (dict(min_agree=0), dict(min_agree=101), dict(min_alt=0), dict(min_pct=0), dict(min_pct=51), dict(slack=-1), dict(slack=33), dict(max_win=0), dict(max_win=513),
                dict(gap=-1), dict(match=(1 << 20) + 1), dict(depth=0), dict(sites=outside), dict(n_sites=33), dict(roff=wrong), dict(cap=-1)):
        assert call(**bad) == (-1, True), bad
    assert call(cap=bound - 1) == (-4, True)
    # a NULL pointer that is needed: the window records, the read lengths
    outs = [np.full(m, 0xA5, np.uint8) for m in (S * 32, S * 32, n * S, n * 8, n * 8)]
    for win, lens in ((None, ql.ctypes.data), (outs[0].ctypes.data, None)):
        rc = L.ioc_host_insert_window_variants(base.ctypes.data, qpos.ctypes.data, lens, n, rlen, sites.ctypes.data, S, keys.ctypes.data, blob, roff.ctypes.data, 8, 80, 2, -2,
                                               2, 3, 45, 3, 25, win, outs[1].ctypes.data, outs[2].ctypes.data, None, None, None, 0, None, None, outs[3].ctypes.data,
                                               outs[4].ctypes.data)
        assert rc == -1 and all((o == 0xA5).all() for o in outs)
    # the agreement and the recount
    out = np.full(1, 0x5A5A5A5A, np.int32)
    assert L.ioc_host_ops_agreement(b"==Z", 3, out.ctypes.data_as(C.POINTER(C.c_int32))) == -1 and out[0] == 0x5A5A5A5A
    assert L.ioc_host_ops_agreement(b"==", -1, out.ctypes.data_as(C.POINTER(C.c_int32))) == -1 and out[0] == 0x5A5A5A5A
    g, h, c = np.full(4, 0x5A, np.int32), np.full(4, 0x5A, np.int32), np.full(5, 0x5A, np.int32)
    k = np.zeros(4, np.uint64)
    for args in ((None, None, 0, k.ctypes.data, k.ctypes.data, 0, 4, 0), (k.ctypes.data, None, 0, k.ctypes.data, k.ctypes.data, 0, 4, 1),
                 (None, None, 0, k.ctypes.data, k.ctypes.data, 0, -1, 1), (None, None, 0, None, k.ctypes.data, 0, 4, 1)):
        assert L.ioc_host_key_isoforms(*args, g.ctypes.data, h.ctypes.data, c.ctypes.data) == -1
        assert (g == 0x5A).all() and (h == 0x5A).all() and (c == 0x5A).all()


def test_the_property_case_on_the_host_path():
    """two exons at one junction, 8 % errors: the site splits, every carrier is of its planted exon, each consensus is its own exon's"""
    assert vc.SEEDS_TRIED <= 5
    frame, exons, reads, planted, (base, qpos, ins), got = vc.host_property()
    assert len(ins["sites"]) == 2 and int(got["win"][0]["n_voters"]) == 20
    splits, right, margin = vc.property_holds(got, planted, frame, exons)
    dist = vc.distances(frame, exons, got, planted)
    print("variants", got["var"], "(to its own true window, to the other's, length)", dist)
    assert splits and right and margin
    assert dist == vc.PINNED
    assert int(got["var"][1]["split"]) == 0 and got["seq"][3] == b""
    # the window stage alone calls a mixture here: nearer to neither true window than the variants' consensus is to its own
    old = wc.host_windows(reads, base, qpos, ins["sites"], ins["reads"]["key"])
    assert old["seq"][1] == got["seq"][2] and old["seq"][0] != got["seq"][0]
    # the isoforms again: four of them, where the insert stage saw three
    S = 2
    g, h, c = api.key_isoforms(got["key2"], got["mask2"], (1 << (2 * S)) - 1, 3)
    assert c["n_groups"] == 4 and int(ins["seg"]["n_groups"]) == 3
    assert [int(got["key2"][i]) for i in (0, 10, 20, 26)] == [6, 5, 4, 0] and [int(g[i]) for i in (0, 10, 20, 26)] == [3, 2, 1, 0]
