"""ioc_planes_correct_groups: k_group_pile over the groups' tables and one more per segment, and k_iso_correct_count /
k_iso_correct_emit over host planes that are uploaded, against the definition restated in Python (tests/iso_correct_common.py:
py_planes_pile for the tables, py_correct_long pair by pair).  One call holds two segments of 130 and 200 rows, so that runs and
long rows cross a 64-row step, and 37 pairs (ten workgroups of four waves, the last one short): pairs in no group, a group of
min_depth - 1 members, one of exactly min_depth, an empty one; long rows of 7, 8 and 254 bases at rows 0, 63, 64 and rlen and two
in one chunk; one pair for each way of being unresolved.  Sequences, qualities and records are compared as bytes."""
import numpy as np
import pytest

from isonclust2_amd import api
from tests import correct_common as cc
from tests import iso_correct_common as ic

pytestmark = pytest.mark.gpu

PLANES = ("frames", "seg_of_pair", "group", "n_groups")


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


@pytest.fixture(scope="module")
def case(ctx):
    c = ic.grouped_case()
    ctx.align_set_pool(c["queries"])   # (pair i's read is sequence i of the pool)
    return c


def _call(ctx, c, query=None, **kw):
    n = len(c["base"])
    return ctx.planes_correct_groups(c["frames"], c["seg_of_pair"], c["group"], c["n_groups"], list(range(n)) if query is None else query, c["base"], c["slots"],
                                     c["ilen"], c["qpos"], **kw)


@pytest.mark.parametrize("max_run", [10, 0])
def test_against_the_definition(ctx, case, max_run):
    c = case
    assert len(c["base"]) == 37
    seqs, quals, recs = _call(ctx, c, max_run=max_run)
    want = ic.py_correct_groups(c["frames"], c["seg_of_pair"], c["group"], c["n_groups"], c["queries"], c["base"], c["slots"], c["ilen"], c["qpos"], max_run=max_run)
    assert recs.dtype == api.ISO_CORRECT_STATS_DTYPE
    got = ic.stats_dicts(recs)
    for i in range(len(seqs)):
        assert got[i] == want[2][i], i
        assert seqs[i] == want[0][i] and quals[i] == want[1][i], i
    assert [len(s) for s in seqs] == recs["out_len"].tolist()
    # which table: group 0 of segment 0 (9 members) and the group of exactly min_depth are held against their own, the group of
    # min_depth - 1 and the pairs in no group against their segment's
    sop, grp = np.array(c["seg_of_pair"]), np.array(c["group"])
    assert set(recs["table"][(sop == 0) & (grp == 0)]) == {0} and set(recs["table"][(sop == 0) & (grp == 2)]) == {2}
    assert set(recs["table"][(sop == 0) & ((grp == 1) | (grp == -1))]) == {-1} and set(recs["table"][(sop == 1) & (grp == -1)]) == {-2}
    assert set(recs["table"][(sop == 1) & (grp == 0)]) == {4} and set(recs["table"][(sop == 1) & (grp == 1)]) == {5}
    # the unresolved ones, and nobody else
    assert np.flatnonzero(recs["flags"]).tolist() == c["unresolved"] == [1, 15, 27] and all(seqs[i] == b"" for i in c["unresolved"])
    # the long rows came through: 7, 8 and 254 bases, at every step
    assert int(recs["n_long_runs"].sum()) == 17 and int(recs["n_long_bases"][5]) == 254 and int(recs["n_long_bases"][30]) == 7 + 254 + 254
    for i in (2, 5, 9, 20, 30):   # ... as the read has them, at quality 0
        for p in np.flatnonzero(c["ilen"][i] > ic.SLOTS):
            run = c["queries"][i][int(c["qpos"][i][p]):int(c["qpos"][i][p]) + int(c["ilen"][i][p])]
            at = seqs[i].find(run)
            assert at >= 0 and quals[i][at:at + len(run)] == b"!" * len(run)
    total = {f: int(recs[f].sum()) for f in ic.FIELDS}
    print(total)
    assert total["n_sub"] and total["n_ins_drop"] and total["n_guarded"] and total["n_low"]
    assert (total["n_fill"] > 0) == (max_run > 0)


def test_the_isoforms_keep_what_the_cluster_would_fill(ctx, case):
    """What the groups are for: the reads of group 2 of segment 0 (exactly min_depth of them) lack rows 60 .. 67; held against their
    own table nothing is filled there, held against the whole segment (as a pair in no group is) the 8 rows are filled."""
    c = case
    _, _, recs = _call(ctx, c)
    alone = dict(c, group=[-1] * len(c["group"]))
    _, _, all_recs = _call(ctx, alone)
    mine = [i for i in range(len(c["group"])) if (c["seg_of_pair"][i], c["group"][i]) == (0, 2)]
    assert len(mine) == cc.DEFAULT["min_depth"]
    assert all(int(all_recs["n_fill"][i]) >= 8 for i in mine) and all(int(recs["n_fill"][i]) < 8 for i in mine)
    assert set(all_recs["table"].tolist()) == {-1, -2}


def test_one_group_of_everything_is_planes_correct(ctx, case):
    """one group per segment that holds every pair, no long row: ioc_planes_correct on T(g, *)"""
    c = case
    n = len(c["base"])
    short = [np.minimum(l, ic.SLOTS).astype(np.uint8) for l in c["ilen"]]
    seqs, quals, recs = ctx.planes_correct_groups(c["frames"], c["seg_of_pair"], [0] * n, [1, 1], list(range(n)), c["base"], c["slots"], short, c["qpos"])
    cols = [np.zeros(len(f) + 1, api.PILEUP_DTYPE) for f in c["frames"]]
    ins = [np.zeros(len(f) + 1, api.PILEUP_INS_DTYPE) for f in c["frames"]]
    for i in range(n):
        api.planes_pile(c["base"][i], c["slots"][i], cols=cols[c["seg_of_pair"][i]], ins=ins[c["seg_of_pair"][i]])
    s2, q2, r2 = ctx.planes_correct(c["frames"], np.concatenate(cols), np.concatenate(ins), c["seg_of_pair"], c["base"], c["slots"])
    assert seqs == s2 and quals == q2
    for f in cc.FIELDS:
        assert recs[f].tolist() == r2[f].tolist(), f
    assert recs["table"].tolist() == c["seg_of_pair"] and not recs["flags"].any() and not recs["n_long_runs"].any()


def test_the_refusals_write_nothing(ctx, case):
    c = case
    n = len(c["base"])
    bound = sum(api.pileup_call_bound(len(c["frames"][g])) for g in c["seg_of_pair"]) + sum(len(q) for q in c["queries"])
    seqs, _, _ = _call(ctx, c, cap=bound)
    assert sum(len(s) for s in seqs) <= bound
    for bad, code in ((dict(cap=bound - 1), -4), (dict(min_depth=0), -1), (dict(min_pct=51), -1), (dict(max_run=65), -1), (dict(query=[n] + list(range(1, n))), -1),
                      (dict(query=[-1] + list(range(1, n))), -1)):
        with pytest.raises(api.IocError) as e:
            _call(ctx, c, **bad)
        assert e.value.code == code, bad
    for group, n_groups in (([4] + c["group"][1:], c["n_groups"]), ([-2] + c["group"][1:], c["n_groups"]), (c["group"], [4, -1])):
        with pytest.raises(api.IocError) as e:
            _call(ctx, dict(c, group=group, n_groups=n_groups))
        assert e.value.code == -1
    assert ctx.planes_correct_groups([], [], [], [], [], [], [], [], [])[:2] == ([], [])
