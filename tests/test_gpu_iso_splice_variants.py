"""The slot-aware plan kernel of ioc_iso_splice.hip (k_splice_plan<true>) and the call passes behind it against the host definition,
as bytes, through ioc_planes_isoforms_full_variants: sequences, qualities, offsets, the polish, splice and site records and the group
tables.  The first segment is variants_common.planted_segment with the variant stage's own records and slots; the others are random
planes as inserts_common.random_planes makes them, with windows, variant records and slots placed where the plan or the offsets can
go wrong: site_off and slot_off that do not begin at 0, a window at the first row of the call kernel's second step of 256 rows, an
interval across that step, 32 sites whose slot indices run to 63, a segment of one base, a group without members.

The issue that asked for this file names "a segment of rlen 256 (257 rows)" for the window that begins at row 256 and the interval
[250, 262).  Neither fits: a window needs lo < hi <= rlen.  The window that begins at row 256 stands in a segment of 257 bases, the
shortest that holds it, and the interval [250, 262) with a split site inside it in one of 262."""
import ctypes as C

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests import inserts_common as ic
from tests import splice_common as sc
from tests import splice_variants_common as svc
from tests import variants_common as vc

pytestmark = pytest.mark.gpu

L, A, B, N = api.INS_LACK, api.INS_CARRY, api.INS_CARRY_B, api.INS_NONE
MIN_DEPTH = 3


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _planted():
    """variants_common.planted_segment through the host's variant stage.  With 15 reads of nine different key2 only one isoform has
    the three direct reads the count asks for, so the groups here are the reads of one key2 each, in ascending order of the key:
    A and B at both split sites, NONE at the sites the short and the long read were re-keyed at, and the reads that lack everything.
    (frame, base, slots, group, win, var, slot strings, keys)"""
    reads, base, qpos, sites, keys = vc.planted_segment()
    got = api.insert_window_variants(base, qpos, [len(r) for r in reads], sites, keys, reads, **vc.PLANT)
    assert got["var"]["split"].tolist() == [1, 0, 0, 1, 0]
    distinct = sorted({int(k) for k in got["key2"]})
    return (reads[13], list(base), svc.plant_slots(reads, qpos), [distinct.index(int(k)) for k in got["key2"]], got["win"], got["var"],
            list(zip(got["seq"], got["qual"])), distinct)


def _segment(rng, rlen, reads_of_group, spans=(), split=(), lens=(), tlen=None, tlen_b=None, keys=()):
    """a random segment; lens holds the length of slot A and of slot B per site"""
    n = sum(reads_of_group)
    base = ic.random_planes(rng, n, rlen)[0] if n else np.zeros((0, rlen + 1), np.uint8)
    base[base > api.ALLELE_DEL] = api.ALLELE_NONE   # (the host's planes_pile refuses the bytes no projection writes)
    slots = rng.choice(np.array([0, 0, 0, 1, 2, 3, 4, 5], np.uint8), (n, _lib.PILE_INS_SLOTS, rlen + 1))
    group = [h for h, k in enumerate(reads_of_group) for _ in range(k)]
    rng.shuffle(group)
    frame = bytes(b"ACGTN"[x] for x in rng.integers(0, 5, rlen))
    ss = [sc.random_string(rng, k) for ab in lens for k in ab]
    return (frame, list(base), list(slots), group, sc.windows(list(spans), tlen), svc.variants(list(split), tlen_b), ss,
            [sc.key_of(k) for k in keys] or [0] * len(reads_of_group))


def _case():
    rng = np.random.default_rng(29)
    S = [_planted()]
    # a split site whose window begins at row 256, the first of the call kernel's second step: A, B, NONE and LACK there
    S.append(_segment(rng, 257, [3, 3, 2, 2], [(256, 257)], [1], [(8, 5)], keys=[[A], [B], [N], [L]]))
    # [250, 262) crosses the step and ends at rlen; the split site [256, 260) lies inside it and is OVERLAP wherever site 0 is DONE.
    # Site 0 does not split: B there is UNCALLED, and site 1 is taken.
    S.append(_segment(rng, 262, [3, 3, 2, 2, 0], [(250, 262), (256, 260)], [0, 1], [(40, 0), (8, 1)], tlen_b=[0, 3],
                      keys=[[A, A], [B, B], [N, A], [L, B], [A, B]]))       # the last group has no members: the frame around the window
    # 32 kept sites, all split, alternating A and B, all DONE: the plan is full and the slot indices run to 63
    S.append(_segment(rng, 100, [3, 2], [(1 + 3 * b, 4 + 3 * b) for b in range(32)], [1] * 32, [(int(x), int(y)) for x, y in rng.integers(0, 9, (32, 2))],
                      keys=[[A if b % 2 == 0 else B for b in range(32)], [B if b % 2 == 0 else A for b in range(32)]]))
    S.append(_segment(rng, 1, [3]))                                       # a segment of one base: no junction, no site
    return S


def _interleave(S):
    left = [list(range(len(s[1]))) for s in S]
    sop, group, base, slots = [], [], [], []
    while any(left):
        for g, s in enumerate(S):
            if left[g]:
                i = left[g].pop(0)
                sop.append(g), group.append(s[3][i]), base.append(s[1][i]), slots.append(s[2][i])
    return sop, group, base, slots


def _args(S):
    sop, group, base, slots = _interleave(S)
    return dict(frames=[s[0] for s in S], seg_of_pair=sop, group=group, n_groups=[len(s[7]) for s in S], base=base, slots=slots,
                iso_key=np.array([k for s in S for k in s[7]], np.uint64), win=[s[4] for s in S], var=[s[5] for s in S],
                slot_seq=[[w[0] for w in s[6]] for s in S], slot_qual=[[w[1] for w in s[6]] for s in S])


@pytest.fixture(scope="module")
def run(ctx):
    S = _case()
    args = _args(S)
    want = svc.host_isoforms_full_variants(min_depth=MIN_DEPTH, **args)
    got = ctx.planes_isoforms_full_variants(min_depth=MIN_DEPTH, tables=True, **args)
    return S, args, got, want


def test_every_group_segment_is_the_definition_as_bytes(run):
    _, _, got, want = run
    sc.same_full(got, want)
    assert all((r["reserved"] == 0).all() for r in got["splice"]) and (got["sstats"]["reserved"] == 0).all()


def test_the_case_holds_what_it_was_planted_for(run):
    S, args, _, want = run
    off = [int(x) for x in want["gseg_off"]]
    # the planted segment: its split sites are 0 and 3, some isoform counted again holds B at one of them and takes that slot
    states = [[(k >> (2 * b)) & 3 for b in range(5)] for k in S[0][7]]
    assert any(s[0] == B for s in states) and any(s[0] == A for s in states) and any(s[3] == B for s in states)
    for h, s in enumerate(states):
        rec = want["splice"][off[0] + h]
        assert [int(r) == sc.DONE for r in rec["state"]] == [x in (A, B) for x in s]
        for b in (0, 3):
            if s[b] in (A, B):
                assert int(rec[b]["len"]) == len(S[0][6][2 * b + (s[b] == B)][0]) > 0
    assert sum(len(w) for w in args["win"][:1]) == 5 and off[1] == len(S[0][7])   # site_off and slot_off of the segments behind begin at 5 and 10
    x = off[1]
    assert [want["splice"][x + h]["state"].tolist() for h in range(4)] == [[sc.DONE], [sc.DONE], [sc.LACK], [sc.LACK]]
    assert [int(want["splice"][x + h][0]["len"]) for h in range(2)] == [8, 5]
    x = off[2]
    assert [want["splice"][x + h]["state"].tolist() for h in range(5)] == [[sc.DONE, sc.OVERLAP], [sc.UNCALLED, sc.DONE], [sc.LACK, sc.DONE], [sc.LACK, sc.DONE],
                                                                           [sc.DONE, sc.OVERLAP]]
    assert [int(want["splice"][x + h][1]["len"]) for h in range(1, 4)] == [1, 8, 1]
    assert int(want["gpolish"][2][4]["n_low"]) == 262 - 12   # no members: the frame with quality 0 around the window
    x = off[3]
    assert all(int(want["sstats"][x + h]["n_done"]) == 32 and int(want["sstats"][x + h]["rows_replaced"]) == 96 for h in range(2))
    lens = [[len(S[3][6][2 * b + ((b + h) % 2)][0]) for b in range(32)] for h in range(2)]
    assert [want["splice"][x + h]["len"].tolist() for h in range(2)] == lens
    assert want["splice"][off[4]].size == 0 and len(want["sstats"]) == off[5]


def test_a_key_of_0_everywhere_gives_planes_polish_groups(ctx, run):
    _, args, _, _ = run
    plain = ctx.planes_polish_groups(args["frames"], args["seg_of_pair"], args["group"], args["n_groups"], args["base"], args["slots"], min_depth=MIN_DEPTH)
    none = ctx.planes_isoforms_full_variants(**{**args, "iso_key": np.zeros(len(args["iso_key"]), np.uint64)}, min_depth=MIN_DEPTH)
    assert none["gseq"] == plain["gseq"] and none["gqual"] == plain["gqual"]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(none["gpolish"], plain["gpolish"])) and int(none["sstats"]["n_done"].sum()) == 0
    assert all(int(r["state"].sum()) == 0 and (r["at"] == -1).all() for r in none["splice"])


def test_a_key_without_a_2_over_slots_that_hold_the_windows_is_planes_isoforms_full(ctx, run):
    _, args, _, _ = run
    keys = np.array([sc.key_of([s if s != B else (A, L, N)[b % 3] for b, s in enumerate((int(k) >> (2 * b)) & 3 for b in range(32))]) for k in args["iso_key"]], np.uint64)
    a = {**args, "iso_key": keys}
    byvar = ctx.planes_isoforms_full_variants(**a, min_depth=MIN_DEPTH, tables=True)
    var, sseq, squal = a.pop("var"), a.pop("slot_seq"), a.pop("slot_qual")
    parent = ctx.planes_isoforms_full(**a, win_seq=[s[0::2] for s in sseq], win_qual=[q[0::2] for q in squal], min_depth=MIN_DEPTH, tables=True)
    sc.same_full(byvar, parent)
    assert int(parent["sstats"]["n_done"].sum()) > 32


def test_the_empty_call(ctx):
    got = ctx.planes_isoforms_full_variants([], [], [], [], [], [], np.zeros(0, np.uint64), [], [], [], [])
    assert got["gseq"] == [] and got["off"].tolist() == [0] and got["splice_off"].tolist() == [0]
    # segments without a group, and groups without a site
    got = ctx.planes_isoforms_full_variants([b"ACGT"], [], [], [0], [], [], np.zeros(0, np.uint64), [sc.windows([(1, 2)])], [svc.variants([1])], [[b"A", b"C"]],
                                            [[b"I", b"I"]])
    assert got["gseq"] == [[]] and got["off"].tolist() == [0]


def _raw(ctx, args, cap, splice_cap, **swap):
    """the C entry itself over outputs filled with a mark: (status, anything written)"""
    a = {**args, **swap}
    frames, ns, n = a["frames"], len(a["frames"]), len(a["base"])
    rlen = np.array([len(f) for f in frames], np.int32)
    f_off = np.concatenate([[0], np.cumsum(rlen)]).astype(np.int64)
    sop, grp, ng = np.array(a["seg_of_pair"], np.int32), np.array(a["group"], np.int32), np.array(a["n_groups"], np.int32)
    fb = np.concatenate([np.asarray(b, np.uint8) for b in a["base"]])
    fs = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint8) for x in a["slots"]], axis=1))
    G = int(ng.sum())
    soff = np.concatenate([[0], np.cumsum([len(w) for w in a["win"]])]).astype(np.int64)
    wrec = np.concatenate([np.asarray(w, api.INSERT_WINDOW_DTYPE) for w in a["win"]])
    vrec = np.concatenate([np.asarray(v, api.WINDOW_VARIANT_DTYPE) for v in a["var"]])
    flat = [bytes(s) for g in range(ns) for s in a["slot_seq"][g]]
    slot_off = a.get("slot_off", np.concatenate([[0], np.cumsum([len(s) for s in flat])]).astype(np.int64))
    sseq, squal = b"".join(flat), b"".join(bytes(q) for g in range(ns) for q in a["slot_qual"][g])
    mark = lambda count, dt: np.frombuffer(bytes([0xEE]) * (max(count, 1) * np.dtype(dt).itemsize), dt).copy()
    seq, qual = mark(max(cap, 0) + 8, np.uint8), mark(max(cap, 0) + 8, np.uint8)
    off, spoff = mark(G + 1, np.int64), mark(G + 1, np.int64)
    pol, sst, rec = mark(G, api.POLISH_STATS_DTYPE), mark(G, api.SPLICE_STATS_DTYPE), mark(max(splice_cap, 0) + 8, api.SPLICE_SITE_DTYPE)
    outs = (seq, qual, off, spoff, pol, sst, rec)
    p = lambda x, t: x.ctypes.data_as(C.POINTER(t))
    keys = np.asarray(a["iso_key"], np.uint64)
    rc = ctx.L.ioc_planes_isoforms_full_variants(ctx.h, ns, p(rlen, C.c_int32), b"".join(frames), p(f_off, C.c_int64), p(ng, C.c_int32), n, p(sop, C.c_int32),
                                                 p(grp, C.c_int32), fb.ctypes.data, fs.ctypes.data, keys.ctypes.data, wrec.ctypes.data,
                                                 None if a.get("no_var") else vrec.ctypes.data, p(soff, C.c_int64), sseq, squal, p(np.ascontiguousarray(slot_off, np.int64), C.c_int64),
                                                 a.get("min_depth", MIN_DEPTH), seq.ctypes.data, qual.ctypes.data, cap, p(off, C.c_int64), pol.ctypes.data, sst.ctypes.data,
                                                 rec.ctypes.data, splice_cap, p(spoff, C.c_int64), None, None)
    return rc, any((x.view(np.uint8) != 0xEE).any() for x in outs), outs


def test_the_room_exactly_at_its_bounds_and_the_refusals(ctx, run):
    S, args, got, want = run
    bound = sum(len(s[7]) * api.isoform_splice_bound(len(s[0]), sum(len(w[0]) for w in s[6])) for s in S)   # the bytes of ALL slots of a segment
    records = int(got["splice_off"][-1])
    assert int(got["off"][-1]) <= bound and records == sum(len(s[7]) * len(s[4]) for s in S)
    sc.same_full(ctx.planes_isoforms_full_variants(**args, min_depth=MIN_DEPTH, tables=True, cap=bound, splice_cap=records), want)
    rc, written, outs = _raw(ctx, args, bound, records)
    assert rc == 0 and written and bytes(outs[0][:int(got["off"][-1])]) == b"".join(s for g in got["gseq"] for s in g)
    assert (outs[0][int(got["off"][-1]):] == 0xEE).all() and (outs[6][records:].view(np.uint8) == 0xEE).all()   # nothing behind what was called
    CAP, ARG = -4, -1
    assert _raw(ctx, args, bound - 1, records)[:2] == (CAP, False) and _raw(ctx, args, bound, records - 1)[:2] == (CAP, False)
    flat = [len(s) for g in args["slot_seq"] for s in g]
    off = np.concatenate([[0], np.cumsum(flat)]).astype(np.int64)
    down = off.copy()
    assert down[11] > 0
    down[12] = down[11] - 1                                         # slot 11, the B slot of the second segment's site, does not ascend
    for bad in (dict(no_var=True), dict(slot_off=down), dict(slot_off=off + 1), dict(min_depth=0),
                dict(var=[svc.variants([2]) if g == 1 else v for g, v in enumerate(args["var"])]),
                dict(var=[svc.variants([1], [-1]) if g == 1 else v for g, v in enumerate(args["var"])]),
                dict(win=[sc.windows([(256, 258)]) if g == 1 else w for g, w in enumerate(args["win"])])):     # hi > rlen
        assert _raw(ctx, args, bound, records, **bad)[:2] == (ARG, False), list(bad)
    with pytest.raises(api.IocError) as e:
        ctx.planes_isoforms_full_variants(**args, min_depth=MIN_DEPTH, cap=bound - 1)
    assert e.value.code == CAP
