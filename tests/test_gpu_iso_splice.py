"""The kernels of ioc_iso_splice.hip against the host definition, as bytes, through ioc_planes_isoforms_full: sequences, qualities,
offsets, the polish, splice and site records and the group tables on planted planes — random planes as inserts_common.random_planes
makes them (no alignment is needed), windows of random strings placed where a wave, a chunk of IOC_PILE_CALL_CHUNK rows and the
scan's step of 64 group-segments end."""
import numpy as np
import pytest

from isonclust2_amd import api
from tests import inserts_common as ic
from tests import splice_common as sc

pytestmark = pytest.mark.gpu

L, C, N = api.INS_LACK, api.INS_CARRY, api.INS_NONE
LONG = api.pileup_call_bound(api.WIN_MAX)   # 3590: what a window of max_win 512 may hold
MIN_DEPTH = 3                               # with 2 .. 5 reads a group, random gaps and uncovered bytes, some rows of every group are low


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _segment(rng, rlen, reads_of_group, spans=(), lens=(), tlen=None, keys=()):
    """(frame, base planes, slot planes, group per read, windows, (sequence, qualities) per site, key per group)"""
    n = sum(reads_of_group)
    base = ic.random_planes(rng, n, rlen)[0] if n else np.zeros((0, rlen + 1), np.uint8)
    base[base > api.ALLELE_DEL] = api.ALLELE_NONE   # (the host's planes_pile refuses the bytes no projection writes)
    slots = rng.choice(np.array([0, 0, 0, 1, 2, 3, 4, 5], np.uint8), (n, api._lib.PILE_INS_SLOTS, rlen + 1))
    group = [h for h, k in enumerate(reads_of_group) for _ in range(k)]
    rng.shuffle(group)
    frame = bytes(b"ACGTN"[x] for x in rng.integers(0, 5, rlen))
    ws = [sc.random_string(rng, k) for k in lens]
    return frame, list(base), list(slots), group, sc.windows(list(spans), tlen), ws, [sc.key_of(k) for k in keys] or [0] * len(reads_of_group)


def _case():
    rng = np.random.default_rng(23)
    S = []
    S.append(_segment(rng, 1, [3]))                                                        # no junction: a segment with no site
    S.append(_segment(rng, 63, [3, 3], [(1, 63)], [8], keys=[[C], [L]]))                    # lo = 1 and hi = rlen: only row 0 and row rlen's insertions stay
    S.append(_segment(rng, 64, [4, 0], [(60, 64)], [1], keys=[[C], [C]]))                   # hi = rlen at a wave's end; group 1 has no reads
    S.append(_segment(rng, 255, [3], [(250, 255)], [0], keys=[[C]]))                        # a called window of no bytes; row 255 ends the chunk
    S.append(_segment(rng, 256, [3], [(250, 256)], [LONG], keys=[[C]]))                     # hi = rlen: row 256, the next chunk's first, follows the window
    S.append(_segment(rng, 257, [3], [(256, 257)], [8], keys=[[C]]))                        # a window that begins at a chunk's first row
    # three chunks.  Site 0 straddles a wave boundary, 1 a chunk boundary, 2 begins at a chunk's first row and overlaps 1, 3 is not
    # called, 5 is called with no bytes, 6 ends at rlen.  Two long windows begin in chunk 0.
    spans = [(60, 70), (250, 262), (256, 270), (300, 310), (400, 420), (580, 585), (590, 600)]
    S.append(_segment(rng, 600, [4, 5, 0, 3, 2], spans, [LONG, LONG, 8, 0, 1, 0, 8], tlen=[9, 9, 9, 0, 9, 9, 9],
                      keys=[[C, C, C, C, L, C, C],      # all four states: done, done, overlap, uncalled, lack, done, done
                            [C, L, C, N, C, 2, C],      # site 2 done: rows 256 .. 269 go
                            [C] * 7,                    # no reads: the frame around the windows
                            [L] * 7,                    # nothing carried: the call itself
                            [L, C, C, C, C, C, C]]))
    S.append(_segment(rng, 100, [3, 2], [(1 + 3 * b, 4 + 3 * b) for b in range(32)], [int(x) for x in rng.integers(0, 9, 32)],
                      keys=[[C] * 32, [C if b % 2 else L for b in range(32)]]))             # 32 sites, all done, back to back
    S.append(_segment(rng, 5, [1 + h % 2 for h in range(130)], [(2, 4)], [8],
                      keys=[[C] if h % 3 else [L] for h in range(130)]))                    # 130 group-segments: the scan carries across steps of 64
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


@pytest.fixture(scope="module")
def run(ctx):
    S = _case()
    sop, group, base, slots = _interleave(S)
    args = dict(frames=[s[0] for s in S], seg_of_pair=sop, group=group, n_groups=[len(s[6]) for s in S], base=base, slots=slots,
                iso_key=np.array([k for s in S for k in s[6]], np.uint64), win=[s[4] for s in S], win_seq=[[w[0] for w in s[5]] for s in S],
                win_qual=[[w[1] for w in s[5]] for s in S])
    want = sc.host_isoforms_full(min_depth=MIN_DEPTH, **args)
    got = ctx.planes_isoforms_full(min_depth=MIN_DEPTH, tables=True, **args)
    return S, args, got, want


def test_every_group_segment_is_the_definition_as_bytes(run):
    _, _, got, want = run
    sc.same_full(got, want)


def test_the_case_holds_what_it_was_planted_for(run):
    S, _, _, want = run
    x600 = int(want["gseg_off"][6])
    assert want["splice"][x600]["state"].tolist() == [sc.DONE, sc.DONE, sc.OVERLAP, sc.UNCALLED, sc.LACK, sc.DONE, sc.DONE]
    assert want["splice"][x600 + 1]["state"].tolist() == [sc.DONE, sc.LACK, sc.DONE, sc.LACK, sc.DONE, sc.LACK, sc.DONE]
    assert int(want["sstats"][x600]["spliced_bytes"]) == 2 * LONG + 8 and int(want["sstats"][x600]["rows_replaced"]) == 10 + 12 + 5 + 10
    assert int(want["sstats"][int(want["gseg_off"][7])]["n_done"]) == 32 and len(want["sstats"]) == 1 + 2 + 2 + 1 + 1 + 1 + 5 + 2 + 130
    low = [int(p["n_low"]) for g in want["gpolish"] for p in g]
    assert sum(v > 0 for v in low) > len(low) // 2 and any(int(p["n_ins"]) > 0 for g in want["gpolish"] for p in g)
    # a group without reads: its frame with quality 0 around the windows
    assert int(want["gpolish"][6][2]["n_low"]) == 600 - (10 + 12 + 20 + 5 + 10)


def test_a_key_that_carries_nothing_gives_planes_polish_groups(ctx, run):
    _, args, got, _ = run
    plain = ctx.planes_polish_groups(args["frames"], args["seg_of_pair"], args["group"], args["n_groups"], args["base"], args["slots"], min_depth=MIN_DEPTH)
    x = int(got["gseg_off"][6]) + 3
    assert got["gseq"][6][3] == plain["gseq"][6][3] and got["gpolish"][6][3].tobytes() == plain["gpolish"][6][3].tobytes()
    none = ctx.planes_isoforms_full(**{**args, "iso_key": np.zeros(len(args["iso_key"]), np.uint64)}, min_depth=MIN_DEPTH)
    assert none["gseq"] == plain["gseq"] and none["gqual"] == plain["gqual"]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(none["gpolish"], plain["gpolish"])) and int(none["sstats"]["n_done"].sum()) == 0
    assert int(got["splice"][x]["state"].sum()) == 0


def test_refusals(ctx, run):
    _, args, got, _ = run
    need = int(got["off"][-1])
    bound = sum(len(s[6]) * api.isoform_splice_bound(len(s[0]), sum(len(w[0]) for w in s[5])) for s in run[0])
    assert need <= bound
    for kw in (dict(cap=bound - 1), dict(splice_cap=int(got["splice_off"][-1]) - 1)):
        with pytest.raises(api.IocError) as e:
            ctx.planes_isoforms_full(**args, min_depth=MIN_DEPTH, **kw)
        assert e.value.code == -4
    for bad in (dict(win=[sc.windows([(0, 1)]) if len(w) == 1 and g == 1 else w for g, w in enumerate(args["win"])]),   # lo < 1
                dict(win=[sc.windows([(60, 65)]) if g == 2 else w for g, w in enumerate(args["win"])]),                # hi > rlen
                dict(min_depth=0)):
        with pytest.raises(api.IocError) as e:
            ctx.planes_isoforms_full(**{**args, "min_depth": MIN_DEPTH, **bad})
        assert e.value.code == -1
    sc.same_full(ctx.planes_isoforms_full(**args, min_depth=MIN_DEPTH, tables=True, cap=bound, splice_cap=int(got["splice_off"][-1])), run[3])
