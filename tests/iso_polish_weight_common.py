"""What the tests of the quality-weighted consensus of every isoform share (test_planes_weights_host.py,
test_gpu_planes_polish_groups_weighted.py, test_gpu_align_blocks_polish_weighted.py, test_cli_isoforms_polish_weighted.py):
plain-Python restatements of the two definitions — ioc_host_ops_project_weights byte by byte, ioc_host_planes_pile_weighted byte
by byte, in Python's unbounded integers reduced modulo 2^32 — as the independent witness, and the definition of the feature from
the host functions: group-segment (g, h) is pileup_call_weighted of frame g on the counts planes_pile adds up and the weights
planes_pile_weighted adds up from the pairs of segment g whose group is h."""
import numpy as np

from isonclust2_amd import api
from tests import iso_polish_common as ic
from tests import plane_pile_common as pp
from tests import polish_common as pc
from tests import polish_weight_common as pw

SLOTS, M32 = pp.SLOTS, pc.M32


def py_project_weights(ops, query, qual, rlen):
    """The walk of ioc_host_ops_project_weights, byte by byte: (wbase, wslots), rlen + 1 values and SLOTS lists of them."""
    qlen = len(query)
    assert len(qual) == qlen
    wbase, wslots = [0] * (rlen + 1), [[0] * (rlen + 1) for _ in range(SLOTS)]
    r = q = j = 0
    for op in bytes(ops):
        op = chr(op)
        if op == "I":
            if j < SLOTS:
                wslots[j][r] = pw.py_weight(qual[q])
            j, q = j + 1, q + 1
            continue
        j = 0
        if op in "=X":
            wbase[r] = pw.py_weight(qual[q])
        elif op == "D":
            near = ([pw.py_weight(qual[q - 1])] if q > 0 else []) + ([pw.py_weight(qual[q])] if q < qlen else [])
            wbase[r] = min(near) if near else 1
        q += op in "=Xi"
        r += op in "=XDd"
    assert (q, r) == (qlen, rlen)
    return wbase, wslots


def py_planes_pile_weighted(base, slots, wbase, wslots, wcols, wins):
    """ioc_host_planes_pile_weighted, byte by byte, ADDED (modulo 2^32) to wcols / wins in place."""
    rows = len(base)
    assert all(int(b) in pp.BASE_BYTES for b in base) and all(int(s) in pp.SLOT_BYTES for j in range(SLOTS) for s in slots[j])
    for r in range(rows):
        b = int(base[r])
        if b != pp.NONE:
            f = pc.COL_FIELDS[b]
            wcols[f][r] = (int(wcols[f][r]) + int(wbase[r])) & M32
        for j in range(SLOTS):
            s = int(slots[j][r])
            if s:
                wins["slot"][r, j, s - 1] = (int(wins["slot"][r, j, s - 1]) + int(wslots[j][r])) & M32
    return wcols, wins


def planes_of(ops, query, qual, rlen):
    """(base, slots, wbase, wslots) of one string through the host functions."""
    return pp.planes_of(ops, query, rlen) + api.ops_project_weights(ops, query, qual, rlen)


def host_planes(frame, reads, quals, e=0.1):
    """every read's four planes through the host aligner and the three host projections: (base, slots, wbase, wslots), a list each"""
    out = ([], [], [], [])
    for rd, ql in zip(reads, quals):
        ops, _ = api.host_align_ops(rd, frame, gap_open=pc.gap_open(e))
        for lst, plane in zip(out, planes_of(ops, rd, ql, len(frame))):
            lst.append(plane)
    return out


def host_groups_polish_weighted(frames, seg_of_pair, group, n_groups, base, slots, wbase, wslots, min_depth):
    """The definition from the host functions, walked through the grouped member lists.  Returns a dict like
    Context.planes_polish_groups_weighted's with tables=True."""
    ns = len(frames)
    gseg_off, gmem_off, gmembers = ic.py_group_member_lists(ns, seg_of_pair, group, n_groups)
    gseq, gqual, gpol, gcols, gwcols, gwins, grow0 = [], [], [], [], [], [], []
    rows = 0
    for g, frame in enumerate(frames):
        gseq.append([]), gqual.append([])
        pol = np.zeros(int(n_groups[g]), api.POLISH_STATS_DTYPE)
        for h in range(int(n_groups[g])):
            x = gseg_off[g] + h
            n = len(frame) + 1
            cols, ins = np.zeros(n, api.PILEUP_DTYPE), np.zeros(n, api.PILEUP_INS_DTYPE)
            wcols, wins = np.zeros(n, api.PILEUP_DTYPE), np.zeros(n, api.PILEUP_INS_DTYPE)
            for i in gmembers[gmem_off[x]:gmem_off[x + 1]]:
                api.planes_pile(base[i], slots[i], cols=cols, ins=ins)
                api.planes_pile_weighted(base[i], slots[i], wbase[i], wslots[i], wcols=wcols, wins=wins)
            s, q, st = api.pileup_call_weighted(cols, wcols, wins, frame, min_depth)
            gseq[g].append(s), gqual[g].append(q)
            for f in api.POLISH_STATS_FIELDS:
                pol[h][f] = st[f]
            gcols.append(cols), gwcols.append(wcols), gwins.append(wins), grow0.append(rows)
            rows += n
        gpol.append(pol)
    cat = lambda parts, dt: np.concatenate([np.zeros(0, dt)] + parts)
    return {"gseq": gseq, "gqual": gqual, "gpolish": gpol, "gseg_off": np.array(gseg_off, np.int64), "gcols": cat(gcols, api.PILEUP_DTYPE),
            "gwcols": cat(gwcols, api.PILEUP_DTYPE), "gwins": cat(gwins, api.PILEUP_INS_DTYPE), "grow0": np.array(grow0, np.int64)}


def same_groups_weighted(got, want, tables=True):
    """a result of Context.planes_polish_groups_weighted (or the isoform part of the fused call) against the definition, as bytes"""
    ic.same_groups(got, want, tables=False)
    if tables:
        for f in ("gcols", "gwcols", "gwins"):
            assert got[f].tobytes() == want[f].tobytes(), f
        assert got["grow0"].tolist() == want["grow0"].tolist()
