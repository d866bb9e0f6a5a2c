"""What the tests of the groups' consensus share (test_plane_pile_host.py, test_gpu_planes_polish.py,
test_gpu_align_split_polish.py, test_cli_split_polish.py): plain-Python restatements of the two definitions —
ioc_host_ops_project_ins byte by byte, ioc_host_planes_pile byte by byte — which are the independent witness for the host functions
and, through them, for the kernels; and the definition of the feature itself, group-segment by group-segment, from the host
functions."""
import numpy as np

from isonclust2_amd import api
from tests import polish_common as pc

SLOTS = pc.SLOTS
NONE, DEL = 7, 5
SPLIT_NONE = 255
BASE_BYTES = (0, 1, 2, 3, 4, DEL, NONE)   # what ioc_host_ops_project writes
SLOT_BYTES = (0, 1, 2, 3, 4, 5)           # what ioc_host_ops_project_ins writes


def py_project_ins(ops, query, rlen):
    """The walk of ioc_host_ops_project_ins, byte by byte: SLOTS lists of rlen + 1 values."""
    slots = [[0] * (rlen + 1) for _ in range(SLOTS)]
    r = q = j = 0
    for op in bytes(ops):
        op = chr(op)
        if op == "I":
            if j < SLOTS:
                slots[j][r] = 1 + pc.CH.get(query[q], 4)
            j, q = j + 1, q + 1
            continue
        j = 0
        q += op in "=Xi"
        r += op in "=XDd"
    assert (q, r) == (len(query), rlen)
    return slots


def py_planes_pile(base, slots, cols, ins):
    """ioc_host_planes_pile, byte by byte, ADDED to cols / ins in place (numpy records; Python integers in between)."""
    rows = len(base)
    assert all(int(b) in BASE_BYTES for b in base) and all(int(s) in SLOT_BYTES for j in range(SLOTS) for s in slots[j])
    for r in range(rows):
        b = int(base[r])
        if b != NONE:
            f = pc.COL_FIELDS[b]
            cols[f][r] = int(cols[f][r]) + 1
        for j in range(SLOTS):
            s = int(slots[j][r])
            if s == 0:
                continue
            ins["slot"][r, j, s - 1] = int(ins["slot"][r, j, s - 1]) + 1
            cols["ins_bases"][r] = int(cols["ins_bases"][r]) + 1
            if j == 0:
                cols["ins_runs"][r] = int(cols["ins_runs"][r]) + 1
    return cols, ins


def runs_per_row_at_most_one(ops):
    """No row of the string has two runs of 'I' in front of it (every aligner's string; not every random one)."""
    seen, r, prev = set(), 0, None
    for op in bytes(ops):
        op = chr(op)
        if op == "I" and prev != "I":
            if r in seen:
                return False
            seen.add(r)
        r += op in "=XDd"
        prev = op
    return True


def ins_run_lengths(ops):
    """{row: [lengths of the runs of 'I' in front of it]}"""
    out, r, run = {}, 0, 0
    for op in bytes(ops) + b"=":
        op = chr(op)
        if op == "I":
            run += 1
            continue
        if run:
            out.setdefault(r, []).append(run)
            run = 0
        r += op in "=XDd"
    return out


def planes_of(ops, query, rlen):
    """(base, slots) of one string through the host functions."""
    return api.ops_project(ops, query, rlen)[0], api.ops_project_ins(ops, query, rlen)


def host_group_polish(frames, seg_of_pair, group, base, slots, min_depth):
    """The definition of the feature from the host functions: group-segment 2 g + h is pileup_call of frame g on the tables
    planes_pile adds up from the pairs of segment g whose group byte is h.  Returns a dict like Context.planes_polish's with
    tables=True."""
    ns = len(frames)
    gseq, gqual, gpol, gcols, gins = [], [], np.zeros((ns, 2), api.POLISH_STATS_DTYPE), [], []
    for g, frame in enumerate(frames):
        gseq.append([]), gqual.append([])
        for h in (0, 1):
            cols, ins = np.zeros(len(frame) + 1, api.PILEUP_DTYPE), np.zeros(len(frame) + 1, api.PILEUP_INS_DTYPE)
            for i in range(len(base)):
                if seg_of_pair[i] == g and group[i] == h:
                    api.planes_pile(base[i], slots[i], cols=cols, ins=ins)
            s, q, st = api.pileup_call(cols, ins, frame, min_depth)
            gseq[g].append(s), gqual[g].append(q)
            for f in api.POLISH_STATS_FIELDS:
                gpol[g, h][f] = st[f]
            gcols.append(cols), gins.append(ins)
    cat = lambda parts, dt: np.concatenate([np.zeros(0, dt)] + parts)
    return {"gseq": gseq, "gqual": gqual, "gpolish": gpol, "gcols": cat(gcols, api.PILEUP_DTYPE), "gins": cat(gins, api.PILEUP_INS_DTYPE)}


def same_polish(got, want, tables=True):
    assert got["gseq"] == want["gseq"] and got["gqual"] == want["gqual"]
    assert got["gpolish"].tobytes() == want["gpolish"].tobytes()
    if tables:
        assert got["gcols"].tobytes() == want["gcols"].tobytes() and got["gins"].tobytes() == want["gins"].tobytes()
