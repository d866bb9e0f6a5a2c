"""A numpy restatement of the upper bound of totalMapped, from the header comment of ioc_resolve.hip — shared by the CPU
preconditions (tests/test_structured_host.py) and the device check (tests/test_gpu_structured.py).

totalMapped (src/cluster.cpp:324-353) adds the distance of two consecutive hits when the gap between their indices passes
pow(pError, gap) >= MinProbNoHits, the position of the first hit when its index passes, and the rest of the sequence behind
the last hit when the number of minimizers behind it passes.  With glim = the largest passing exponent of the (target cell,
query cell) pair (api.host_gap_limits) and lim = glim + 1, a candidate of Size H has
    totalMapped <= (H - 1) * D + head + tail,
    D    = max_i pos[min(i + lim, M - 1)] - pos[i]         (two counted hits are at most lim indices apart)
    head = max_{i < lim} pos[i]                            (a counted first hit has index <= glim)
    tail = max_{i >= M - lim} hpcLen - pos[i]              (a counted last hit has at most glim minimizers behind it)
per (query, strand, target cell)."""
import functools

import numpy as np

from isonclust2_amd import api


@functools.lru_cache(maxsize=None)
def _glim(k, w, min_prob_no_hits):
    return api.host_gap_limits(k, w, min_prob_no_hits)[0]               # [target cell - 1][query cell - 1]


def strand_bound_terms(pos, hpc_len, lim):
    """(D, head + tail) of one minimizer list (ascending positions `pos`) for the limit `lim` = glim + 1 (0: nothing counts)"""
    pos = np.asarray(pos, np.int64)
    M = len(pos)
    if M == 0 or lim <= 0:
        return 0, 0
    j = np.minimum(np.arange(M) + lim, M - 1)
    D = int((pos[j] - pos).max())
    m = min(int(lim), M)
    head = int(pos[:m].max())
    tail = int(np.maximum(int(hpc_len) - pos[M - m:], 0).max())
    return D, head + tail


class MappedBound:
    """The bound for the candidates of the queries of `view` (fields of ioc_batch_view).  target_cells[t]: the error cell
    (api.host_err_cell, 1..15; 0 = none) of the representative of target t, in whatever numbering the caller's targets use."""

    def __init__(self, view, k, w, target_cells, min_prob_no_hits=0.1):
        self.view = view
        self.glim = _glim(int(k), int(w), float(min_prob_no_hits))
        self.tcell = np.asarray(target_cells, np.int64)
        self._terms = {}

    def terms(self, q, strand, tcell):
        key = (int(q), int(strand), int(tcell))
        if key not in self._terms:
            v = self.view
            off = v["off_fwd"] if strand == 1 else v["off_rev"]
            pos = np.asarray(v["min_pos"])[int(off[q]):int(off[q + 1])]
            qcell = api.host_err_cell(float(v["hpc_err"][q]))
            assert 1 <= qcell <= 15 and 1 <= tcell <= 15, (q, qcell, tcell)
            self._terms[key] = strand_bound_terms(pos, int(v["hpc_len"][q]), int(self.glim[tcell - 1, qcell - 1]) + 1)
        return self._terms[key]

    def __call__(self, q, target, strand, size):
        """the bound of totalMapped of query q's candidate (target, strand +1 / -1) of Size `size`"""
        D, ht = self.terms(q, strand, int(self.tcell[target]))
        return (int(size) - 1) * D + ht


def size_floor(view, q, k, w, need, keep, min_prob_no_hits=0.1):
    """The per-query cut of the candidate lists (fast mode; k_gap_bounds' keep_q) restated: the smallest Size that reaches `need`
    by SOME bound of query q — either strand, any of the 15 target cells — or `keep` (the Size rule's own cut, ioc_set_params)
    where that is larger.  A candidate of a smaller Size is cut from the list and exported as rejected.
        (Size - 1) * D + ht >= need   <=>   Size >= ceil((need - ht) / D) + 1   (0 when ht alone reaches need, never when D = 0)"""
    glim = _glim(int(k), int(w), float(min_prob_no_hits))
    qcell = api.host_err_cell(float(view["hpc_err"][q]))
    assert 1 <= qcell <= 15, (q, qcell)
    smin = None
    for off in (view["off_fwd"], view["off_rev"]):
        pos = np.asarray(view["min_pos"])[int(off[q]):int(off[q + 1])]
        if len(pos) == 0:
            continue
        for tcell in range(1, 16):
            D, ht = strand_bound_terms(pos, int(view["hpc_len"][q]), int(glim[tcell - 1, qcell - 1]) + 1)
            if need <= ht:
                thr = 0
            elif D:
                thr = -(-(int(need) - ht) // D) + 1
            else:
                continue
            smin = thr if smin is None else min(smin, thr)
    return int(keep) if smin is None or smin <= keep else int(smin)


def entry_cells(view):
    """target_cells for MappedBound, targets numbered by ENTRY (the device's targets of a single batch, L = 0)"""
    return np.array([api.host_err_cell(float(e)) for e in view["hpc_err"]], np.int64)


def single_batch_cells(view, cls):
    """target_cells for MappedBound, targets numbered by CLUSTER ID of a single-batch run: the representative of cluster c
    is the first entry (in loop order) assigned to it.  cls: cluster of every entry (-1: none)."""
    cls = np.asarray(cls)
    n_cls = int(cls.max()) + 1 if len(cls) else 0
    cells = np.zeros(n_cls, np.int64)
    seen = np.zeros(n_cls, bool)
    for e, c in enumerate(cls.tolist()):
        if c >= 0 and not seen[c]:
            seen[c] = True
            cells[c] = api.host_err_cell(float(view["hpc_err"][e]))
    return cells


def slack_counts(bound, view, rows, thr=0.65):
    """Over the oracle's trace rows: (rows, rows whose exact total exceeds the bound, bound-rejected rows with bound >= 0.8 need,
    unrejected failing rows with bound < 1.25 need) — need = api.host_min_total of the query."""
    unsound = near_rej = near_unrej = 0
    need_of = {}
    for e, c, s, sz, tot in zip(rows["entry"].tolist(), rows["cls"].tolist(), rows["strand"].tolist(), rows["size"].tolist(),
                                rows["total_mapped"].tolist()):
        if e not in need_of:
            need_of[e] = api.host_min_total(int(view["hpc_len"][e]), thr)
        need = need_of[e]
        b = bound(e, c, s, sz)
        unsound += b < tot
        if b < need:
            near_rej += 5 * b >= 4 * need            # bound >= 0.8 need
        elif tot < need:
            near_unrej += 4 * b < 5 * need           # bound < 1.25 need
    return len(rows["entry"]), int(unsound), int(near_rej), int(near_unrej)


def subset_view(view, entries):
    """the fields the bound reads (offsets, positions, lengths, error rates) of these entries of `view`, renumbered 0..: the
    representatives of a fast-mode clustering are the entries that opened its clusters"""
    entries = np.asarray(entries, np.int64)
    out = dict(hpc_len=np.asarray(view["hpc_len"])[entries], hpc_err=np.asarray(view["hpc_err"])[entries])
    pos, base = [], 0
    for key in ("off_fwd", "off_rev"):
        off = np.asarray(view[key])
        lens = off[entries + 1] - off[entries]
        out[key] = base + np.concatenate([[0], np.cumsum(lens)])
        pos += [np.asarray(view["min_pos"])[int(off[e]):int(off[e + 1])] for e in entries]
        base = int(out[key][-1])
    out["min_pos"] = np.concatenate(pos) if pos else np.zeros(0, np.uint32)
    return out


def openers(cls):
    """the entry that opened every cluster of a single-batch run (the first one assigned to it)"""
    cls = np.asarray(cls)
    first = np.full(int(cls.max()) + 1 if len(cls) else 0, -1, np.int64)
    for e in range(len(cls) - 1, -1, -1):
        if cls[e] >= 0:
            first[cls[e]] = e
    return first


def in_walk_rejections(bound, view, rows, k, w, thr=0.65, min_shared=5, min_fraction=0.8, only=None):
    """The oracle's trace rows for which the device MUST consult the bound in its sweeps (k_decide_scan's bound_rejects) and it
    rejects: candidates in reach of the walk (Size >= int(top * MinFraction), top >= MinShared) of a query none of whose walk
    candidates passes (so the sweeps go through the whole walk, not only the top Size), that survive the list cut
    (Size >= size_floor) with a bound below the query's threshold.  only: a mask over the rows to count (e.g. left targets)."""
    keep = max(1, min(int(min_shared * min_fraction), min_shared))
    ent, size, tot = rows["entry"].tolist(), rows["size"].tolist(), rows["total_mapped"].tolist()
    top, need, decided = {}, {}, set()
    for e, z in zip(ent, size):
        top[e] = max(top.get(e, 0), z)
    reach = [top[e] >= min_shared and z >= int(float(top[e]) * min_fraction) for e, z in zip(ent, size)]
    for i, e in enumerate(ent):
        if e not in need:
            need[e] = api.host_min_total(int(view["hpc_len"][e]), thr)
        if reach[i] and tot[i] >= need[e]:
            decided.add(e)
    n, floor = 0, {}
    for i, (e, c, s, z) in enumerate(zip(ent, rows["cls"].tolist(), rows["strand"].tolist(), size)):
        if not reach[i] or e in decided or (only is not None and not only[i]):
            continue
        if e not in floor:
            floor[e] = size_floor(view, e, k, w, need[e], keep)
        n += z >= floor[e] and bound(e, c, s, z) < need[e]
    return int(n)
