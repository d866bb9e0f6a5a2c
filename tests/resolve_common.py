"""The greedy loop's bookkeeping restated sequentially (src/cluster.cpp:355-406, 481-489, 545-567), as the reference for what
ioc_resolve returns besides the decisions — the cuts, the tie sets and the flag byte — plus the builders of the crafted
inputs of tests/test_resolve_host.py and tests/test_gpu_resolve_outputs.py and the comparison both share.

Nothing here looks at the device: Size is a plain membership count, the loop runs over the queries in order, and whether a
candidate passes the mapped-fraction test is the caller's callback (for the crafted inputs it depends on `need` alone)."""
import numpy as np

INT32_MAX = 2 ** 31 - 1
NO_VERDICT = -2 ** 31
NEED_ALL, NEED_NONE = 0, 1 << 30           # min_total every candidate passes / no candidate passes (above every hpc_len)
WALK_SLOTS, TIE_SLOTS, SCAN_ITEMS, SCAN_REGS = 32, 16, 256, 8 * 256      # ioc_kernels.h, ioc_resolve.hip
K = 11


def list_keep(min_shared, min_fraction):
    """Size below which ioc_score leaves a candidate out of the lists (ioc_set_params): it can never be walked."""
    if 0.0 <= min_fraction <= 1.0 and min_shared > 0:
        return max(1, min(int(float(min_shared) * min_fraction), min_shared))
    return 1


def cut_of(top, min_fraction):
    return int(float(top) * min_fraction)


def cut_of_f32(top, min_fraction):
    """What a 32-bit float product would give: the tests place tops where it differs from cut_of."""
    return int(np.float32(top) * np.float32(min_fraction))


class Restated:
    """Per query: target, strand, flags, cut, ties (a set of keys), top, and the counts the path assertions use — n_cand (list
    entries, clusters or not), walk (cluster candidates with Size >= min(cut, top)), items (cluster candidates with Size >=
    cut), pass_keys (the passing candidates at the winner's Size win_size) — and, with tables=True, cands: (target, strand, Size) of
    the candidates that are clusters when the loop reaches the query."""

    def __init__(self, n):
        self.target = np.full(n, -1, np.int32)
        self.strand = np.zeros(n, np.int8)
        self.flags = np.zeros(n, np.uint8)
        self.cut = np.full(n, INT32_MAX, np.int32)
        self.top = np.zeros(n, np.int64)
        self.ties = [frozenset() for _ in range(n)]
        self.pass_keys = [frozenset() for _ in range(n)]
        self.n_cand = np.zeros(n, np.int64)
        self.walk = np.zeros(n, np.int64)
        self.items = np.zeros(n, np.int64)
        self.win_size = np.zeros(n, np.int64)
        self.cands = [None] * n

    @property
    def n_ties(self):
        return np.array([len(t) for t in self.ties], np.int64)


def greedy_resolve(n, L, fwd, rev, left_sets, need, min_shared, min_fraction, forced=None, verdict_t=None, verdict_s=None,
                   passes=None, tables=False):
    """fwd / rev: per query its forward / reverse minimizer values in list order; left_sets: per left cluster its forward
    values; forced: {query: -1 | -2 | (target, strand)}; verdict_t / verdict_s: per query NO_VERDICT, -1 or a target and its
    strand; passes(q, target, strand, size) -> bool (default: need[q] == 0).  Targets: left cluster t < L, or L + the query
    that opened the cluster."""
    forced = forced or {}
    if passes is None:
        passes = lambda q, t, s, z: need[q] == 0     # noqa: E731
    lists = [np.asarray(x, np.int64) for x in list(left_sets) + list(fwd) + list(rev)]
    vals = np.unique(np.concatenate(lists)) if lists else np.zeros(0, np.int64)
    ident = lambda x: np.searchsorted(vals, np.asarray(x, np.int64))     # noqa: E731
    T = L + n
    member = np.zeros((T, max(len(vals), 1)), bool)       # member[t, v]: value v is in target t's forward set
    for t in range(L):
        member[t, ident(left_sets[t])] = True
    fid, rid = [ident(x) for x in fwd], [ident(x) for x in rev]
    for j in range(n):
        member[L + j, fid[j]] = True
    is_cluster = np.zeros(T, bool)
    is_cluster[:L] = True
    keep = list_keep(min_shared, min_fraction)
    R = Restated(n)
    for j in range(n):
        Tn = L + j
        # Size: the entries of the query's list whose value the target holds, one count per entry
        size = np.concatenate([member[:Tn, fid[j]].sum(1), member[:Tn, rid[j]].sum(1)]).astype(np.int64)
        tgt = np.concatenate([np.arange(Tn), np.arange(Tn)])
        rbit = np.concatenate([np.zeros(Tn, np.int64), np.ones(Tn, np.int64)])
        R.n_cand[j] = int((size >= keep).sum())
        live = is_cluster[tgt] & (size > 0)
        if tables:
            R.cands[j] = (tgt[live], np.where(rbit[live] == 1, -1, 1), size[live])
        if j in forced:
            f = forced[j]
            if f == -1 or f == -2:
                R.target[j] = f
                is_cluster[L + j] = f == -1
            else:
                R.target[j], R.strand[j] = f
            continue
        top = int(size[live].max()) if live.any() else 0
        if top == 0 or top < min_shared:
            is_cluster[L + j] = True
            continue
        cut = cut_of(top, min_fraction)
        R.top[j], R.cut[j] = top, cut
        key = (tgt << 1) | rbit
        R.ties[j] = frozenset(key[live & (size == top)].tolist())
        R.walk[j] = int((live & (size >= min(cut, top))).sum())
        R.items[j] = int((live & (size >= cut)).sum())
        won = None
        for z in sorted(set(size[live & (size >= cut)].tolist()), reverse=True):
            at = np.flatnonzero(live & (size == z))
            ok = [int(c) for c in at if passes(j, int(tgt[c]), -1 if rbit[c] else 1, z)]
            if ok:
                won, R.win_size[j] = ok, z
                break
        if won:
            R.pass_keys[j] = frozenset(int(key[c]) for c in won)
            c = won[0]
            R.target[j], R.strand[j] = int(tgt[c]), -1 if rbit[c] else 1
            R.flags[j] = 1 if len(won) > 1 else 0
            continue
        R.flags[j] = 2
        vt = NO_VERDICT if verdict_t is None else int(verdict_t[j])
        if vt != NO_VERDICT and vt >= 0:
            R.target[j], R.strand[j] = vt, int(verdict_s[j])
        else:
            is_cluster[L + j] = True
    return R


def compare(R, dec, cuts, ties, where=None):
    """The device's decisions(), cuts() and ties() against the restatement; every comparison is of integers.  where: the
    queries to compare (default: all)."""
    t, s, f = dec
    count, keys = ties
    n = len(R.target)
    assert len(t) == len(cuts) == len(count) == n
    idx = np.arange(n) if where is None else np.asarray(where)
    bad = idx[cuts[idx] != R.cut[idx]]
    assert not len(bad), ("cut", bad[:8].tolist(), cuts[bad[:8]].tolist(), R.cut[bad[:8]].tolist())
    bad = idx[f[idx] != R.flags[idx]]
    assert not len(bad), ("flags", bad[:8].tolist(), f[bad[:8]].tolist(), R.flags[bad[:8]].tolist())
    nt = R.n_ties
    bad = idx[count[idx] != nt[idx]]
    assert not len(bad), ("tie count", bad[:8].tolist(), count[bad[:8]].tolist(), nt[bad[:8]].tolist())
    for j in idx.tolist():
        got = keys[j, :min(int(count[j]), TIE_SLOTS)].tolist()
        if count[j] <= TIE_SLOTS:
            assert sorted(got) == sorted(R.ties[j]), ("tie keys", j, sorted(got), sorted(R.ties[j]))
        else:
            assert len(set(got)) == TIE_SLOTS and set(got) <= R.ties[j], ("tie keys", j, sorted(got))
        if f[j] & 1:
            k = (int(t[j]) << 1) | (1 if s[j] == -1 else 0)
            assert t[j] >= 0 and s[j] in (1, -1) and k in R.pass_keys[j], ("tied winner", j, int(t[j]), int(s[j]))
        else:
            assert (t[j], s[j]) == (R.target[j], R.strand[j]), ("decision", j, int(t[j]), int(s[j]), int(R.target[j]), int(R.strand[j]))


def path_counts(R):
    """The counts that show which kernel paths a case reaches (all from the restatement)."""
    nt = R.n_ties
    return dict(max_cand=int(R.n_cand.max()), max_ties=int(nt.max()), max_walk=int(R.walk.max()), max_items=int(R.items.max()),
                cand_over_regs=int((R.n_cand > SCAN_REGS).sum()), walk_over_slots=int((R.walk > WALK_SLOTS).sum()),
                ties_over_slots=int((nt > TIE_SLOTS).sum()), items_over_stage=int((R.items > SCAN_ITEMS).sum()),
                flag1=int((R.flags == 1).sum()), flag2=int((R.flags == 2).sum()), walks=int((R.cut != INT32_MAX).sum()))


# ---- crafted inputs ------------------------------------------------------------------------------------------------------
def records(fwd, rev, k=K, cells=None):
    """The arrays queries_upload takes for these lists: [all forward][all reverse], positions ascending in steps of 7,
    hpc_len above the last position + k, cells in 1..15."""
    n = len(fwd)
    off_fwd, off_rev = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    np.cumsum([len(x) for x in fwd], out=off_fwd[1:])
    np.cumsum([len(x) for x in rev], out=off_rev[1:])
    off_rev += off_fwd[-1]
    both = list(fwd) + list(rev)
    min_val = np.concatenate([np.asarray(x, np.uint32) for x in both]) if both else np.zeros(0, np.uint32)
    assert min_val.size == 0 or int(min_val.max()) < 4 ** k
    min_pos = np.concatenate([7 * np.arange(len(x), dtype=np.uint32) for x in both]) if both else np.zeros(0, np.uint32)
    longest = np.array([max(len(a), len(b)) for a, b in zip(fwd, rev)], np.uint32)
    hpc_len = 7 * longest + k + 20
    cells = (1 + np.arange(n) % 15).astype(np.uint8) if cells is None else np.asarray(cells, np.uint8)
    return dict(off_fwd=off_fwd, off_rev=off_rev, min_val=min_val, min_pos=min_pos, hpc_len=hpc_len, err_cell=cells)


def left_csr(left_sets):
    """The left MinDB as left_load takes it: keys ascending, per key the ascending clusters that hold it."""
    post = {}
    for t, vs in enumerate(left_sets):
        for v in sorted(set(int(x) for x in vs)):
            post.setdefault(v, []).append(t)
    keys = np.array(sorted(post), np.uint32)
    offs = np.zeros(len(keys) + 1, np.int64)
    np.cumsum([len(post[int(v)]) for v in keys], out=offs[1:])
    postings = np.concatenate([np.asarray(post[int(v)], np.uint32) for v in keys]) if len(keys) else np.zeros(0, np.uint32)
    return keys, offs, postings


def _subset(rng, pool, size):
    return rng.permutation(pool)[:size]


def pool_case(n=1100, seed=5, late=1030):
    """Every list a random subset of a pool of 12 values: forward lists of 9 - 12 of them, reverse lists of 7 - 12, so that any
    two queries share >= 4 values on either strand and every earlier query is a candidate twice.  The first `late` queries, and
    every second one after them, draw from 11 of the values only: the hundreds of targets that hold all 11 tie at their top.  The
    other late queries carry all 12 values in their reverse list: their top Size is reached by candidates among the last targets
    alone — behind the first 2048 entries of the list, whichever way the list is ordered."""
    rng = np.random.default_rng(seed)
    pool = 1000 + 37 * np.arange(12)
    fwd, rev = [], []
    for j in range(n):
        p = pool[:11] if j < late or j % 2 == 0 else pool
        fwd.append(_subset(rng, p, int(rng.integers(9, len(p) + 1))))
        full_rev = j >= late and j % 2 == 1
        rev.append(_subset(rng, p, len(p) if full_rev else int(rng.integers(7, len(p) + 1))))
    return dict(n=n, L=0, fwd=fwd, rev=rev, left_sets=[], need=np.full(n, NEED_NONE, np.uint32))


EDGE_TIES = (1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 300)


def edges_case(L=300):
    """L left clusters that all hold four shared values; query i's six own values are held by the clusters 0 .. EDGE_TIES[i] - 1
    (a posting list of that length), so exactly that many candidates tie at its top Size of 10 and make its walk (cut 8).  The
    last query carries such a list on the reverse strand only, its forward values are nobody's."""
    shared = [50, 60, 70, 80]
    left_sets = [list(shared) for _ in range(L)]
    fwd, rev = [], []
    for i, c in enumerate(EDGE_TIES + (5,)):
        own = [10000 + 100 * i + x for x in range(6)]
        for t in range(c):
            left_sets[t] += own
        mixed = own[:3] + shared[:2] + own[3:] + shared[2:]
        if i < len(EDGE_TIES):
            fwd.append(mixed)
            rev.append(shared[:2 + i % 3])
        else:
            fwd.append([900000 + x for x in range(6)])
            rev.append(mixed)
    n = len(fwd)
    return dict(n=n, L=L, fwd=fwd, rev=rev, left_sets=left_sets, need=np.zeros(n, np.uint32))


def mixed_case(n=400, L=50, seed=11):
    """Three pools of 6, 12 and 40 values; every left cluster and every list draws a random subset of one of them (lists repeat an
    entry now and then: duplicates count once each).  need per query from {0, large}; 5 % of the queries forced over -1, -2 and
    an earlier cluster; half of them with a verdict: a left cluster with a random strand, or -1."""
    rng = np.random.default_rng(seed)
    pools = [2000 + 11 * np.arange(6), 5000 + 13 * np.arange(12), 9000 + 17 * np.arange(40)]

    def draw(lo=1):
        p = pools[int(rng.integers(0, 3))]
        x = _subset(rng, p, int(rng.integers(lo, min(len(p), 16) + 1)))
        if rng.random() < 0.15:
            x = np.insert(x, int(rng.integers(0, len(x) + 1)), x[int(rng.integers(0, len(x)))])
        return x

    left_sets = [np.unique(draw(3)) for _ in range(L)]
    fwd = [draw() for _ in range(n)]
    rev = [draw() for _ in range(n)]
    # left cluster 0 holds the whole pool of 40; three lists of exactly 10, 90 and 170 entries of it: tops at which
    # int(top * 0.7) differs between a double and a 32-bit product (see test_resolve_host.FLOAT_PARTS)
    left_sets[0] = pools[2].copy()
    long_q = {n // 4: 10, n // 2: 90, (3 * n) // 4: 170}
    for j, m in long_q.items():
        fwd[j] = _subset(rng, pools[2], m) if m <= 40 else rng.choice(pools[2], m)
    need = np.where(rng.random(n) < 0.5, NEED_ALL, NEED_NONE).astype(np.uint32)
    forced, openers = {}, []
    for j in np.flatnonzero(rng.random(n) < 0.05).tolist():
        if j in long_q:
            continue
        kind = int(rng.integers(0, 3))
        if kind == 0:
            forced[j] = -1
            openers.append(L + j)
        elif kind == 1:
            forced[j] = -2
        else:
            cl = list(range(L)) + openers
            forced[j] = (int(cl[int(rng.integers(0, len(cl)))]), int(rng.choice([1, -1])))
    vt, vs = np.full(n, NO_VERDICT, np.int32), np.zeros(n, np.int8)
    for j in np.flatnonzero(rng.random(n) < 0.5).tolist():
        if rng.random() < 0.5:
            vt[j] = -1
        else:
            vt[j], vs[j] = int(rng.integers(0, L)), int(rng.choice([1, -1]))
    return dict(n=n, L=L, fwd=fwd, rev=rev, left_sets=left_sets, need=need, forced=forced, verdict_t=vt, verdict_s=vs)


MIXED_PARAMS = ((5, 0.8), (5, 0.7), (5, 1.25), (0, 0.5), (1, 0.0), (12, 1.0))


def restate(case, min_shared=5, min_fraction=0.8, **over):
    c = dict(case, **over)
    return greedy_resolve(c["n"], c["L"], c["fwd"], c["rev"], c["left_sets"], c["need"], min_shared, min_fraction,
                          forced=c.get("forced"), verdict_t=c.get("verdict_t"), verdict_s=c.get("verdict_s"),
                          passes=c.get("passes"), tables=c.get("tables", False))


def lists_of_view(view):
    """Per entry the forward and the reverse value lists of a batch in the layout of ioc_batch_view."""
    mv = np.asarray(view["min_val"])
    n = len(view["off_fwd"]) - 1
    fwd = [mv[view["off_fwd"][j]:view["off_fwd"][j + 1]] for j in range(n)]
    rev = [mv[view["off_rev"][j]:view["off_rev"][j + 1]] for j in range(n)]
    return fwd, rev
