"""Plain-Python statements of the three alignment types of the POA engine (`cluster -A`: 0 local, 1 global, 2 semi-global;
DESIGN.md 5.7): the sequence-to-graph recurrence over an exported graph, a path scorer that knows the types' boundaries, and
a brute force over the source-to-sink paths of a small graph.  oracle/poa_oracle.cpp states the three types too, tie rules
included; what is here is what pins IT (tests/test_oracle_poa_modes.py: scores, rescored paths, boundaries, the brute force),
before the engine is compared with it pair by pair (tests/test_gpu_poa_oracle.py).  This file knows scores, not tie rules."""
import numpy as np

from tests.poa_common import NEG, SC, _path_score

LOCAL, GLOBAL, SEMI_GLOBAL = 0, 1, 2


def gap(k, sc=SC):
    """convex gap of k bases: the better of the two affine pieces (g, e) and (q, c)"""
    return 0 if k <= 0 else max(sc["g"] + (k - 1) * sc["e"], sc["q"] + (k - 1) * sc["c"])


def _graph(n, ef, et):
    preds = [[] for _ in range(n)]
    sink = [True] * n
    for a, b in zip(ef, et):
        preds[int(b)].append(int(a))
        sink[int(a)] = False
    return preds, sink


def mode_score(bases, rank, ef, et, seq, mode, sc=SC, planes=None):
    """Best end cell of the sequence-to-graph DP.  Rows: row 0 the virtual source, then the nodes in the order `rank`;
    columns 0..L.  Per row, numpy over the columns: vertical moves F1 / F2 and the diagonal from the predecessors, then the
    horizontal gaps as prefix maxima of H-without-them (opening right after a gap never beats extending it: g <= e, q <= c).
    planes: a dict that receives the rows themselves, {"H" | "F1" | "F2": {node (-1: row 0): row}} and "preds": the
    predecessor lists in in-edge order ([-1] for a node without in-edges)."""
    n, L = len(bases), len(seq)
    preds, sink = _graph(n, ef, et)
    read = np.frombuffer(bytes(seq), np.uint8).astype(np.int64)
    cols = np.arange(L + 1, dtype=np.int64)
    row0 = np.zeros(L + 1, np.int64) if mode == LOCAL else np.array([gap(j, sc) for j in range(L + 1)], np.int64)
    neg = np.full(L + 1, NEG, np.int64)
    H, F1, F2 = {-1: row0}, {-1: neg}, {-1: neg}
    best = 0 if mode == LOCAL else None
    for v in [int(x) for x in rank]:
        ps = preds[v] or [-1]
        f1 = np.max([np.maximum(H[p] + sc["g"], F1[p] + sc["e"]) for p in ps], axis=0)
        f2 = np.max([np.maximum(H[p] + sc["q"], F2[p] + sc["c"]) for p in ps], axis=0)
        diag = np.full(L + 1, NEG, np.int64)
        s = np.where(read == bases[v], sc["m"], sc["n"])
        diag[1:] = np.max([H[p][:-1] for p in ps], axis=0) + s
        hn = np.maximum(diag, np.maximum(f1, f2))
        if mode == LOCAL:
            hn = np.maximum(hn, 0)
        if mode in (LOCAL, SEMI_GLOBAL):
            hn[0] = 0                       # (global: column 0 is the best vertical move from row 0)
        h = hn.copy()
        for g, e in ((sc["g"], sc["e"]), (sc["q"], sc["c"])):
            pm = np.maximum.accumulate(hn - e * cols)       # max over x <= j of Hn[x] - e x
            h[1:] = np.maximum(h[1:], pm[:-1] + g + (cols[1:] - 1) * e)
        H[v], F1[v], F2[v] = h, f1, f2
        if planes is not None:
            planes.update(H=H, F1=F1, F2=F2)
            planes.setdefault("preds", {})[v] = ps
        if mode == LOCAL:
            cand = int(h.max())                                  # every cell
        elif mode == GLOBAL:
            if not sink[v]:
                continue
            cand = int(h[L])                                     # column L of a sink
        else:
            cand = int(h.max()) if sink[v] else int(h[L])        # any column of a sink, column L of any node
        best = cand if best is None else max(best, cand)
    return best


def first_read_pos(pos):
    ps = [int(p) for p in pos if p >= 0]
    return ps[0] if ps else None


def mode_path_score(bases, ef, et, seq, nodes, pos, mode, sc=SC):
    """Score of an alignment path (poa_common._path_score checks that it is a walk) plus what its type's boundary charges: a
    semi-global walk that stopped on row 0 left the read's head unaligned at gap(first read position) (on column 0 that is 0).
    Global paths carry their row-0 insertions as pairs of their own."""
    total = _path_score(bases, ef, et, seq, nodes, pos, sc)
    if mode == SEMI_GLOBAL:
        p0 = first_read_pos(pos)
        total += gap(p0, sc) if p0 is not None else 0
    return total


def boundary_violations(ef, et, n_nodes, L, nodes, pos, mode):
    """What a path of the type must look like.  Global: every read position in order, first node a source, last node a sink.
    Semi-global: it starts on row 0 (first pair on a source node) or column 0 (first read position 0) and ends in column L
    (last read position L - 1) or on a sink (last node)."""
    preds, sink = _graph(n_nodes, ef, et)
    nd = [int(v) for v in nodes if v >= 0]
    ps = [int(p) for p in pos if p >= 0]
    bad = []
    if mode == GLOBAL:
        if ps != list(range(L)):
            bad.append("read positions are not 0..L-1")
        if not nd or preds[nd[0]]:
            bad.append("first node is not a source")
        if not nd or not sink[nd[-1]]:
            bad.append("last node is not a sink")
    elif mode == SEMI_GLOBAL and len(nodes):
        first_node = int(nodes[0])
        if not (ps and ps[0] == 0) and not (first_node >= 0 and not preds[first_node]):
            bad.append("does not start on row 0 or column 0")
        if not (ps and ps[-1] == L - 1) and not (nd and sink[nd[-1]]):
            bad.append("does not end in column L or on a sink")
    return bad


def seq_score(a, b, mode, sc=SC):
    """Plain sequence-to-sequence DP of a path's letters a against the read b, every gap run charged gap(k) directly
    (O(n^3), no affine pieces): H[i][j] = max(diagonal, H[i - k][j] + gap(k), H[i][j - k] + gap(k))."""
    n, L = len(a), len(b)
    H = [[NEG] * (L + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        for j in range(L + 1):
            if i == 0:
                H[0][j] = gap(j, sc)                                 # the read's prefix costs
                continue
            if j == 0:
                H[i][0] = gap(i, sc) if mode == GLOBAL else 0       # global: the path's prefix costs; semi-global: free
                continue
            v = H[i - 1][j - 1] + (sc["m"] if a[i - 1] == b[j - 1] else sc["n"])
            v = max([v] + [H[i - k][j] + gap(k, sc) for k in range(1, i + 1)] + [H[i][j - k] + gap(k, sc) for k in range(1, j + 1)])
            H[i][j] = v
    if mode == GLOBAL:
        return H[n][L]
    return max(max(H[i][L] for i in range(1, n + 1)), max(H[n]))   # column L of any row, any column of the last row


def brute_force(bases, ef, et, seq, mode, sc=SC):
    """Best over every source-to-sink path of the graph of seq_score (global or semi-global)."""
    n = len(bases)
    preds, sink = _graph(n, ef, et)
    succ = [[] for _ in range(n)]
    for a, b in zip(ef, et):
        succ[int(a)].append(int(b))
    best = None

    def walk(v, path):
        nonlocal best
        path = path + [v]
        if sink[v]:
            s = seq_score(bytes(bases[x] for x in path), seq, mode, sc)
            best = s if best is None else max(best, s)
        for w in succ[v]:
            walk(w, path)

    for v in range(n):
        if not preds[v]:
            walk(v, [])
    return best
