"""The scores the POA engine is tested at besides the reference's 4 / -8 / -8 / -4 / -20 / -1 (ioc_poa_create* accept any m >= 0,
n <= 0, g <= e <= 0, q <= c <= 0 within int8), shared by tests/test_oracle_poa_params.py (the oracle's scalar POA against the
plain statements, on the CPU) and tests/test_gpu_poa_params.py (the engine against the plain recurrence and against the oracle).
Also the one workload both files run under every set: the reads of test_gpu_poa_oracle._random_additions, which do not depend
on the scores, and the count of gap runs in an alignment; and small inputs on which the rule between the two gap pieces decides."""
import random

from tests.poa_common import mutate, random_addition
from tests.poa_modes_common import GLOBAL, LOCAL, SEMI_GLOBAL, first_read_pos, mode_score

# name: ((m, n, g, e, q, c), why it is here)
SCORE_TABLE = {
    "default": ((4, -8, -8, -4, -20, -1), "the control: the reference's scores, the pieces cross at a gap of 5"),
    "linear": ((4, -8, -6, -6, -6, -6), "open / extend tie on every continued gap, vertical and horizontal, both pieces equal"),
    "equal_pieces": ((4, -8, -8, -4, -8, -4), "F1 / F2 and E1 / E2 tie in every cell and come through the same predecessor: the first piece stands, always"),
    "second_never": ((4, -8, -8, -4, -120, -4), "plain affine: the second piece never wins"),
    "free_ext": ((2, -2, -3, 0, -3, 0), "zero extension: the scan offsets vanish, flat prefix maxima, flat row 0"),
    "unit": ((1, -1, -1, -1, -2, -1), "small scores, many equal-score paths"),
    "m0": ((0, -1, -1, -1, -1, -1), "no match reward: local and semi-global alignments are all empty"),
    "int8": ((127, -128, -128, -127, -128, -128), "the reference's type at its corners"),
    "pieces_cross_at_2": ((1, -1, -1, -1, -2, 0), "gap(2) ties between the pieces and every longer gap is the flat second piece: a "
                          "vertical move by the first piece through one predecessor often ties with the second piece through another"),
}
SCORE_NAMES = list(SCORE_TABLE)
TYPES = [LOCAL, GLOBAL, SEMI_GLOBAL]
TYPE_IDS = {LOCAL: "local", GLOBAL: "global", SEMI_GLOBAL: "semi_global"}


def scores(name):
    """the set as the keyword arguments of OraclePoa / Poa / ModePoa and the sc of the plain statements"""
    return dict(zip("mngeqc", SCORE_TABLE[name][0]))


def random_addition_graphs(n_graphs=10):
    """The reads of tests/test_gpu_poa_oracle._random_additions — random.Random(41), the same calls in the same order — for its
    first n_graphs graphs: [(seed read, [(read, weight), ...])].  10 graphs: 71 additions, lengths from 40 / 90 / 200 / 260 /
    330 / 700 (330 and 700 cross the 256-column and 64-row tile edges and the wave carries)."""
    rng = random.Random(41)
    out = []
    for g in range(n_graphs):
        ln = rng.choice([40, 90, 200, 260, 330, 700])
        truth = bytes(rng.choice(b"ACGT") for _ in range(ln))
        first = mutate(rng, truth, rng.choice([0.0, 0.05, 0.15]))
        adds = []
        for t in range(rng.randint(4, 9)):
            r = random_addition(rng, truth, t)
            if not r:
                continue
            adds.append((r, 1 + t % 3))
        out.append((first, adds))
    return out


def gap_runs(nodes, pos):
    """(vertical, horizontal): the alignment's runs of two or more (node, -1) pairs and of two or more (-1, position) pairs"""
    counts = {"vert": 0, "horz": 0}
    kind, length = None, 0
    for v, p in list(zip(nodes.tolist(), pos.tolist())) + [(0, 0)]:
        k = "vert" if p < 0 else ("horz" if v < 0 else None)
        if k != kind:
            if kind and length >= 2:
                counts[kind] += 1
            kind, length = k, 0
        length += 1
    return counts["vert"], counts["horz"]


# what the workload of random_addition_graphs() must hold under every (set, type): runs of two or more, of each kind, over the
# oracle's 71 alignments (measured minimum: 43 vertical / 37 horizontal, `default` under local alignment) ...
MIN_GAP_RUNS = 30


def all_empty(name, t):
    """... except where no alignment exists at all: without a match reward nothing beats the empty local alignment, nor column
    0 of a sink (a semi-global end cell, score 0)"""
    return name == "m0" and t in (LOCAL, SEMI_GLOBAL)


# ---- "the first piece, unless the second piece's predecessor comes earlier in the node's edge list"  ----------------
# The rule needs a cell whose vertical move scores the same through the first piece from one predecessor and through the second
# piece from ANOTHER.  Equal pieces never give that (both pieces then come through the same predecessor), and the random
# workloads above do not either: an engine that always took the first piece passed them all.  These do — graphs of two reads
# and a short third read whose global (one: semi-global) alignment has to skip most of the graph; found by searching small
# inputs for which the choice changes the oracle's pairs, and each checked by piece_predecessor_ties() below.
# ((m, n, g, e, q, c), type, reads)
PIECE_RULE_CASES = [
    ((1, -1, -1, -1, -2, 0), GLOBAL, [b"ACC", b"CGACGC", b"AG"]),         # by hand in tests/test_oracle_poa_params.py
    ((1, -1, -1, -1, -2, 0), GLOBAL, [b"GCCGGACAGAA", b"CAC", b"GG"]),
    ((1, -1, -2, -2, -3, -1), GLOBAL, [b"CAAACCC", b"CAACACC", b"AC"]),
    ((2, -2, -2, -2, -4, -1), GLOBAL, [b"GGGGACAA", b"GCCAGGCGA", b"CCG"]),
    ((3, -2, -3, -2, -5, -1), GLOBAL, [b"ACACCCCACC", b"CCACACC", b"AAAC"]),
    ((4, -8, -8, -4, -20, -1), GLOBAL, [b"AAACCCCAACCC", b"CCACCAACAAC", b"AACA"]),      # (the reference's scores)
    ((1, -1, -1, -1, -2, 0), SEMI_GLOBAL, [b"GCCCCAAGGCAG", b"CAAGCACCCA", b"CACACCCA"]),
]


def piece_predecessor_ties(bases, rank, ef, et, seq, mode, sc, nodes, pos):
    """How many vertical gaps of the alignment (nodes, pos) are entered in a cell where the rule above decides: the cell's
    H is its vertical move, the first piece's best predecessor (first in in-edge order among equals) and the second piece's
    differ, and both give H.  From the plain recurrence's rows alone (poa_modes_common.mode_score)."""
    P = {}
    mode_score(bases, rank, ef, et, seq, mode, sc, planes=P)
    col = first_read_pos(pos) or 0
    pairs = list(zip(nodes.tolist(), pos.tolist()))
    hits = 0
    for x, (v, p) in enumerate(pairs):
        if p >= 0:
            col = p + 1
        last_of_run = v >= 0 and p < 0 and (x + 1 == len(pairs) or not (pairs[x + 1][0] >= 0 and pairs[x + 1][1] < 0))
        if not last_of_run:
            continue
        a1 = [max(int(P["H"][u][col]) + sc["g"], int(P["F1"][u][col]) + sc["e"]) for u in P["preds"][v]]
        a2 = [max(int(P["H"][u][col]) + sc["q"], int(P["F2"][u][col]) + sc["c"]) for u in P["preds"][v]]
        h = int(P["H"][v][col])
        hits += max(a1) == max(a2) == h and a1.index(max(a1)) != a2.index(max(a2))
    return hits
