#!/usr/bin/env python3
"""A handful of alignments from the GPU, shown: score, ratio, CIGAR and the three-row picture.

    tools/align_dump.py QUERY.fa REF.fa [--revcomp] [-e E] [-k K] [--width 100] [--max-pairs 8] [--full]

Record i of QUERY.fa is aligned against record i of REF.fa (FASTA or FASTQ; a single record in REF.fa is taken for every
query) through ioc_align_pairs_ops.  Long alignments are shown around their first columns that are no match unless --full."""
import argparse
import sys

sys.path.insert(0, ".")
from isonclust2_amd import api  # noqa: E402

_COMP = {65: 84, 67: 71, 71: 67, 84: 65}


def records(path):
    """(name, sequence) of every record of a FASTA file, or of a FASTQ file with four lines per record."""
    with open(path, "rb") as f:
        lines = [ln.strip() for ln in f if ln.strip()]
    if lines and lines[0].startswith(b"@"):
        return [(lines[i][1:].split()[0].decode(), lines[i + 1].upper()) for i in range(0, len(lines) - 1, 4)]
    out = []
    for ln in lines:
        if ln.startswith(b">"):
            out.append([(ln[1:].split() or [b""])[0].decode(), b""])
        elif out:
            out[-1][1] += ln.upper()
    return [(n, s) for n, s in out]


def picture(ops, q, r):
    """The gapped query row, the comparison row, the gapped reference row."""
    top, mid, bot = bytearray(), bytearray(), bytearray()
    i = j = 0
    for op in ops:
        a = b = 0x2D
        if op in b"=XIi":
            a, i = q[i], i + 1
        if op in b"=XDd":
            b, j = r[j], j + 1
        top.append(a)
        bot.append(b)
        mid.append(0x7C if op == 0x3D else (0x2E if op == 0x58 else 0x20))
    return bytes(top), bytes(mid), bytes(bot)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("query")
    ap.add_argument("ref")
    ap.add_argument("--revcomp", action="store_true", help="align against the reverse complement of the reference")
    ap.add_argument("-e", type=float, default=0.12, help="summed error rate of the two sequences (gap open, window limit)")
    ap.add_argument("-k", type=int, default=11)
    ap.add_argument("--width", type=int, default=100)
    ap.add_argument("--max-pairs", type=int, default=8)
    ap.add_argument("--full", action="store_true", help="the whole picture, however long")
    a = ap.parse_args()
    qs, rs = records(a.query), records(a.ref)
    if len(rs) == 1:
        rs = rs * len(qs)
    n = min(len(qs), len(rs), a.max_pairs)
    seqs = [s for _, s in qs[:n]] + [s for _, s in rs[:n]]
    ctx = api.Context(0)
    ctx.align_set_pool(seqs)
    score, win, ratio, ops = ctx.align_pairs_ops([(i, n + i, int(a.revcomp), a.e) for i in range(n)], a.k)
    for i in range(n):
        q, r = seqs[i], seqs[n + i]
        if a.revcomp:
            r = bytes(_COMP.get(ch, ch) for ch in reversed(r))
        cigar = api.ops_to_cigar(ops[i])
        print(f"{qs[i][0]} ({len(q)}) x {rs[i][0]} ({len(r)}){' revcomp' if a.revcomp else ''}: score {score[i]}, windows {win[i]}, ratio {ratio[i]:.6f}, "
              f"{len(ops[i])} columns")
        print("  CIGAR", cigar if a.full or len(cigar) <= 400 else cigar[:400] + " ...")
        top, mid, bot = picture(ops[i], q, r)
        spans = [(0, len(mid))]
        if not a.full and len(mid) > 6 * a.width:
            first = next((x for x, op in enumerate(ops[i]) if op in b"=X"), 0)
            spans = [(max(0, first - a.width), min(len(mid), first + 2 * a.width)), (max(0, len(mid) - 2 * a.width), len(mid))]
        for lo, hi in spans:
            for x in range(lo, hi, a.width):
                print(f"  {x:>8} {top[x:x + a.width].decode(errors='replace')}\n  {'':>8} {mid[x:x + a.width].decode()}\n  {'':>8} {bot[x:x + a.width].decode(errors='replace')}\n")
            if (lo, hi) != spans[-1]:
                print("           ...\n")
    ctx.close()


if __name__ == "__main__":
    main()
