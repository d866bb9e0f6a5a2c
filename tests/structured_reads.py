"""Test-only read sets with the structure of real transcriptomes, which synth.generate (independent uniform transcripts, at
most exact duplicates) never has: gene families that share a core, isoforms that share exons, truncated reads and tandem
repeats.  Same noise model as synth.generate — substitution, insertion and deletion at e/3 each, e = 10^(-Q/10), Q uniform in
[q_lo, q_hi], random strand, quality Q+33 with +-2 jitter — and the same container (synth.ReadSet); deterministic in the seed.

Transcript builders (each takes the generator first and returns a list of uint8 arrays):
  core_family   one shared random core at a random offset inside unique flanks; optionally transcripts that are the core alone
  isoforms      per gene a list of exons; every isoform keeps each exon with probability ~0.7
  repeat_block  a shared tandem repeat inside unique sequence; the unit has no two equal neighbours, also across the unit
                junction, so homopolymer compression leaves the block as it is

CASES names the fixed cases of tests/test_structured_host.py (preconditions on the CPU) and tests/test_gpu_structured.py."""
import numpy as np

from isonclust2_amd.synth import _ACGT, _COMP, ReadSet


def _rand(rng, n):
    return _ACGT[rng.integers(0, 4, int(n))]


def _length(rng, length):
    """length: a number, or (lo, hi) drawn uniformly per transcript"""
    if isinstance(length, (tuple, list)):
        return int(rng.integers(int(length[0]), int(length[1]) + 1))
    return int(length)


def _inside_flanks(rng, shared, total):
    """`shared` at a random offset of a transcript of `total` bases whose other bases are its own"""
    rest = max(0, total - len(shared))
    a = int(rng.integers(0, rest + 1))
    return np.concatenate([_rand(rng, a), shared, _rand(rng, rest - a)])


def core_family(rng, members, length, core_frac, bare=0):
    """bare: this many further transcripts that are the core alone (a short isoform of nothing but the shared exon): their reads
    share as much with every member as with each other"""
    core = _rand(rng, int(round(_length(rng, length) * core_frac)))
    tr = [_inside_flanks(rng, core, max(_length(rng, length), len(core))) for _ in range(members)]
    return tr + [core.copy() for _ in range(bare)]


def isoforms(rng, genes, exons, per_gene, exon_len=(50, 130), keep=0.7):
    tr = []
    for _ in range(genes):
        ex = [_rand(rng, _length(rng, exon_len)) for _ in range(exons)]
        for _ in range(per_gene):
            on = rng.random(exons) < keep
            if on.sum() < 2:                      # (an isoform of at least two exons)
                on[rng.choice(exons, 2, replace=False)] = True
            tr.append(np.concatenate([e for e, o in zip(ex, on) if o]))
    return tr


def repeat_unit(rng, period):
    """`period` letters, no two neighbours equal, the last differing from the first (period >= 2)"""
    assert period >= 2
    while True:
        u = [int(rng.integers(0, 4))]
        for _ in range(period - 1):
            u.append(int((u[-1] + rng.integers(1, 4)) % 4))
        if u[-1] != u[0]:
            return _ACGT[np.array(u)]


def repeat_block(rng, members, length, period, block_len):
    unit = repeat_unit(rng, period)
    block = np.tile(unit, block_len // period + 1)[:block_len]
    return [_inside_flanks(rng, block, max(_length(rng, length), block_len)) for _ in range(members)]


BUILDERS = {"core_family": core_family, "isoforms": isoforms, "repeat_block": repeat_block}


def _truncate(rng, src, min_frac=0.3):
    """a random prefix, suffix or infix of at least min_frac of the transcript"""
    L = len(src)
    keep = max(1, int(np.ceil(L * (min_frac + (1.0 - min_frac) * rng.random()))))
    kind = int(rng.integers(0, 3))
    a = 0 if kind == 0 else (L - keep if kind == 1 else int(rng.integers(0, L - keep + 1)))
    return src[a:a + keep]


def reads_from(tr, n_reads, rng, q_lo=10.0, q_hi=21.0, first_pass=True, truncate=0.0, tag="structured"):
    """first_pass: read i < len(tr) comes from transcript i (every transcript is read at least once), the others from
    random ones.  truncate: probability that a read covers only a random prefix, suffix or infix (>= 30 %) of its transcript."""
    G = len(tr)
    which = rng.integers(0, G, n_reads).astype(np.int32)
    if first_pass:
        m = min(G, n_reads)
        which[:m] = np.arange(m)
    strand = np.where(rng.random(n_reads) < 0.5, -1, 1).astype(np.int8)
    seqs, quals = [], []
    for i in range(n_reads):
        src = tr[which[i]]
        if truncate > 0 and rng.random() < truncate:
            src = _truncate(rng, src)
        L = len(src)
        Q = q_lo + (q_hi - q_lo) * rng.random()
        e = 10.0 ** (-Q / 10.0)
        u = rng.random(L)
        dele = u < e / 3
        sub = (u >= e / 3) & (u < 2 * e / 3)
        ins = (u >= 2 * e / 3) & (u < e)
        base = src.copy()
        ns = int(sub.sum())
        if ns:
            cur = np.searchsorted(_ACGT, base[sub])
            base[sub] = _ACGT[(cur + rng.integers(1, 4, ns)) % 4]
        cnt = np.ones(L, np.int64)
        cnt[dele] = 0
        cnt[ins] = 2
        out = np.repeat(base, cnt)
        starts = np.cumsum(cnt) - cnt
        ins_pos = starts[ins]
        out[ins_pos] = _ACGT[rng.integers(0, 4, len(ins_pos))]   # the first copy of every inserted pair: a random base
        if strand[i] < 0:
            out = _COMP[out[::-1]]
        q = np.clip(np.rint(Q + 33 + rng.integers(-2, 3, len(out))), 34, 126).astype(np.uint8)
        seqs.append(out)
        quals.append(q)
    offs = np.zeros(n_reads + 1, np.int64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return ReadSet(np.concatenate(seqs), np.concatenate(quals), offs, which, strand, tag)


def generate(builder, args, n_reads, seed, q=(10.0, 21.0), first_pass=True, truncate=0.0):
    rng = np.random.default_rng(seed)
    tr = BUILDERS[builder](rng, **args)
    tag = f"{builder}({','.join(f'{k}={v}' for k, v in args.items())},n={n_reads},Q=[{q[0]:g},{q[1]:g}],seed={seed},trunc={truncate:g})"
    return reads_from(tr, n_reads, rng, q[0], q[1], first_pass=first_pass, truncate=truncate, tag=tag)


# The fixed cases (every set <= 360 reads of <= 900 bases).  The seeds are chosen so that the ORACLE alone meets the
# preconditions that tests/test_structured_host.py asserts on the CPU (which kernel path each case is there for).
CASES = {
    # walks longer than IOC_WALK_SLOTS (32): k_decide_pick scans the whole candidate list
    "family44": dict(builder="core_family", args=dict(members=44, length=700, core_frac=0.55), n_reads=120, seed=1, q=(10.0, 21.0)),
    # more than IOC_SCAN_ITEMS (256) unevaluated candidates of one query: the spill straight to the global queue
    "family340": dict(builder="core_family", args=dict(members=340, length=(400, 500), core_frac=0.55), n_reads=360, seed=1,
                      q=(17.0, 25.0)),
    # long walks that END in a join: reads of the bare core meet 40+ clusters that all hold it, tie at the top Size and pass
    "family_ties": dict(builder="core_family", args=dict(members=44, length=700, core_frac=0.3, bare=16), n_reads=160, seed=2,
                        q=(14.0, 24.0)),
    # shared exons + truncated reads: bounds of totalMapped close to the threshold on both sides
    "isoforms_trunc": dict(builder="isoforms", args=dict(genes=6, exons=6, per_gene=5), n_reads=150, seed=1, q=(10.0, 21.0),
                           truncate=0.4),
    # one read repeats a minimizer value >= 100 times; one posting list hit by every query
    "repeat2": dict(builder="repeat_block", args=dict(members=12, length=800, period=2, block_len=400), n_reads=72, seed=1,
                    q=(12.0, 21.0)),
    # (truncated reads on top: candidates that share only a short stretch of a flank, bounds close to the threshold)
    "repeat3": dict(builder="repeat_block", args=dict(members=12, length=800, period=3, block_len=400), n_reads=150, seed=2,
                    q=(12.0, 21.0), truncate=0.5),
    # a shared core of ~0.22: the alignment fallback's verdicts fall on both sides of aligned_threshold
    "family_aln": dict(builder="core_family", args=dict(members=24, length=500, core_frac=0.22), n_reads=72, seed=1, q=(10.0, 21.0)),
}


def case(name, seed=None):
    c = dict(CASES[name])
    if seed is not None:
        c["seed"] = seed
    rs = generate(c["builder"], c["args"], c["n_reads"], c["seed"], q=c["q"], first_pass=c.get("first_pass", True),
                  truncate=c.get("truncate", 0.0))
    rs.tag = f"{name}:{rs.tag}"
    return rs
