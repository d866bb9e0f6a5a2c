"""ioc_align_pairs_ops: the batched GPU aligner returning the alignment itself.  For every pair of every case the GPU's operation
string equals ioc_host_align_ops' byte for byte; score / windows / ratio equal what ioc_align_pairs returns for the same pairs in
the same context; and the string is checked by itself (tests/align_ops_checks.py: lengths, columns, end gaps, re-scoring), so that
a failure says which side is wrong.  Every route of the aligner: version 2 with and without corridor, one and two traceback
launches, version 1 (forced, fat arena, other letters, refusals of the 16-bit window, a wait that ran out), the re-run of pairs the
corridor's certificate refuses, slices, verdict mode around the call.  No tolerance anywhere: integers and bytes."""
import ctypes as C
import random

import numpy as np
import pytest

from isonclust2_amd import _lib, api
from tests.align_ops_checks import check_ops, revcomp
from tests.test_gpu_align import _mutate

pytestmark = pytest.mark.gpu

GUARD = 64
_host_cache = {}


@pytest.fixture(scope="module")
def ctx():
    return api.Context(0)


def _host_ops(q, r, rc, e):
    """ioc_host_align_ops of one pair (cached: the routes below align the same pairs again and again)."""
    go = _lib.load().ioc_host_gap_open(e)
    key = (q, r, bool(rc), go)
    if key not in _host_cache:
        _host_cache[key] = api.host_align_ops(q, revcomp(r) if rc else r, gap_open=go)
    return _host_cache[key]


def _call(ctx, pairs, k, short=0):
    """The raw C call with guard bytes behind the buffer; returns (rc, score, windows, ratio, [ops], bound)."""
    L = _lib.load()
    n = len(pairs)
    arr = ctx._aln_pairs(pairs)
    bound = L.ioc_align_ops_bound(ctx.h, n, arr)
    assert bound >= 0
    cap = bound - short
    buf = np.full(max(cap, 0) + GUARD, 0xA5, np.uint8)
    off = np.full(n + 1, -7, np.int64)
    score, win, ratio = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.float64)
    rc = L.ioc_align_pairs_ops(ctx.h, n, arr, k, 2, -2, 1, score.ctypes.data_as(C.POINTER(C.c_int32)), win.ctypes.data_as(C.POINTER(C.c_int64)),
                               ratio.ctypes.data_as(C.POINTER(C.c_double)), buf.ctypes.data, cap, off.ctypes.data_as(C.POINTER(C.c_int64)))
    assert np.all(buf[max(cap, 0):] == 0xA5), "bytes written past ops_cap"
    if rc < 0:
        return rc, None, None, None, buf, bound
    assert off[0] == 0 and np.all(np.diff(off) >= 0) and off[n] <= bound
    return rc, score, win, ratio, [buf[off[i]:off[i + 1]].tobytes() for i in range(n)], bound


def _check(ctx, seqs, pairs, k, plain=None, set_pool=True):
    """One emitting call against the host aligner, against a plain ioc_align_pairs (`plain`: its result, taken here if None)
    and against the string's own invariants.  Returns (score, windows, ratio, ops)."""
    if set_pool:
        ctx.align_set_pool(seqs)
    rc, score, win, ratio, ops, _ = _call(ctx, pairs, k)
    assert rc == 0
    if plain is None:
        plain = ctx.align_pairs(pairs, k)
    assert np.array_equal(score, plain[0]) and np.array_equal(win, plain[1]) and np.array_equal(ratio, plain[2])
    L = _lib.load()
    for i, pr in enumerate(pairs):
        qi, ri, rcomp, e = pr[:4]
        q, r = seqs[qi], seqs[ri]
        tag = (i, len(q), len(r), rcomp, e)
        hops, hscore = _host_ops(q, r, rcomp, e)
        if ops[i] != hops:
            d = next((x for x in range(min(len(hops), len(ops[i]))) if hops[x] != ops[i][x]), min(len(hops), len(ops[i])))
            raise AssertionError(f"pair {tag}: device string (len {len(ops[i])}) leaves the host's (len {len(hops)}) at column {d}: "
                                 f"{ops[i][max(0, d - 10):d + 10]!r} / {hops[max(0, d - 10):d + 10]!r}")
        assert score[i] == hscore, tag
        check_ops(ops[i], q, revcomp(r) if rcomp else r, int(score[i]), L.ioc_host_gap_open(e), tag=tag)
        comp = api.ops_to_comp(ops[i])
        assert ratio[i] == L.ioc_host_aln_ratio(comp, len(comp), e, len(q), k) if len(q) else True, tag
    return score, win, ratio, ops


def _small_pairs(seed, count=120):
    rng = random.Random(seed)
    seqs, pairs = [], []
    for t in range(count):
        n, m = rng.randint(0, 200), rng.randint(0, 200)
        base = bytes(rng.choice(b"ACGT") for _ in range(max(n, m) + 20))
        q = _mutate(rng, base, 0.15)[:n]
        r = _mutate(rng, base[rng.randint(0, 12):], 0.15)[:m]
        if t % 9 == 0:
            q = bytes(rng.choice(b"AC") for _ in range(n))
        if t % 11 == 0:
            r = q
        seqs += [q, r]
        pairs.append((2 * t, 2 * t + 1, t % 2, rng.choice([0.0, 0.02, 0.05, 0.12, 0.3, 0.95, 1.3])))
    return seqs, pairs


def test_small_random_pairs(ctx):
    """Lengths 0 .. 200 incl. empty and one base, every gap-open class, limits <= 0 and > k (sizes of test_gpu_align)."""
    seqs, pairs = _small_pairs(13)
    for k in (1, 11, 32):
        _check(ctx, seqs, pairs, k)


def test_multi_strip_pairs(ctx):
    """References wider than one strip: same transcript, a short read inside a long one, suffix / prefix overlap, unrelated."""
    rng = random.Random(5)
    base = bytes(rng.choice(b"ACGT") for _ in range(12000))
    seqs = [
        _mutate(rng, base[:9000], 0.08), _mutate(rng, base[:9100], 0.10),
        _mutate(rng, base[2000:3000], 0.05), _mutate(rng, base, 0.12),
        _mutate(rng, base[6000:], 0.1), _mutate(rng, base[:7000], 0.1),
        bytes(rng.choice(b"ACGT") for _ in range(4100)), _mutate(rng, base[:4097], 0.02),
    ]
    pairs = [(0, 1, 0, 0.18), (1, 0, 0, 0.18), (2, 3, 0, 0.17), (3, 2, 0, 0.17), (4, 5, 0, 0.2), (6, 7, 0, 0.05),
             (0, 1, 1, 0.18), (7, 0, 0, 0.1)]
    _check(ctx, seqs, pairs, 11)


def _edge_pairs():
    rng = random.Random(17)
    base = bytes(rng.choice(b"ACGT") for _ in range(2200))
    lens = [63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2049]
    seqs = [_mutate(rng, base, 0.1)[:ln] for ln in lens] + [base[:1024], base[:1024]]
    pairs = []
    for a in range(len(lens)):
        for b in (a, (a + 5) % len(lens), (a + 8) % len(lens)):
            pairs.append((a, b, (a + b) % 2, rng.choice([0.05, 0.2])))
    pairs.append((len(lens), len(lens) + 1, 0, 0.01))  # identical sequences: one long diagonal
    return seqs, pairs


def test_tile_and_block_edges(ctx):
    """Lengths on and next to every tile and block edge: multiples of 64, 128, 256, 512 and +- 1."""
    seqs, pairs = _edge_pairs()
    _check(ctx, seqs, pairs, 11)


def _unequal_pairs():
    rng = random.Random(37)
    lens = [5000, 700, 2300, 1025, 1023, 513, 512, 4097, 33, 1, 0, 1500, 2600]
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in lens]
    seqs += [_mutate(rng, seqs[0], 0.1), _mutate(rng, seqs[2], 0.08), seqs[3][:500] + b"N" + seqs[3][501:], _mutate(rng, seqs[7], 0.12)]
    n = len(seqs)
    pairs = [(i, (i * 5 + 3) % n, i % 2, rng.choice([0.05, 0.2, 0.3])) for i in range(n)] + [(0, 13, 0, 0.2), (14, 2, 1, 0.2), (7, 16, 0, 0.1)]
    return seqs, pairs


def test_couples_of_unequal_pairs_odd_counts_and_other_letters(ctx):
    """Pairs of very different sizes in one couple, an odd number of pairs, empty and tiny sequences, and pairs with a letter
    other than A C G T — version 1's comparing kernel — in the same call as ordinary ones."""
    seqs, pairs = _unequal_pairs()
    assert len(pairs) % 2 == 0 and any(b"N" in seqs[p[0]] or b"N" in seqs[p[1]] for p in pairs)
    _check(ctx, seqs, pairs + [(13, 0, 1, 0.2)], 11)     # odd
    _check(ctx, seqs, pairs, 7)
    tm = ctx.timings()
    assert tm["align_version"] == 1                       # (the last run of the call: the pairs with the other letter)


def test_full_length_pairs(ctx):
    """16.7 kb reads (config 2): one pair of one transcript, one unrelated pair (a wrong candidate: the walk that wanders), forward
    and reverse-complemented.  The host side costs seconds and 280 MB a pair: four pairs."""
    from isonclust2_amd import synth
    rs = synth.generate_config("config2", seed=1)
    tr = {}
    for i in range(rs.n):
        tr.setdefault(int(rs.transcript[i]), []).append(i)
    same = next(v for v in tr.values() if len(v) >= 2)
    other = next(i for i in range(rs.n) if int(rs.transcript[i]) != int(rs.transcript[same[0]]))
    seqs = [bytes(rs.read(i)[0]) for i in (same[0], same[1], other)]
    assert min(len(s) for s in seqs) > 12000
    pairs = [(0, 1, 0, 0.2), (0, 1, 1, 0.2), (0, 2, 0, 0.12), (2, 0, 1, 0.12)]
    score, win, ratio, ops = _check(ctx, seqs, pairs, 11)
    assert max(ratio[0], ratio[1]) > 0.5 and max(ratio[2], ratio[3]) < 0.2


def _route_pairs():
    rng = random.Random(41)
    base = bytes(rng.choice(b"ACGT") for _ in range(2600))
    seqs = [_mutate(rng, base, 0.1) for _ in range(6)] + [bytes(rng.choice(b"ACGT") for _ in range(1800))]
    seqs += [_mutate(rng, base + base[:2000], 0.08), _mutate(rng, base + base[:1900], 0.08), b"ACGTTGCA" * 9, b""]
    n = len(seqs)
    return seqs, [(i, (i + 1) % n, i % 2, 0.2) for i in range(n)] + [(7, 8, 0, 0.12), (8, 7, 1, 0.12), (0, 6, 0, 0.3)]


@pytest.mark.parametrize("env", [{"IOC_ALIGN_V1": "1"}, {"IOC_ALIGN_ARENA": "fat"}, {"IOC_TRACE2_EARLY": "0"}, {"IOC_TRACE2_DEADLINE": "0"},
                                 {"IOC_ALIGN_VARIANT": "carry"}, {"IOC_ALIGN_CORRIDOR": "0"}, {"IOC_ALIGN_NO_PROFILE": "1"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_every_route(ctx, monkeypatch, env):
    """The switches test_gpu_align.py chooses its routes with.  IOC_ALIGN_VARIANT=carry has no walk: the emitting call takes the
    traced route and still returns strings (the plain call beside it does run the carry kernel: two formulations agree)."""
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    seqs, pairs = _route_pairs()
    _check(ctx, seqs, pairs, 11)
    seqs, pairs = _small_pairs(19, 40)
    _check(ctx, seqs, pairs, 7)
    if "IOC_ALIGN_V1" in env or "IOC_ALIGN_ARENA" in env:
        assert ctx.timings()["align_version"] == 1


def _long_pairs():
    rng = random.Random(61)
    base = bytes(rng.choice(b"ACGT") for _ in range(9000))
    seqs = [_mutate(rng, base, 0.05) for _ in range(10)] + [bytes(rng.choice(b"ACGT") for _ in range(8800)) for _ in range(2)]
    return seqs, [(i, (i + 1) % 10, 0, 0.12) for i in range(10)] + [(0, 10, 0, 0.12), (11, 3, 0, 0.12)]


def test_corridor_against_every_tile(ctx, monkeypatch):
    """Pairs of >= 9 kb (the corridor exists from ~5 kb on), as test_corridor_with_several_slices: every tile, the default corridor,
    and the corridor under a small budget (several slices, each with its own probe launch) return the same strings."""
    seqs, pairs = _long_pairs()
    monkeypatch.setenv("IOC_ALIGN_CORRIDOR", "0")
    ref = _check(ctx, seqs, pairs, 11)
    monkeypatch.delenv("IOC_ALIGN_CORRIDOR")
    got = _check(ctx, seqs, pairs, 11)
    assert got[3] == ref[3]
    monkeypatch.setenv("IOC_ALIGN_CK_BUDGET_MB", "12")
    got = _check(ctx, seqs, pairs, 11)
    assert ctx.timings()["align_slices"] > 1 and got[3] == ref[3]


def test_v2_refusals_come_back_through_version_1(ctx, monkeypatch):
    """Both re-runs of test_v2_fallbacks, with switches that exist already: a guard of 40 makes the 16-bit window refuse (nearly)
    every pair — their bytes are those of version 1's walk —, and a wait that "ran out" sends the whole batch through version 1."""
    seqs, pairs = _route_pairs()
    pairs = [p for p in pairs if len(seqs[p[0]]) and len(seqs[p[1]])]
    ctx.align_set_pool(seqs)
    plain = ctx.align_pairs(pairs, 11)
    monkeypatch.setenv("IOC_ALIGN_V2_GUARD", "40")
    t0 = ctx.timings()["n_align_refused"]
    _check(ctx, seqs, pairs, 11, plain=plain)
    t1 = ctx.timings()["n_align_refused"]
    assert t1 - t0 >= 5, "the guard did not refuse the pairs: the case no longer does what it claims"
    monkeypatch.delenv("IOC_ALIGN_V2_GUARD")
    monkeypatch.setenv("IOC_ALIGN_V2_FAKE_TIMEOUT", "1")
    _check(ctx, seqs, pairs, 11, plain=plain)
    assert ctx.timings()["n_align_refused"] - t1 == len(pairs) and ctx.timings()["align_version"] == 1


def refuted_pairs():
    """Two copies of one 9 kb sequence, each with another block of 1500 bases deleted: equal lengths, so the probe's score per row
    does not contradict the planned width, but between the two blocks the path runs 1500 columns off the diagonal — under a fixed
    corridor of 0.15 x length (the narrowest that exists here: a corridor needs a half width of one strip, 1024 columns) the
    certificate, match x (length - effective half width - 1), lies above the pair's score of 9470."""
    rng = random.Random(71)
    base = bytes(rng.choice(b"ACGT") for _ in range(9000))
    q, r = base[:3000] + base[4500:], base[:6000] + base[7500:]
    other = _mutate(rng, base, 0.03)
    return [q, r, base, other], [(0, 1, 0, 0.05), (2, 3, 0, 0.05), (1, 0, 0, 0.05)]


def test_pair_the_corridor_cannot_vouch_for(ctx, monkeypatch, capfd):
    """A pair that comes back from version 2 with INT32_MIN + 1 and is run again by the every-tile route (scatter_results): its
    bytes are the re-run's.  The re-run is not counted in ioc_timings; its trace is the IOC_TRACE line asserted here.

    Found with runs of the PARENT commit's aligner on refuted_pairs() under IOC_TRACE=1: with blocks of 600 bases and
    IOC_ALIGN_CORRIDOR=0.02 .. 0.1 no corridor came about at all ("0 of 234 tiles skipped"); with blocks of 1500 bases and
    IOC_ALIGN_CORRIDOR=0.15 it printed "corridor: 108 of 201 tiles skipped" and "aligner v2: 2 of 3 pairs run again without a
    corridor" (the two pairs with the deleted blocks; scores 9470, 17022, 9470)."""
    seqs, pairs = refuted_pairs()
    ctx.align_set_pool(seqs)
    plain = ctx.align_pairs(pairs, 11)
    monkeypatch.setenv("IOC_ALIGN_CORRIDOR", "0.15")
    monkeypatch.setenv("IOC_TRACE", "1")
    capfd.readouterr()
    got = _check(ctx, seqs, pairs, 11, plain=plain, set_pool=False)
    err = capfd.readouterr().err
    assert "2 of 3 pairs run again without a corridor" in err, err[-2000:]
    assert list(got[0]) == [9470, 17022, 9470]      # (the parent's scores of that run)


def test_verdict_threshold_is_not_applied_and_survives(ctx):
    """A verdict threshold set beforehand: strings and counts of the emitting call are the exact ones all the same, and a plain
    call after it, still in verdict mode, decides every comparison as before (and does stop walks early)."""
    rng = random.Random(43)
    base = bytes(rng.choice(b"ACGT") for _ in range(5000))
    other = bytes(rng.choice(b"ACGT") for _ in range(4800))
    seqs = [base, _mutate(rng, base, 0.06), _mutate(rng, base, 0.15), _mutate(rng, base, 0.3), other, _mutate(rng, other, 0.1),
            base[:700] + other[700:3000], base[:40], b"ACGT" * 3, b""]
    n = len(seqs)
    pairs = [(i, j, (i + j) % 2, 0.12) for i in range(n) for j in range(n) if i != j and (i + 2 * j) % 3 == 1]
    ctx.align_set_pool(seqs)
    ctx.align_set_verdict_threshold(0.0)
    exact = ctx.align_pairs(pairs, 11)
    stopped = 0
    try:
        for thr in (0.2, 0.6):
            ctx.align_set_verdict_threshold(thr)
            _check(ctx, seqs, pairs, 11, plain=exact, set_pool=False)
            s1, w1, r1 = ctx.align_pairs(pairs, 11)
            assert np.array_equal(exact[0], s1) and np.array_equal(exact[2] >= thr, r1 >= thr) and np.all(w1 <= exact[1])
            stopped += int(np.count_nonzero(w1 < exact[1]))
    finally:
        ctx.align_set_verdict_threshold(0.0)
    assert stopped > 0          # (verdict mode was still on after the emitting calls: walks did stop early)


@pytest.mark.parametrize("arena", ["lean", "fat"])
def test_bound_above_the_budget_runs_in_slices(ctx, monkeypatch, arena):
    """The operation bytes count against the checkpoint arena's budget: a call whose bound (1.15 MB) exceeds a budget of 1 MB runs
    in slices (the switches of test_checkpoint_arena_slices) and returns the strings of the unsliced call."""
    rng = random.Random(23)
    base = bytes(rng.choice(b"ACGT") for _ in range(3000))
    seqs = [_mutate(rng, base, 0.1) for _ in range(12)]
    pairs = [(i, (i + 1) % 12, i % 2, 0.2) for i in range(12)] * 16
    ref = _check(ctx, seqs, pairs, 11)
    monkeypatch.setenv("IOC_ALIGN_CK_BUDGET_MB", "1")
    monkeypatch.setenv("IOC_ALIGN_ARENA", arena)
    ctx.align_set_pool(seqs)
    rc, score, win, ratio, ops, bound = _call(ctx, pairs, 11)
    tm = ctx.timings()
    assert rc == 0 and bound > (1 << 20)
    assert tm["align_version"] == (2 if arena == "lean" else 1) and tm["align_slices"] > 1
    assert ops == ref[3] and np.array_equal(score, ref[0]) and np.array_equal(win, ref[1])


def test_capacity_one_byte_short(ctx):
    """ops_cap one byte below ioc_align_ops_bound: IOC_ERR_CAPACITY and nothing written (the guard bytes of _call, and the buffer)."""
    seqs, pairs = _small_pairs(29, 30)
    ctx.align_set_pool(seqs)
    rc, _, _, _, buf, bound = _call(ctx, pairs, 11, short=1)
    assert rc == -4 and bound == sum(len(seqs[p[0]]) + len(seqs[p[1]]) for p in pairs)
    assert np.all(buf == 0xA5)
    assert _call(ctx, pairs, 11)[0] == 0
    with pytest.raises(api.IocError):
        ctx.align_pairs_ops([(0, len(seqs), 0, 0.1)], 11)          # a pair outside the pool
    assert ctx.align_pairs_ops([], 11)[3] == []
