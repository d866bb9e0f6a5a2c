"""The nine calls of the block family — align_pairs_blocks and the calls that go on from its block search to insertion sites,
alternative ends, windows, variants, full-length isoforms and an isoform consensus — over one small pool: two segments of 257 and
262 bases (a row either side of a 64-row word), eight reads each, a skipped exon planted in the first and an inserted exon in the
second.  What the calls share comes back byte for byte from every one of them, each call's whole result is the one recorded when the
nine had a body each (PINNED), the empty call returns zeroed offsets from all nine, and every capacity one below its bound is
refused by the entry point that was called, under its own name."""
import hashlib
import random

import numpy as np
import pytest

from isonclust2_amd import api
from tests import polish_common as pc
from tests import structured_reads as sr

pytestmark = pytest.mark.gpu

K = 11
CALLS = {  # the Python entry point -> the C entry point its refusals name
    "align_pairs_blocks": "ioc_align_pairs_blocks",
    "align_pairs_blocks_inserts": "ioc_align_pairs_blocks_inserts",
    "align_pairs_blocks_ends": "ioc_align_pairs_blocks_ends",
    "align_pairs_blocks_inserts_seq": "ioc_align_pairs_blocks_inserts_seq",
    "align_pairs_blocks_inserts_variants": "ioc_align_pairs_blocks_inserts_variants",
    "align_pairs_isoforms_full": "ioc_align_pairs_isoforms_full",
    "align_pairs_isoforms_full_variants": "ioc_align_pairs_isoforms_full_variants",
    "align_pairs_blocks_polish": "ioc_align_pairs_blocks_polish",
    "align_pairs_blocks_polish_weighted": "ioc_align_pairs_blocks_polish_weighted",
}
SHARED = ("score", "windows", "blocks", "block_off", "reads", "seg", "cols")
WITH_INSERTS = [m for m in CALLS if "inserts" in m or "full" in m]
WITH_WINDOWS = [m for m in WITH_INSERTS if m != "align_pairs_blocks_inserts"]
WITH_VARIANTS = [m for m in CALLS if "variants" in m]
# sha256 of every call's whole result (tables and statistics included), recorded from the library in which every entry point had
# a body of its own
PINNED = {
    "align_pairs_blocks": "64a866d5dc825e0b8530a47e44e7fac67dab3c8cc9968762e657048beffa78c0",
    "align_pairs_blocks_inserts": "74387612488850fa37c2300996c52f5780f03f80f066a8693a1546d15b736d42",
    "align_pairs_blocks_ends": "4e41f1dfd53abe6d00b5a60788991f28ce2aeb27065cf95f159cd32ef1d982af",
    "align_pairs_blocks_inserts_seq": "858e150694bc2c7929e8093ac33314b4fd5238093afe326cfafaeb88afe1dd1b",
    "align_pairs_blocks_inserts_variants": "1cffd5fdeb28af7f5ba5814f27c2657a73c006a9eb6bddfa3c8cab7dba9b6db9",
    "align_pairs_isoforms_full": "8127921c73c931570696247b462ca507d16d4635a7e1a7741b80817d89879352",
    "align_pairs_isoforms_full_variants": "214fa7bd9821656a7f3ba6101488b75f0e80f43ca99d4eb21e176169c21c17ac",
    "align_pairs_blocks_polish": "706bd31de5aa3d4611774c6c224e0709986c59a863e6c24b1cf09b11114a6208",
    "align_pairs_blocks_polish_weighted": "8384cdadbc8ad0c414f3b08e5f26e613a65c94fcfeaa66f8b1988a5ad921129f",
}


def _pool():
    """(sequences, qualities, pairs, seg_of_pair, segs): segment 0 is a 257-base frame that four of its reads follow and four
    follow without its rows 100 .. 149; segment 1 a 262-base frame that four reads follow and four carry 40 bases more in, behind
    row 130.  The segments' pairs are dealt out in turn; the reads differ from what they follow at 2 % of the bases."""
    gen, rng = np.random.default_rng(257262), random.Random(257262)
    f0, f1, exon = (sr._rand(gen, n).tobytes() for n in (257, 262, 40))
    src = [[f0] * 4 + [f0[:100] + f0[150:]] * 4, [f1] * 4 + [f1[:130] + exon + f1[130:]] * 4]
    reads = [[pc.mutate(rng, s, 0.02) for s in seg] for seg in src]
    seqs, pairs = [f0, f1], []
    for j in range(8):
        for g in range(2):
            pairs.append((len(seqs), g, 0, 0.1))
            seqs.append(reads[g][j])
    quals = [bytes(rng.randrange(40, 70) for _ in s) for s in seqs]
    return seqs, quals, pairs, [p[1] for p in pairs], [(0, 0), (1, 0)]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    seqs, quals = _pool()[:2]
    c.align_set_pool(seqs)
    c.align_set_pool_qual(quals)
    return c


@pytest.fixture(scope="module")
def results(ctx):
    """every call's result over the pool, computed once"""
    _, _, pairs, sop, segs = _pool()
    return {m: getattr(ctx, m)(pairs, K, segs, sop, tables=True, stats=True) for m in CALLS}


def _flat(x, path, out):
    if isinstance(x, dict):
        for f in sorted(x):
            _flat(x[f], f"{path}/{f}", out)
    elif isinstance(x, (list, tuple)):
        out.append(f"{path}#{len(x)}".encode())
        for i, u in enumerate(x):
            _flat(u, f"{path}[{i}]", out)
    elif isinstance(x, np.ndarray):
        out.append(f"{path}:{x.dtype.str}:{x.shape}".encode() + np.ascontiguousarray(x).tobytes())
    else:
        out.append(f"{path}=".encode() + (x if isinstance(x, bytes) else repr(x).encode()))


def _bytes(x):
    out = []
    _flat(x, "", out)
    return b"\0".join(out)


@pytest.mark.parametrize("method", list(CALLS))
def test_what_the_calls_share_is_align_pairs_blocks(results, method):
    plain, got = results["align_pairs_blocks"], results[method]
    assert int(plain["block_off"][-1]) >= 1 and plain["seg"]["n_groups"].tolist()[0] >= 2   # (the skipped exon is found: there is something to share)
    for f in SHARED:
        assert _bytes(got[f]) == _bytes(plain[f]), f
    if method in WITH_INSERTS:
        first = results[WITH_INSERTS[0]]["inserts"]
        assert int(first["site_off"][-1]) >= 1 and _bytes(got["inserts"]) == _bytes(first)   # (the inserted exon is found)
    if method in WITH_WINDOWS:
        first = results[WITH_WINDOWS[0]]["insert_windows"]
        assert len(first["seq"][0]) > 0 and _bytes(got["insert_windows"]) == _bytes(first)
    if method in WITH_VARIANTS:
        assert _bytes(got["insert_variants"]) == _bytes(results[WITH_VARIANTS[0]]["insert_variants"])
    assert sorted(k for k in got if k in ("inserts", "insert_windows", "insert_variants", "isoforms_full", "ends", "extents", "gseq")) == sorted(
        (["inserts"] if method in WITH_INSERTS else []) + (["insert_windows"] if method in WITH_WINDOWS else []) +
        (["insert_variants"] if method in WITH_VARIANTS else []) + (["isoforms_full"] if "full" in method else []) +
        (["ends", "extents"] if "ends" in method else []) + (["gseq"] if "polish" in method else []))


@pytest.mark.parametrize("method", list(CALLS))
def test_every_call_returns_what_it_always_did(results, method):
    digest = hashlib.sha256(_bytes(results[method])).hexdigest()
    print(f'    "{method}": "{digest}",')
    assert digest == PINNED.get(method)


def _offsets(x, path=""):
    """every array of offsets of a result, by its path"""
    if isinstance(x, dict):
        for f, v in x.items():
            if isinstance(v, dict):
                yield from _offsets(v, f"{path}/{f}")
            elif f.endswith("off"):
                yield f"{path}/{f}", v


@pytest.mark.parametrize("method", list(CALLS))
def test_the_empty_call_returns_zeroed_offsets(ctx, method):
    got = getattr(ctx, method)([], K, [], [], tables=True, stats=True)
    offs = dict(_offsets(got))
    assert "/block_off" in offs and ("inserts" in method) <= ("/inserts/site_off" in offs) and ("full" in method) <= ("/isoforms_full/splice_off" in offs)
    for path, v in offs.items():
        assert len(v) >= 1 and not np.any(v), path
    assert len(got["score"]) == 0 and len(got["reads"]) == 0 and got["blocks"] == []


def _capacities(method):
    """{keyword: bound} of the capacities a method takes, over the pool at the default rules"""
    rlen, n_reads = [257, 262], [8, 8]
    caps = dict(cap=sum(api.planes_blocks_bound(m, api.BLOCKS_RULE["max_blocks"]) for m in rlen))
    sites = sum(api.planes_inserts_bound(m, api.INSERTS_RULE["max_sites"]) for m in rlen)
    if method in WITH_INSERTS:
        caps.update(sites_cap=sites)
    if method in WITH_WINDOWS:
        caps.update(win_cap=api.insert_windows_bound(sites))
    if method in WITH_VARIANTS:
        caps.update(var_cap=api.insert_window_variants_bound(sites))
    if "full" in method:
        caps.update(zip(("full_cap", "iso_cap", "splice_cap"), api.isoforms_full_bound(rlen, n_reads, 16)))
    if "ends" in method:
        ends = [api.reads_ends_bound(m, k) for m, k in zip(rlen, n_reads)]
        caps.update(sites_cap=sum(e[0] for e in ends), variants_cap=sum(e[1] for e in ends))
    if "polish" in method:
        most = [api.blocks_polish_bound(m, k, 16) for m, k in zip(rlen, n_reads)]
        caps.update(iso_cap=sum(b[0] for b in most), polish_cap=sum(b[1] for b in most))
    return caps


@pytest.mark.parametrize("method", list(CALLS))
def test_a_capacity_below_its_bound_is_refused_under_the_entry_points_name(ctx, results, method):
    _, _, pairs, sop, segs = _pool()
    caps = _capacities(method)
    assert all(b >= 1 for b in caps.values()), caps
    for kw, bound in caps.items():
        with pytest.raises(api.IocError) as e:
            getattr(ctx, method)(pairs, K, segs, sop, **{kw: bound - 1})
        assert e.value.code == -4 and str(e.value).split(": ", 1)[1].startswith(CALLS[method] + ": "), (kw, str(e.value))
    # exactly the bounds: everything fits, and the result is the one computed with the default room
    got = getattr(ctx, method)(pairs, K, segs, sop, tables=True, stats=True, **caps)
    assert hashlib.sha256(_bytes(got)).hexdigest() == hashlib.sha256(_bytes(results[method])).hexdigest()
