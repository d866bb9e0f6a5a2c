"""`dump --isoforms --isoforms-polish --isoforms-polish-weighted`: cluster_isoforms.fq called by weight
(ioc_align_pairs_blocks_polish_weighted on the GPU).  The option is parsed and refused without a GPU.  The read set is that of
test_cli_isoforms_polish.py with base qualities that differ within a read; cluster_isoforms.fq is recomputed through
Context.align_pairs_blocks_polish_weighted from the files `dump` wrote alone, under the quality lines of cluster_cons.fq and
cluster_fastq/.  Every other report file does not change by one byte when the option stands beside it, and without it
cluster_isoforms.fq is the unweighted call's."""
import os
import random

import numpy as np
import pytest

from isonclust2_amd import api, synth
from tests import blocks_common as bc
from tests.test_cli import run
from tests.test_cli_read_stats import K, _fastq_records, _files

POLISH = ["--isoforms", "--isoforms-polish"]
NAMES = {"polish": POLISH, "weighted": POLISH + ["--isoforms-polish-weighted"],
         "polish_all": POLISH + ["--read-stats", "--pileup", "--polish", "--polish-weighted"],
         "weighted_all": POLISH + ["--isoforms-polish-weighted", "--read-stats", "--pileup", "--polish", "--polish-weighted"]}


def test_the_option_is_parsed_and_in_the_help(tmp_path):
    base = ("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"))
    r = run(*base, "--isoforms", "--isoforms-polish-weighted", "nothing.cer")
    assert r.returncode == 1 and "--isoforms-polish-weighted asks for --isoforms-polish" in r.stderr
    r = run(*base, "--isoforms-polish-weighted", "nothing.cer")
    assert r.returncode == 1 and "asks for" in r.stderr
    s = run(*base, "--polish-weighted", "nothing.cer")
    assert s.returncode == 1 and "--polish-weighted asks for --polish" in s.stderr            # (it dies as that one does)
    r = run(*base, "--isoforms", "--isoforms-polish", "--isoforms-polish-weighted", "nothing.cer")
    assert r.returncode == 1 and "asks for" not in r.stderr                                   # (as far as the batch)
    h = run("dump", "--help")
    words = " ".join(h.stderr.split())
    assert h.returncode == 0 and "[--isoforms-polish-weighted]" in h.stderr
    assert "--isoforms-polish-weighted with --isoforms-polish: call every isoform by weight" in words and "still no read is aligned again" in words


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("isoforms_polish_weighted")
    fq = tmp / "reads.fq"
    _, reads, _ = bc.property_case(bc.SEED, rate=0.01)
    rng = random.Random(3)
    with open(fq, "wb") as f:
        rs = synth.generate(30, 3, 400, 12, 21, seed=5)
        for i in range(rs.n):
            s, q = rs.read(i)
            f.write(b"@r%d extra words\n" % i + s + b"\n+\n" + q + b"\n")
        for i, s in enumerate(reads):   # base qualities of 17 .. 31 around the 20 .. 28 of test_cli_isoforms_polish.py
            f.write(b"@t%d\n" % i + s + b"\n+\n" + bytes(33 + rng.randrange(17, 32) for _ in s) + b"\n")
    out = tmp / "sorted"
    r = run("sort", "-o", str(out), str(fq))
    assert r.returncode == 0, r.stderr
    r = run("cluster", "-l", str(out / "batches" / "isONbatch_0.cer"), "-o", str(tmp / "c.cer"), "-x", "fast", env=dict(os.environ, ISONCLUST2_SERVE="0"))
    assert r.returncode == 0, r.stderr
    for name, extra in NAMES.items():
        r = run("dump", "-i", str(out / "sorted_reads_idx.cer"), "-o", str(tmp / name), *extra, str(tmp / "c.cer"))
        assert r.returncode == 0, r.stderr
    return {name: tmp / name for name in NAMES}


@pytest.mark.gpu
def test_the_other_reports_do_not_change(dumps):
    files = {name: _files(d) for name, d in dumps.items()}
    for with_, without in (("weighted", "polish"), ("weighted_all", "polish_all")):
        assert set(files[with_]) == set(files[without]), with_
        for f in files[without]:
            assert (files[with_][f] == files[without][f]) == (f != "cluster_isoforms.fq"), (with_, f)
    assert files["weighted_all"]["cluster_isoforms.fq"] == files["weighted"]["cluster_isoforms.fq"]
    assert files["polish_all"]["cluster_isoforms.fq"] == files["polish"]["cluster_isoforms.fq"]


def _library_records(d, weighted):
    """cluster_isoforms.fq from the files `dump` wrote alone, through the library: the lines of the file"""
    cons = {int(head.split(b" ")[0][8:]): (seq, qual) for head, seq, qual in _fastq_records(d / "cluster_cons.fq")}
    reads = {cid: (_fastq_records(d / "cluster_fastq" / f"{cid}.fq") if os.path.exists(d / "cluster_fastq" / f"{cid}.fq") else []) for cid in cons}
    lines = [q for _, q in cons.values()] + [q for cid in cons for _, _, q in reads[cid]]
    offs = np.zeros(len(lines) + 1, np.int64)
    offs[1:] = np.cumsum([len(q) for q in lines])
    ctx = api.Context(0)
    _, err = ctx.qual_scores(offs, np.frombuffer(b"".join(lines), np.uint8), K)
    err = [float(e) for e in err]
    cons_err, read_err = dict(zip(cons, err)), iter(err[len(cons):])
    seqs, quals, pairs, sop, segs, seg_cls = [], [], [], [], [], []
    for cid, (ref, ref_q) in cons.items():
        if not reads[cid]:
            continue
        seqs.append(ref), quals.append(ref_q)
        segs.append((len(seqs) - 1, 0))
        seg_cls.append(cid)
        for head, s, q in reads[cid]:
            seqs.append(s), quals.append(q)
            pairs.append((len(seqs) - 1, segs[-1][0], 0, next(read_err) + cons_err[cid]))
            sop.append(len(segs) - 1)
    ctx.align_set_pool(seqs)
    ctx.align_set_pool_qual(quals)
    assert len(pairs) >= 60
    call = ctx.align_pairs_blocks_polish_weighted if weighted else ctx.align_pairs_blocks_polish
    got = call(pairs, K, segs, sop, rows=False, polish_min_depth=3, max_iso=16)
    want, planted = [], 0
    for g, cid in sorted(enumerate(seg_cls), key=lambda t: t[1]):   # (cluster order)
        z, mine = got["seg"][g], got["reads"][[x for x, s in enumerate(sop) if s == g]]
        if int(z["n_blocks"]) < 1:
            continue
        for h, (seq, qual, st) in enumerate(zip(got["gseq"][g], got["gqual"][g], got["gpolish"][g])):
            direct = mine[(mine["group"] == h) & (mine["how"] == api.ISO_DIRECT)]
            n = len(direct) + int(((mine["group"] == h) & (mine["how"] == api.ISO_ASSIGNED)).sum())
            head = (f"@cluster_{cid}/iso{h} key={bc.signature(direct['key'][0], int(z['n_blocks']))} reads={n} subs={int(st['n_sub'])} dels={int(st['n_del'])} "
                    f"ins={int(st['n_ins'])} low={int(st['n_low'])}")
            want += [head.encode(), seq, b"+", qual]
        planted += int(z["n_blocks"]) == 2 and int(z["n_groups"]) == 4
    ctx.close()
    return want + [b""], planted


@pytest.mark.gpu
def test_the_file_holds_the_weighted_calls_of_the_library(dumps):
    want, planted = _library_records(dumps["weighted"], True)
    assert open(dumps["weighted"] / "cluster_isoforms.fq", "rb").read().split(b"\n") == want
    assert planted >= 1 and len(want) >= 4 * 4
    plain, _ = _library_records(dumps["polish"], False)
    assert open(dumps["polish"] / "cluster_isoforms.fq", "rb").read().split(b"\n") == plain      # without the option: the unweighted call
    names = lambda lines: [x.split(b" ")[0] for x in lines[0:-1:4]]
    assert plain != want and names(plain) == names(want)   # the same names, in order
