"""`dump --isoforms --isoforms-ends`: cluster_ends.tsv, cluster_end_variants.tsv and read_ends.tsv (ioc_align_pairs_blocks_ends on the
GPU).  The options are parsed and refused without a GPU.  The read set is that of test_cli_isoforms_inserts.py with eight reads that
stop at base 600 of the transcript and eight that start at base 300 beside it.  The three files are recomputed through
Context.align_pairs_blocks_ends from the files `dump` wrote alone.  The three files of --isoforms, and every other report file, do
not change by one byte when the option stands beside them."""
import os
import random

import numpy as np
import pytest

from isonclust2_amd import api, synth
from tests import blocks_common as bc
from tests import polish_common as pc
from tests.test_cli import run
from tests.test_cli_read_stats import K, _fastq_records, _files

NAMES = {"isoforms": ["--isoforms"], "ends": ["--isoforms", "--isoforms-ends"],
         "isoforms_stats": ["--isoforms", "--read-stats", "--pileup"], "ends_stats": ["--isoforms", "--isoforms-ends", "--read-stats", "--pileup"],
         "ends_rule": ["--isoforms", "--isoforms-ends", "--isoforms-ends-slack", "3", "--isoforms-ends-min-over", "5", "--isoforms-ends-min-pct", "30",
                       "--isoforms-ends-max", "1", "--isoforms-ends-max-variants", "1"]}
RULES = {"ends": {}, "ends_rule": dict(slack=3, min_over=5, ends_min_pct=30, max_sites=1, max_variants=1)}
NEW = {"cluster_ends.tsv", "cluster_end_variants.tsv", "read_ends.tsv"}
REPRESENTATIVE = bc.SIZES[0]   # the first read of the isoform without [150, 190), as in test_cli_isoforms_inserts.py


def test_the_options_are_parsed_and_in_the_help(tmp_path):
    base = ("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--isoforms", "--isoforms-ends")
    for flag, bad in (("--isoforms-ends-slack", "-1"), ("--isoforms-ends-slack", "33"), ("--isoforms-ends-min-over", "0"), ("--isoforms-ends-min-pct", "0"),
                      ("--isoforms-ends-min-pct", "101"), ("--isoforms-ends-max", "0"), ("--isoforms-ends-max", "33"), ("--isoforms-ends-max-variants", "0"),
                      ("--isoforms-ends-max", "all")):
        r = run(*base, flag, bad, "nothing.cer")
        assert r.returncode == 1 and flag in r.stderr and "must be" in r.stderr, (flag, bad)
    r = run(*base, "--isoforms-ends-slack", "32", "--isoforms-ends-min-over", "1", "--isoforms-ends-min-pct", "100", "--isoforms-ends-max", "32",
            "--isoforms-ends-max-variants", "1", "nothing.cer")
    assert r.returncode == 1 and "--isoforms" not in r.stderr and "must be" not in r.stderr   # (as far as the batch)
    r = run("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--isoforms-ends", "nothing.cer")
    assert r.returncode == 1 and "--isoforms-ends asks for --isoforms" in r.stderr
    r = run(*base, "--isoforms-inserts", "nothing.cer")
    assert r.returncode == 1 and "--isoforms-ends is not offered together with --isoforms-inserts" in r.stderr
    r = run(*base, "--isoforms-polish", "nothing.cer")
    assert r.returncode == 1 and "--isoforms-ends is not offered together with --isoforms-polish" in r.stderr
    h = run("dump", "--help")
    words = " ".join(h.stderr.split())
    assert h.returncode == 0 and all(w in h.stderr for w in ("--isoforms-ends ", "--isoforms-ends-slack", "--isoforms-ends-min-over", "--isoforms-ends-min-pct",
                                                             "--isoforms-ends-max ", "--isoforms-ends-max-variants", "cluster_ends.tsv", "cluster_end_variants.tsv",
                                                             "read_ends.tsv"))
    assert "0 .. 32 (default 10: a choice that was not measured on real data)" in words and "one fused call a run" in words


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("isoforms_ends")
    fq = tmp / "reads.fq"
    T, reads, _ = bc.property_case(bc.SEED, rate=0.01)
    rng = random.Random(4)
    short = [pc.mutate(rng, T[:600], 0.01) for _ in range(8)] + [pc.mutate(rng, T[300:], 0.01) for _ in range(8)]
    with open(fq, "wb") as f:
        rs = synth.generate(30, 3, 400, 12, 21, seed=5)
        for i in range(rs.n):
            s, q = rs.read(i)
            f.write(b"@r%d extra words\n" % i + s + b"\n+\n" + q + b"\n")
        for i, s in enumerate(reads + short):
            f.write(b"@t%d\n" % i + s + b"\n+\n" + bytes([33 + (28 if i == REPRESENTATIVE else 16 + i % 2)]) * len(s) + b"\n")
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
    for with_, without in (("ends", "isoforms"), ("ends_stats", "isoforms_stats"), ("ends_rule", "isoforms")):
        assert set(files[with_]) == set(files[without]) | NEW, with_
        for f in files[without]:
            assert files[with_][f] == files[without][f], (with_, f)
    for f in NEW:
        assert files["ends_stats"][f] == files["ends"][f], f
    assert files["ends_rule"]["cluster_ends.tsv"] != files["ends"]["cluster_ends.tsv"]


@pytest.mark.gpu
def test_the_three_files_are_the_library_call(dumps):
    d = dumps["ends"]
    cons = {int(head.split(b" ")[0][8:]): (seq, qual) for head, seq, qual in _fastq_records(d / "cluster_cons.fq")}
    reads = {cid: (_fastq_records(d / "cluster_fastq" / f"{cid}.fq") if os.path.exists(d / "cluster_fastq" / f"{cid}.fq") else []) for cid in cons}
    lines = [q for _, q in cons.values()] + [q for cid in cons for _, _, q in reads[cid]]
    offs = np.zeros(len(lines) + 1, np.int64)
    offs[1:] = np.cumsum([len(q) for q in lines])
    ctx = api.Context(0)
    _, err = ctx.qual_scores(offs, np.frombuffer(b"".join(lines), np.uint8), K)
    err = [float(e) for e in err]
    cons_err, read_err = dict(zip(cons, err)), iter(err[len(cons):])
    seqs, pairs, sop, segs, seg_cls, pair_of = [], [], [], [], [], {}
    for cid, (ref, _) in cons.items():
        if not reads[cid]:
            continue
        seqs.append(ref)
        segs.append((len(seqs) - 1, 0))
        seg_cls.append(cid)
        for head, s, q in reads[cid]:
            seqs.append(s)
            pair_of[head] = len(pairs)
            pairs.append((len(seqs) - 1, segs[-1][0], 0, next(read_err) + cons_err[cid]))
            sop.append(len(segs) - 1)
    ctx.align_set_pool(seqs)
    rows = [ln.split(b"\t") for ln in open(d / "clusters.tsv", "rb").read().split(b"\n")[1:] if ln]
    rows = [(int(c), rid) for c, _, rid in rows if int(c) in cons]
    assert len(rows) == len(pairs) >= 60
    text = lambda path: open(path).read().split("\n")
    dot = lambda v: "." if int(v) < 0 else int(v)
    for name, rule in RULES.items():
        got = ctx.align_pairs_blocks_ends(pairs, K, segs, sop, rows=False, **rule)
        ends = got["ends"]
        sites, variants = ["ClusterId\tKind\tIndex\tFirst\tEnd\tPeakRow\tPeakReads\tReads\tOver"], ["ClusterId\tVariant\tIsoform\tStartSite\tStopSite\tReads"]
        for g, cid in sorted(enumerate(seg_cls), key=lambda t: t[1]):   # (cluster order)
            z = ends["seg"][g]
            for kind, what in (("starts", "start"), ("stops", "stop")):
                if int(z[f"n_{kind}_found"]) > int(z[f"n_{kind}"]):
                    sites.append(f"# cluster {cid}: kept {int(z[f'n_{kind}'])} of {int(z[f'n_{kind}_found'])} {what} sites")
            for kind, what in (("starts", "start"), ("stops", "stop")):
                for b, k in enumerate(ends[kind][g]):
                    sites.append("\t".join(str(v) for v in (cid, what, b, *(int(k[f]) for f in ("first", "end", "peak_row", "peak_reads", "n_reads", "n_over")))))
            if int(z["n_variants_found"]) > int(z["n_variants"]):
                variants.append(f"# cluster {cid}: kept {int(z['n_variants'])} of {int(z['n_variants_found'])} variants")
            for v, k in enumerate(ends["variants"][g]):
                variants.append("\t".join(str(int(x)) for x in (cid, v, k["pre_group"], k["start_site"], k["stop_site"], k["n_reads"])))
        assert text(dumps[name] / "cluster_ends.tsv") == sites + [""], name
        assert text(dumps[name] / "cluster_end_variants.tsv") == variants + [""], name
        per_read = ["Read\tClusterId\tFirstRow\tEndRow\tHead\tTail\tStartSite\tStopSite\tVariant"]
        for cid, rid in rows:   # (the order of clusters.tsv)
            x = pair_of[rid]
            e, r = got["extents"][x], ends["reads"][x]
            per_read.append("\t".join(str(v) for v in (rid.decode(), cid, *(int(e[f]) for f in e.dtype.names), dot(r["start_site"]), dot(r["stop_site"]), dot(r["variant"]))))
        assert text(dumps[name] / "read_ends.tsv") == per_read + [""], name
        if name == "ends":   # every cluster of at least three reads has a start site and a stop site, and some cluster a variant
            big = [g for g in range(len(segs)) if int(ends["seg"][g]["n_reads"]) >= 10]
            assert big and all(len(ends["starts"][g]) >= 1 and len(ends["stops"][g]) >= 1 for g in big) and int(ends["seg"]["n_variants"].max()) >= 1
        else:
            assert int(ends["seg"]["n_starts"].max()) == 1 and int(ends["seg"]["n_variants"].max()) == 1
    ctx.close()
