"""`dump --isoforms --isoforms-inserts`: cluster_inserts.tsv and read_inserts.tsv (ioc_align_pairs_blocks_inserts on the GPU).  The
options are parsed and refused without a GPU.  The read set is that of test_cli_isoforms.py, with one difference: the read that
represents its cluster is one of the isoform that lacks [150, 190) — so `--isoforms` alone sees one block, [400, 520), and two
isoforms, and the first exon is an insertion site that splits one of them.  (The sort's score grows with a read's length: the
960-base read at quality 28 comes first because the qualities of the others say 2 to 2.5 % errors.  The fast mode puts only some
of the 1000-base reads into that read's cluster, and none into the cluster of a read that lacks both exons, 160 bases of it: what
is asked of the planted cluster is the block, the site and more isoforms with the sites than without.)
The two files are recomputed through Context.align_pairs_blocks_inserts from the files `dump` wrote alone.  The three files of
--isoforms, and every other report file, do not change by one byte when the option stands beside them."""
import os

import numpy as np
import pytest

from isonclust2_amd import api, synth
from tests import blocks_common as bc
from tests.test_cli import run
from tests.test_cli_read_stats import K, _fastq_records, _files

NAMES = {"isoforms": ["--isoforms"], "inserts": ["--isoforms", "--isoforms-inserts"],
         "isoforms_stats": ["--isoforms", "--read-stats", "--pileup"], "inserts_stats": ["--isoforms", "--isoforms-inserts", "--read-stats", "--pileup"],
         "inserts_rule": ["--isoforms", "--isoforms-inserts", "--isoforms-min-ins", "30", "--isoforms-ins-slack", "3", "--isoforms-ins-max", "1"]}
RULES = {"inserts": {}, "inserts_rule": dict(min_ins=30, slack=3, max_sites=1)}
NEW = {"cluster_inserts.tsv", "read_inserts.tsv"}
REPRESENTATIVE = bc.SIZES[0]   # the first read of the isoform without [150, 190)


def test_the_options_are_parsed_and_in_the_help(tmp_path):
    base = ("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--isoforms", "--isoforms-inserts")
    for flag, bad in (("--isoforms-min-ins", "0"), ("--isoforms-min-ins", "256"), ("--isoforms-ins-slack", "-1"), ("--isoforms-ins-slack", "33"),
                      ("--isoforms-ins-max", "0"), ("--isoforms-ins-max", "33"), ("--isoforms-ins-max", "all")):
        r = run(*base, flag, bad, "nothing.cer")
        assert r.returncode == 1 and flag in r.stderr and "must be" in r.stderr, (flag, bad)
    r = run(*base, "--isoforms-min-ins", "255", "--isoforms-ins-slack", "0", "--isoforms-ins-max", "32", "nothing.cer")
    assert r.returncode == 1 and "--isoforms" not in r.stderr and "must be" not in r.stderr   # (as far as the batch)
    r = run("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--isoforms-inserts", "nothing.cer")
    assert r.returncode == 1 and "--isoforms-inserts asks for --isoforms" in r.stderr
    p = run("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--isoforms-polish", "nothing.cer")
    assert p.returncode == 1 and "--isoforms-polish asks for --isoforms" in p.stderr        # (it dies as that one does)
    r = run(*base, "--isoforms-polish", "nothing.cer")
    assert r.returncode == 1 and "not offered together with --isoforms-polish" in r.stderr
    h = run("dump", "--help")
    words = " ".join(h.stderr.split())
    assert h.returncode == 0 and all(w in h.stderr for w in ("--isoforms-inserts ", "--isoforms-min-ins", "--isoforms-ins-slack", "--isoforms-ins-max",
                                                             "cluster_inserts.tsv", "read_inserts.tsv"))
    assert "(default 20: a choice that was not measured on real data)" in words and "a choice that was not measured on real data) --isoforms-ins-max" in words
    assert "0 .. 32 (default 8:" in words


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("isoforms_inserts")
    fq = tmp / "reads.fq"
    _, reads, _ = bc.property_case(bc.SEED, rate=0.01)
    with open(fq, "wb") as f:
        rs = synth.generate(30, 3, 400, 12, 21, seed=5)
        for i in range(rs.n):
            s, q = rs.read(i)
            f.write(b"@r%d extra words\n" % i + s + b"\n+\n" + q + b"\n")
        for i, s in enumerate(reads):
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
    for with_, without in (("inserts", "isoforms"), ("inserts_stats", "isoforms_stats"), ("inserts_rule", "isoforms")):
        assert set(files[with_]) == set(files[without]) | NEW, with_
        for f in files[without]:
            assert files[with_][f] == files[without][f], (with_, f)
    for f in NEW:
        assert files["inserts_stats"][f] == files["inserts"][f], f
    assert files["inserts_rule"]["cluster_inserts.tsv"] != files["inserts"]["cluster_inserts.tsv"]


@pytest.mark.gpu
def test_the_two_files_are_the_library_call(dumps):
    d = dumps["inserts"]
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
    how = ("direct", "assigned", "rare", "ambiguous")
    sig = lambda key, n: "".join("=+?."[(int(key) >> (2 * b)) & 3] for b in range(n)) or "*"
    for name, rule in RULES.items():
        got = ctx.align_pairs_blocks_inserts(pairs, K, segs, sop, rows=False, **rule)
        ins = got["inserts"]
        sites = ["ClusterId\tFirst\tEnd\tCarry\tLack\tNone\tLenMin\tLenMax"]
        for g, cid in sorted(enumerate(seg_cls), key=lambda t: t[1]):   # (cluster order)
            z = ins["seg"][g]
            if int(z["n_found"]) > int(z["n_sites"]):
                sites.append(f"# cluster {cid}: kept {int(z['n_sites'])} of {int(z['n_found'])} sites")
            for k in ins["sites"][g]:
                sites.append("\t".join(str(int(v)) for v in (cid, k["first"], k["end"], k["n_carry"], k["n_lack"], k["n_none"], k["len_min"], k["len_max"])))
        assert text(dumps[name] / "cluster_inserts.tsv") == sites + [""], name
        per_read = ["ClusterId\tRead\tInserts\tIsoform\tHow"]
        for cid, rid in rows:   # (the order of clusters.tsv)
            x = pair_of[rid]
            r, n = ins["reads"][x], int(ins["seg"][sop[x]]["n_sites"])
            per_read.append("\t".join(str(v) for v in (cid, rid.decode(), sig(r["key"], n), "." if r["group"] < 0 else int(r["group"]), how[int(r["how"])])))
        assert text(dumps[name] / "read_inserts.tsv") == per_read + [""], name
        if name == "inserts":   # the planted transcript: the cluster of the read in front has the block [400, 520) and the first exon as a site
            planted = [g for g in range(len(segs)) if int(ins["seg"][g]["n_sites"]) >= 1]
            assert len(planted) == 1, ins["seg"]
            z, zi, site = got["seg"][planted[0]], ins["seg"][planted[0]], ins["sites"][planted[0]][0]
            assert int(z["n_blocks"]) == 1 and int(zi["n_sites"]) == 1 and int(zi["n_groups"]) > int(z["n_groups"]) == 2, (z, zi)
            assert int(site["first"]) <= 150 < int(site["end"]) and 36 <= int(site["len_min"]) <= int(site["len_max"]) <= 44, site
            assert int(site["n_carry"]) >= 3 and int(site["n_lack"]) >= 3
        else:
            assert int(ins["seg"]["n_sites"].max()) == 1 and sites != ["ClusterId\tFirst\tEnd\tCarry\tLack\tNone\tLenMin\tLenMax"]
    ctx.close()
