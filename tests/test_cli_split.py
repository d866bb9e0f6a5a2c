"""`dump --split`: cluster_split.tsv and read_split.tsv (ioc_align_pairs_split on the GPU).  The options are parsed and refused
without a GPU.  On a small read set that holds the two-haplotype case of tests/sites_common.py among ordinary transcripts, both
files are recomputed from the files `dump` wrote alone — reads as cluster_fastq/<id>.fq has them, the representative as
cluster_cons.fq has it — through Context.align_pairs_split; the 6 + 5 reads of the haplotypes land in two groups of 6 and 5; and
the reports of the other options do not change by one byte when --split stands beside them."""
import os

import numpy as np
import pytest

from isonclust2_amd import api, synth
from tests import sites_common as sc
from tests.test_cli import run
from tests.test_cli_read_stats import K, _fastq_records, _files

NAMES = {"split": ["--split"], "all": ["--split", "--sites", "--read-stats", "--pileup"], "reports": ["--sites", "--read-stats", "--pileup"],
         "strict": ["--split", "--split-min-link", "12", "--split-min-margin", "2", "--split-rounds", "0"],
         "loose": ["--split", "--sites-min-depth", "2", "--sites-min-alt", "2", "--sites-min-pct", "10", "--split-min-link", "2"],
         "polish": ["--split", "--polish"], "polish_alone": ["--polish"]}
RULES = {"split": ((3, 3, 25, 4096), (3, 1, 2)), "strict": ((3, 3, 25, 4096), (12, 2, 0)), "loose": ((2, 2, 10, 4096), (2, 1, 2))}


@pytest.mark.parametrize("args, word", [(["--split-min-link", "0"], "--split-min-link"), (["--split-min-link", "x"], "--split-min-link"),
                                        (["--split-min-margin", "0"], "--split-min-margin"), (["--split-min-margin", "2x"], "--split-min-margin"),
                                        (["--split-rounds", "-1"], "--split-rounds"), (["--split-rounds", "65"], "--split-rounds"),
                                        (["--split-rounds", ""], "--split-rounds"), (["--split-min-link", "99999999999999999999"], "--split-min-link"),
                                        (["--sites-min-pct", "51"], "--sites-min-pct")])
def test_malformed_values_die_with_a_message(tmp_path, args, word):
    r = run("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--split", *args, "nothing.cer")
    assert r.returncode == 1 and word in r.stderr and "must be" in r.stderr


def test_well_formed_values_get_as_far_as_the_batch(tmp_path):
    r = run("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--split", "--split-min-link", "1", "--split-min-margin", "7", "--split-rounds", "64",
            "--sites-min-alt", "2", "nothing.cer")
    assert r.returncode == 1 and "--split" not in r.stderr and "must be" not in r.stderr
    r = run("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--split", "--split-rounds", "0", "nothing.cer")
    assert r.returncode == 1 and "--split" not in r.stderr and "must be" not in r.stderr
    h = run("dump", "--help")
    assert h.returncode == 0 and all(w in h.stderr for w in ("--split ", "--split-min-link", "--split-min-margin", "--split-rounds", "cluster_split.tsv",
                                                             "read_split.tsv"))


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """3 transcripts x 10 reads of ~400 bases and the 6 + 5 reads of the two haplotypes: sort, cluster (fast mode), the dumps."""
    tmp = tmp_path_factory.mktemp("split")
    fq = tmp / "reads.fq"
    T, B, reads = sc.haplotypes()
    with open(fq, "wb") as f:
        rs = synth.generate(30, 3, 400, 12, 21, seed=5)
        for i in range(rs.n):
            s, q = rs.read(i)
            f.write(b"@r%d extra words\n" % i + s + b"\n+\n" + q + b"\n")
        for i, s in enumerate(reads):
            f.write(b"@h%d\n" % i + s + b"\n+\n" + bytes([33 + 30 + i % 3]) * len(s) + b"\n")
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
    new = {"cluster_split.tsv", "read_split.tsv"}
    assert set(files["all"]) == set(files["reports"]) | new
    assert set(files["split"]) == set(files["all"]) - {"read_stats.tsv", "cluster_pileup.tsv", "cluster_sites.tsv", "read_alleles.tsv"}
    for f in files["reports"]:
        assert files["all"][f] == files["reports"][f], f
    for f in new:
        assert files["all"][f] == files["split"][f] == files["polish"][f], f
    assert files["polish"]["cluster_polished.fq"] == files["polish_alone"]["cluster_polished.fq"]


@pytest.mark.gpu
def test_both_files_recomputed_from_the_written_files(dumps):
    d = dumps["split"]
    cons = {int(head.split(b" ")[0][8:]): (seq, qual) for head, seq, qual in _fastq_records(d / "cluster_cons.fq")}
    tsv = [ln.split("\t") for ln in open(d / "clusters.tsv").read().splitlines()]
    want_rows = [r for r in tsv[1:] if int(r[0]) in cons]
    reads = {cid: (_fastq_records(d / "cluster_fastq" / f"{cid}.fq") if os.path.exists(d / "cluster_fastq" / f"{cid}.fq") else []) for cid in cons}
    lines = [q for _, q in cons.values()] + [q for cid in cons for _, _, q in reads[cid]]
    offs = np.zeros(len(lines) + 1, np.int64)
    offs[1:] = np.cumsum([len(q) for q in lines])
    ctx = api.Context(0)
    _, err = ctx.qual_scores(offs, np.frombuffer(b"".join(lines), np.uint8), K)
    err = [float(e) for e in err]
    cons_err, read_err = dict(zip(cons, err)), iter(err[len(cons):])
    # one call: a segment per cluster with reads
    seqs, pairs, sop, names, segs, seg_cid = [], [], [], [], [], []
    for cid, (ref, _) in cons.items():
        if not reads[cid]:
            continue
        seqs.append(ref)
        segs.append((len(seqs) - 1, 0))
        seg_cid.append(cid)
        for head, s, _ in reads[cid]:
            seqs.append(s)
            pairs.append((len(seqs) - 1, segs[-1][0], 0, next(read_err) + cons_err[cid]))
            sop.append(len(segs) - 1)
            names.append((cid, head.decode()))
    ctx.align_set_pool(seqs)
    hap = next(cid for cid in cons if any(h.startswith(b"h") for h, _, _ in reads[cid]))
    for name, ((md, ma, mp, mx), (ml, mm, rounds)) in RULES.items():
        got = ctx.align_pairs_split(pairs, K, segs, sop, md, ma, mp, mx, ml, mm, rounds)
        want = ["ClusterId\tNSites\tNLinked\tSeedPos\tSeedKind\tNReads\tNGroup0\tNGroup1\tNNone"]
        for cid in cons:
            if cid not in seg_cid:
                want.append(f"{cid}\t0\t0\t.\t.\t0\t0\t0\t0")
                continue
            g = seg_cid.index(cid)
            z, s = got["seg"][g], got["sites"][g]
            seed = int(z["seed"])
            where = (str(int(s[seed]["row"])), "ins" if int(s[seed]["kind"]) == sc.INS else "base") if seed >= 0 else (".", ".")
            want.append("\t".join(str(x) for x in (cid, len(s), int(z["n_linked"]), *where, int(z["n_reads"]), int(z["n_group0"]), int(z["n_group1"]),
                                                   int(z["n_none"]))))
        assert open(dumps[name] / "cluster_split.tsv").read().splitlines() == want, name
        mine = {key: ("." if g == api.SPLIT_NONE else str(g), str(v)) for key, g, v in zip(names, got["group"].tolist(), got["vote"].tolist())}
        rows = [ln.split("\t") for ln in open(dumps[name] / "read_split.tsv").read().splitlines()]
        assert rows[0] == ["Read", "ClusterId", "Group", "Vote"]
        assert [(r[1], r[0]) for r in rows[1:]] == [(r[0], r[2]) for r in want_rows]       # one row per row of read_stats.tsv, in its order
        assert [(r[2], r[3]) for r in rows[1:]] == [mine[(int(r[1]), r[0])] for r in rows[1:]], name
        z = got["seg"][seg_cid.index(hap)]
        if name == "split":
            # the closed form: the haplotypes' cluster falls into the 6 reads of one haplotype and the 5 of the other — the minor
            # allele's side is group 1 —, every site linked; the other clusters' reads disagree nowhere systematically
            assert len(reads[hap]) == 11 and (int(z["n_group0"]), int(z["n_group1"]), int(z["n_none"])) == (6, 5, 0)
            assert int(z["n_linked"]) == len(got["sites"][seg_cid.index(hap)]) >= 4
            by_group = {}
            for r in rows[1:]:
                if int(r[1]) == hap:
                    by_group.setdefault(r[2], set()).add(int(r[0][1:]) < 6)
            assert by_group in ({"0": {True}, "1": {False}}, {"0": {False}, "1": {True}})
            assert all(int(s["seed"]) == -1 for g, s in enumerate(got["seg"]) if seg_cid[g] != hap)
        if name == "strict":
            # 11 reads cannot link two sites by 12: no split anywhere
            assert int(z["seed"]) == -1 and all(r[2] == "." and r[3] == "0" for r in rows[1:])
    ctx.close()
