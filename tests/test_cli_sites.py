"""`dump --sites`: cluster_sites.tsv and read_alleles.tsv (ioc_align_pairs_alleles on the GPU).  The options are parsed and refused
without a GPU.  On a small read set that holds the two-haplotype case of tests/sites_common.py among ordinary transcripts, both
files are recomputed from the files `dump` wrote alone — reads as cluster_fastq/<id>.fq has them, the representative as
cluster_cons.fq has it — through Context.align_pairs_alleles, and the reports of the other options do not change by one byte
when --sites stands beside them."""
import os

import numpy as np
import pytest

from isonclust2_amd import api, synth
from tests import sites_common as sc
from tests.align_ops_checks import revcomp
from tests.test_cli import run
from tests.test_cli_read_stats import K, _fastq_records, _files

NAMES = {"sites": ["--sites"], "all": ["--sites", "--read-stats", "--pileup"], "reports": ["--read-stats", "--pileup"],
         "cut": ["--sites", "--sites-max", "2"], "loose": ["--sites", "--sites-min-depth", "2", "--sites-min-alt", "2", "--sites-min-pct", "10"],
         "polish": ["--sites", "--polish"], "polish_alone": ["--polish"]}
RULES = {"sites": (3, 3, 25, 4096), "cut": (3, 3, 25, 2), "loose": (2, 2, 10, 4096)}


@pytest.mark.parametrize("args, word", [(["--sites-min-depth", "0"], "--sites-min-depth"), (["--sites-min-depth", "x"], "--sites-min-depth"),
                                        (["--sites-min-alt", "0"], "--sites-min-alt"), (["--sites-min-alt", "3x"], "--sites-min-alt"),
                                        (["--sites-min-pct", "0"], "--sites-min-pct"), (["--sites-min-pct", "51"], "--sites-min-pct"),
                                        (["--sites-min-pct", ""], "--sites-min-pct"), (["--sites-max", "0"], "--sites-max"),
                                        (["--sites-max", "-4"], "--sites-max"), (["--sites-max", "99999999999999999999"], "--sites-max")])
def test_malformed_values_die_with_a_message(tmp_path, args, word):
    r = run("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--sites", *args, "nothing.cer")
    assert r.returncode == 1 and word in r.stderr and "must be" in r.stderr


def test_well_formed_values_get_as_far_as_the_batch(tmp_path):
    r = run("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--sites", "--sites-min-depth", "1", "--sites-min-alt", "7", "--sites-min-pct", "50",
            "--sites-max", "1", "nothing.cer")
    assert r.returncode == 1 and "--sites" not in r.stderr and "must be" not in r.stderr
    h = run("dump", "--help")
    assert h.returncode == 0 and all(w in h.stderr for w in ("--sites ", "--sites-min-depth", "--sites-min-alt", "--sites-min-pct", "--sites-max", "second time"))


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """3 transcripts x 10 reads of ~400 bases and the 6 + 5 reads of the two haplotypes: sort, cluster (fast mode), the dumps."""
    tmp = tmp_path_factory.mktemp("sites")
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
    new = {"cluster_sites.tsv", "read_alleles.tsv"}
    assert set(files["all"]) == set(files["reports"]) | new and set(files["sites"]) == set(files["all"]) - {"read_stats.tsv", "cluster_pileup.tsv"}
    for f in files["reports"]:
        assert files["all"][f] == files["reports"][f], f
    for f in new:
        assert files["all"][f] == files["sites"][f] == files["polish"][f], f
    assert files["polish"]["cluster_polished.fq"] == files["polish_alone"]["cluster_polished.fq"]


def _letters(kind, alleles):
    return "".join(("." if a == 0 else "+" if a == 1 else "?") if kind[s] == sc.INS else ("ACGTN-"[a] if a <= 5 else "?") for s, a in enumerate(alleles))


@pytest.mark.gpu
def test_both_files_recomputed_from_the_written_files(dumps):
    d = dumps["sites"]
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
    for name, (md, ma, mp, mx) in RULES.items():
        got = ctx.align_pairs_alleles(pairs, K, segs, sop, md, ma, mp, mx)
        want_sites = ["ClusterId\tPos\tKind\tDepth\tMajor\tNMajor\tMinor\tNMinor"]
        for g, cid in enumerate(seg_cid):
            s = got["sites"][g]
            if int(got["n_found"][g]) > len(s):
                want_sites.append(f"# cluster {cid}: kept {len(s)} of {int(got['n_found'][g])} sites")
            for t in s:
                ins = int(t["kind"]) == sc.INS
                want_sites.append("\t".join(str(x) for x in (cid, int(t["row"]), "ins" if ins else "base", int(t["depth"]), (".+" if ins else "ACGTN-")[int(t["major"])],
                                                             int(t["n_major"]), (".+" if ins else "ACGTN-")[int(t["minor"])], int(t["n_minor"]))))
        assert open(dumps[name] / "cluster_sites.tsv").read().splitlines() == want_sites, name
        letters = {key: (_letters(got["sites"][g]["kind"], a.tolist()) or "*") for key, g, a in zip(names, sop, got["alleles"])}
        rows = [ln.split("\t") for ln in open(dumps[name] / "read_alleles.tsv").read().splitlines()]
        assert rows[0] == ["Read", "ClusterId", "Alleles"]
        assert [(r[1], r[0]) for r in rows[1:]] == [(r[0], r[2]) for r in want_rows]       # one row per row of read_stats.tsv, in its order
        assert [r[2] for r in rows[1:]] == [letters[(int(r[1]), r[0])] for r in rows[1:]], name
        if name == "sites":
            # the closed form: the haplotypes' cluster has the known sites of whichever read became its representative, and two
            # kinds of rows that differ in every character; the other clusters' reads disagree nowhere systematically
            g = seg_cid.index(hap)
            ref = cons[hap][0]
            assert ref in (sc.haplotypes()[0], sc.haplotypes()[1], revcomp(sc.haplotypes()[0]), revcomp(sc.haplotypes()[1]))
            assert len(got["sites"][g]) == (5 if len(ref) == 300 else 4) and len(reads[hap]) == 11
            mine = sorted({r[2] for r in rows[1:] if int(r[1]) == hap})
            assert len(mine) == 2 and all(a != b for a, b in zip(*mine)) and "?" not in mine[0] + mine[1]
            assert any(r[2] == "*" for r in rows[1:])
        if name == "cut":
            assert f"# cluster {hap}: kept 2 of" in "\n".join(want_sites)
    ctx.close()
