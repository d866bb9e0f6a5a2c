"""`dump --pileup`: the per-position report of what the reads of a cluster say along their representative (cluster_pileup.tsv,
alignments piled on the GPU).  Without the option `dump` writes what it always wrote; with it, every row of the report is
recomputed here from the files `dump` wrote alone — the reads in cluster_fastq/<id>.fq, the representative in cluster_cons.fq —
with the host aligner and ioc_host_ops_pileup; with --read-stats beside it both reports are those of each option alone.
Integers and bytes, no tolerance.  The read set is that of tests/test_cli_read_stats.py."""
import os

import numpy as np
import pytest

from isonclust2_amd import _lib, api, synth
from tests.test_cli import _write_fastq, run
from tests.test_cli_read_stats import K, _fastq_records, _files

pytestmark = pytest.mark.gpu

HEADER = "ClusterId Pos RepBase Depth A C G T N Del InsReads InsBases".split()


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """3 transcripts x 20 reads of ~400 bases: sort, cluster (fast mode, no resident worker), and the four dumps."""
    tmp = tmp_path_factory.mktemp("pileup")
    rs = synth.generate(60, 3, 400, 12, 21, seed=5)
    fq = tmp / "reads.fq"
    _write_fastq(rs, fq)
    out = tmp / "sorted"
    r = run("sort", "-o", str(out), str(fq))
    assert r.returncode == 0, r.stderr
    r = run("cluster", "-l", str(out / "batches" / "isONbatch_0.cer"), "-o", str(tmp / "c.cer"), "-x", "fast", env=dict(os.environ, ISONCLUST2_SERVE="0"))
    assert r.returncode == 0, r.stderr
    names = {"plain": [], "stats": ["--read-stats"], "pileup": ["--pileup"], "both": ["--read-stats", "--pileup"]}
    for name, extra in names.items():
        r = run("dump", "-i", str(out / "sorted_reads_idx.cer"), "-o", str(tmp / name), *extra, str(tmp / "c.cer"))
        assert r.returncode == 0, r.stderr
    return {name: tmp / name for name in names}


def test_without_the_option_nothing_changes(dumps):
    files = {name: _files(d) for name, d in dumps.items()}
    plain = files["plain"]
    assert "cluster_pileup.tsv" not in plain and "read_stats.tsv" not in plain and "clusters.tsv" in plain and "cluster_cons.fq" in plain
    extra = {"plain": set(), "stats": {"read_stats.tsv"}, "pileup": {"cluster_pileup.tsv"}, "both": {"read_stats.tsv", "cluster_pileup.tsv"}}
    for name, got in files.items():
        assert set(got) == set(plain) | extra[name], name
        for f in plain:
            assert got[f] == plain[f], (name, f)


def test_both_options_give_the_reports_of_each_alone(dumps):
    stats, pileup, both = (_files(dumps[n]) for n in ("stats", "pileup", "both"))
    assert both["read_stats.tsv"] == stats["read_stats.tsv"]
    assert both["cluster_pileup.tsv"] == pileup["cluster_pileup.tsv"]


def test_every_row_recomputed_from_the_written_files(dumps):
    d = dumps["pileup"]
    L = _lib.load()
    cons = {}
    for head, seq, qual in _fastq_records(d / "cluster_cons.fq"):
        name = head.split(b" ")[0]
        assert name.startswith(b"cluster_")
        cons[int(name[8:])] = (seq, qual)
    assert list(cons) == sorted(cons) and len(cons) >= 3
    reads = {cid: _fastq_records(d / "cluster_fastq" / f"{cid}.fq") for cid in cons}
    # CalcErrorRate of every quality line as the files have it (the device's, as `dump` computes it)
    lines = [q for _, q in cons.values()] + [q for cid in cons for _, _, q in reads[cid]]
    offs = np.zeros(len(lines) + 1, np.int64)
    offs[1:] = np.cumsum([len(q) for q in lines])
    ctx = api.Context(0)
    _, err = ctx.qual_scores(offs, np.frombuffer(b"".join(lines), np.uint8), K)
    ctx.close()
    err = [float(e) for e in err]
    cons_err, read_err = dict(zip(cons, err)), iter(err[len(cons):])

    want = []
    for cid, (ref, _) in cons.items():
        cols = np.zeros(len(ref) + 1, api.PILEUP_DTYPE)
        for _, q, _ in reads[cid]:
            ops, _ = api.host_align_ops(q, ref, gap_open=L.ioc_host_gap_open(next(read_err) + cons_err[cid]))
            api.ops_pileup(ops, q, len(ref), cols=cols)
        for p in range(len(ref) + 1):
            c = cols[p]
            depth = sum(int(c[f]) for f in ("a", "c", "g", "t", "other", "del"))
            want.append([cid, p, chr(ref[p]) if p < len(ref) else "-", depth, c["a"], c["c"], c["g"], c["t"], c["other"], c["del"], c["ins_runs"],
                         c["ins_bases"]])
    rep = [ln.split("\t") for ln in open(d / "cluster_pileup.tsv").read().splitlines()]
    assert rep[0] == HEADER
    rows = rep[1:]
    assert len(rows) == sum(len(ref) + 1 for ref, _ in cons.values())  # length + 1 rows per cluster
    assert rows == [[str(x) for x in w] for w in want]
    for r in rows:
        assert int(r[3]) == sum(int(x) for x in r[4:10])  # Depth = A + C + G + T + N + Del
    assert max(int(r[3]) for r in rows) >= 15 and sum(int(r[9]) for r in rows) > 0 and sum(int(r[10]) for r in rows) > 0
