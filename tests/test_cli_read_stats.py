"""`dump --read-stats`: the per-read report of how every read fits the representative of its cluster (read_stats.tsv, alignments
reduced to their statistics on the GPU).  Without the option `dump` writes what it always wrote; with it, every row of the report
is recomputed here from the files `dump` wrote alone — the read's record in cluster_fastq/<id>.fq, the cluster's record in
cluster_cons.fq — with the host aligner.  Integers and bytes, no tolerance."""
import os

import numpy as np
import pytest

from isonclust2_amd import _lib, api, synth
from tests.test_cli import _write_fastq, run
from tests.test_align_stats_host import check_identities

pytestmark = pytest.mark.gpu

K = 11  # (`sort`'s default k-mer size: what the batch carries)
HEADER = ("ClusterId Strand Read ReadLen RepLen Score Windows Columns Matches Mismatches Ins Del InsRuns DelRuns LongestIns LongestDel "
          "ReadStart ReadEnd RepStart RepEnd Identity").split()


def _fastq_records(path):
    lines = open(path, "rb").read().split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [(lines[k][1:], lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 1, 4)]


def _files(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            p = os.path.join(d, n)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """3 transcripts x 20 reads of ~400 bases: sort, cluster (fast mode, in this process' child, no resident worker), and the two dumps."""
    tmp = tmp_path_factory.mktemp("read_stats")
    rs = synth.generate(60, 3, 400, 12, 21, seed=5)
    fq = tmp / "reads.fq"
    _write_fastq(rs, fq)
    out = tmp / "sorted"
    r = run("sort", "-o", str(out), str(fq))
    assert r.returncode == 0, r.stderr
    r = run("cluster", "-l", str(out / "batches" / "isONbatch_0.cer"), "-o", str(tmp / "c.cer"), "-x", "fast", env=dict(os.environ, ISONCLUST2_SERVE="0"))
    assert r.returncode == 0, r.stderr
    for name, extra in (("plain", []), ("stats", ["--read-stats"])):
        r = run("dump", "-i", str(out / "sorted_reads_idx.cer"), "-o", str(tmp / name), *extra, str(tmp / "c.cer"))
        assert r.returncode == 0, r.stderr
    return tmp / "plain", tmp / "stats"


def test_without_the_option_nothing_changes(dumps):
    plain, stats = dumps
    a, b = _files(plain), _files(stats)
    assert "read_stats.tsv" not in a and "read_stats.tsv" in b
    del b["read_stats.tsv"]
    assert sorted(a) == sorted(b) and "clusters.tsv" in a and "cluster_cons.fq" in a
    for name in a:
        assert a[name] == b[name], name


def test_every_row_recomputed_from_the_written_files(dumps):
    _, d = dumps
    L = _lib.load()
    cons = {}
    for head, seq, qual in _fastq_records(d / "cluster_cons.fq"):
        name = head.split(b" ")[0]
        assert name.startswith(b"cluster_")
        cons[int(name[8:])] = (seq, qual)
    tsv = [ln.split("\t") for ln in open(d / "clusters.tsv").read().splitlines()]
    assert tsv[0] == ["ClusterId", "Strand", "Read"]
    want_rows = [r for r in tsv[1:] if int(r[0]) in cons]
    rep = [ln.split("\t") for ln in open(d / "read_stats.tsv").read().splitlines()]
    assert rep[0] == HEADER
    rows = rep[1:]
    assert [r[:3] for r in rows] == want_rows and len(rows) >= 50
    assert any(r[1] == "-1" for r in rows), "no read on the other strand: the read set no longer does what it claims"

    reads = {}
    for cid in cons:
        for head, seq, qual in _fastq_records(d / "cluster_fastq" / f"{cid}.fq"):
            reads[(cid, head.decode())] = (seq, qual)
    # CalcErrorRate of every quality line as the files have it (the device's, as `dump` computes it)
    lines = [q for _, q in cons.values()] + [q for _, q in reads.values()]
    offs = np.zeros(len(lines) + 1, np.int64)
    offs[1:] = np.cumsum([len(q) for q in lines])
    ctx = api.Context(0)
    _, err = ctx.qual_scores(offs, np.frombuffer(b"".join(lines), np.uint8), K)
    ctx.close()
    err_of = dict(zip([("c", c) for c in cons] + [("r", key) for key in reads], err))

    flagged = 0
    for r in rows:
        cid, strand, name = int(r[0]), int(r[1]), r[2]
        q, _ = reads[(cid, name)]
        ref, _ = cons[cid]
        e = float(err_of[("r", (cid, name))]) + float(err_of[("c", cid)])
        ops, score = api.host_align_ops(q, ref, gap_open=L.ioc_host_gap_open(e))
        st = api.ops_stats(ops)
        check_identities(st, ops, len(q), len(ref))
        comp = api.ops_to_comp(ops)
        windows = round(L.ioc_host_aln_ratio(comp, len(comp), e, len(q), K) * len(q))
        ident = "%.6f" % (st["matches"] / st["columns"] if st["columns"] else 0.0)
        want = [cid, strand, name, len(q), len(ref), score, windows, st["columns"], st["matches"], st["mismatches"], st["ins"], st["del"],
                st["ins_runs"], st["del_runs"], st["longest_ins"], st["longest_del"], st["lead_i"], len(q) - st["trail_i"], st["lead_d"],
                len(ref) - st["trail_d"], ident]
        assert r == [str(x) for x in want], (r, want)
        flagged += st["columns"] > 0
    assert flagged == len(rows)  # (reads of 400 bases against the representative of their own cluster: every one has a walk)
