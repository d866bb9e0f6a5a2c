"""`dump --polish`: one polished record per record of cluster_cons.fq (cluster_polished.fq: both pileup tables and the consensus
call on the GPU, only the sequences come back).  Without the option `dump` writes what it always wrote; with it, every record is
recomputed here from the files `dump` wrote alone — the reads in cluster_fastq/<id>.fq, the representative in cluster_cons.fq —
with the host aligner and the two host definitions (ioc_host_ops_pileup_ins, ioc_host_pileup_call); with --pileup and
--read-stats beside it the three reports are those of each option alone.  Bytes only, no tolerance.  The read set is that of
tests/test_cli_pileup.py with three reads of two more transcripts: clusters of one and two reads, where a minimum depth of 1
calls what the default of 3 leaves as it is."""
import os

import numpy as np
import pytest

from isonclust2_amd import _lib, api, synth
from tests.test_cli import run
from tests.test_cli_read_stats import K, _fastq_records, _files

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """3 transcripts x 20 reads of ~400 bases and 2 + 1 reads of two more: sort, cluster (fast mode, no resident worker), dumps."""
    tmp = tmp_path_factory.mktemp("polish")
    fq = tmp / "reads.fq"
    with open(fq, "wb") as f:
        for tag, rs in ((b"r", synth.generate(60, 3, 400, 12, 21, seed=5)), (b"s", synth.generate(2, 1, 400, 12, 21, seed=9)),
                        (b"t", synth.generate(1, 1, 400, 12, 21, seed=10))):
            for i in range(rs.n):
                s, q = rs.read(i)
                f.write(b"@%s%d extra words\n" % (tag, i) + s + b"\n+\n" + q + b"\n")
    out = tmp / "sorted"
    r = run("sort", "-o", str(out), str(fq))
    assert r.returncode == 0, r.stderr
    r = run("cluster", "-l", str(out / "batches" / "isONbatch_0.cer"), "-o", str(tmp / "c.cer"), "-x", "fast", env=dict(os.environ, ISONCLUST2_SERVE="0"))
    assert r.returncode == 0, r.stderr
    names = {"plain": [], "stats": ["--read-stats"], "pileup": ["--pileup"], "polish": ["--polish"], "depth1": ["--polish", "--polish-min-depth", "1"],
             "all": ["--pileup", "--read-stats", "--polish"]}
    for name, extra in names.items():
        r = run("dump", "-i", str(out / "sorted_reads_idx.cer"), "-o", str(tmp / name), *extra, str(tmp / "c.cer"))
        assert r.returncode == 0, r.stderr
    return {name: tmp / name for name in names}


def test_without_the_option_nothing_changes(dumps):
    files = {name: _files(d) for name, d in dumps.items()}
    plain = files["plain"]
    assert "cluster_polished.fq" not in plain and "clusters.tsv" in plain and "cluster_cons.fq" in plain
    extra = {"plain": set(), "stats": {"read_stats.tsv"}, "pileup": {"cluster_pileup.tsv"}, "polish": {"cluster_polished.fq"},
             "depth1": {"cluster_polished.fq"}, "all": {"read_stats.tsv", "cluster_pileup.tsv", "cluster_polished.fq"}}
    for name, got in files.items():
        assert set(got) == set(plain) | extra[name], name
        for f in plain:
            assert got[f] == plain[f], (name, f)


def test_three_options_give_the_reports_of_each_alone(dumps):
    stats, pileup, polish, both = (_files(dumps[n]) for n in ("stats", "pileup", "polish", "all"))
    assert both["read_stats.tsv"] == stats["read_stats.tsv"]
    assert both["cluster_pileup.tsv"] == pileup["cluster_pileup.tsv"]
    assert both["cluster_polished.fq"] == polish["cluster_polished.fq"]


def test_bad_min_depth_is_refused(dumps, tmp_path):
    r = run("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--polish", "--polish-min-depth", "0", "nothing.cer")
    assert r.returncode != 0 and "polish-min-depth" in r.stderr


def test_every_record_recomputed_from_the_written_files(dumps):
    d = dumps["polish"]
    L = _lib.load()
    cons = {}
    for head, seq, qual in _fastq_records(d / "cluster_cons.fq"):
        name = head.split(b" ")[0]
        assert name.startswith(b"cluster_")
        cons[int(name[8:])] = (seq, qual)
    assert list(cons) == sorted(cons) and len(cons) >= 4
    reads = {cid: (_fastq_records(d / "cluster_fastq" / f"{cid}.fq") if os.path.exists(d / "cluster_fastq" / f"{cid}.fq") else []) for cid in cons}
    lines = [q for _, q in cons.values()] + [q for cid in cons for _, _, q in reads[cid]]
    offs = np.zeros(len(lines) + 1, np.int64)
    offs[1:] = np.cumsum([len(q) for q in lines])
    ctx = api.Context(0)
    _, err = ctx.qual_scores(offs, np.frombuffer(b"".join(lines), np.uint8), K)
    ctx.close()
    err = [float(e) for e in err]
    cons_err, read_err = dict(zip(cons, err)), iter(err[len(cons):])

    want = {1: [], 3: []}
    for cid, (ref, _) in cons.items():
        cols, ins = np.zeros(len(ref) + 1, api.PILEUP_DTYPE), np.zeros(len(ref) + 1, api.PILEUP_INS_DTYPE)
        for _, q, _ in reads[cid]:
            ops, _ = api.host_align_ops(q, ref, gap_open=L.ioc_host_gap_open(next(read_err) + cons_err[cid]))
            api.ops_pileup(ops, q, len(ref), cols=cols)
            api.ops_pileup_ins(ops, q, len(ref), ins=ins)
        for md in (1, 3):
            seq, qual, st = api.pileup_call(cols, ins, ref, md)
            head = b"cluster_%d reads=%d subs=%d dels=%d ins=%d low=%d" % (cid, len(reads[cid]), st["n_sub"], st["n_del"], st["n_ins"], st["n_low"])
            want[md].append((head, seq, qual))
    assert _fastq_records(d / "cluster_polished.fq") == want[3]
    assert _fastq_records(dumps["depth1"] / "cluster_polished.fq") == want[1]
    # the fixture was chosen so that the minimum depth matters: a cluster of one or two reads is called at 1 and kept at 3
    differ = [a[0] for a, b in zip(want[1], want[3]) if a != b]
    assert differ and len(differ) < len(cons), differ
    assert any(st_seq != cons[cid][0] for (_, st_seq, _), cid in zip(want[3], cons)), "no cluster was changed by the call"
