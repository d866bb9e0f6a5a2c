"""`dump --polish --polish-weighted`: cluster_polished.fq called by weight (ioc_align_pairs_polish_weighted on the GPU).  Without the
option not one byte of `dump --polish` changes; with it only cluster_polished.fq does, and every one of its records is recomputed
here from the files `dump` wrote alone — reads and quality lines as cluster_fastq/<id>.fq has them, the representative as
cluster_cons.fq has it — with the host aligner and the host definitions (ioc_host_ops_pileup, ioc_host_ops_pileup_weighted,
ioc_host_pileup_call_weighted).  Bytes only, no tolerance.  The read set is that of tests/test_cli_polish.py with one more
transcript whose qualities are informative: the closed-form case of tests/polish_weight_common.py at 400 bases, three doubtful
reads against two confident ones, where the weighted call provably differs from the majority call."""
import os

import numpy as np
import pytest

from isonclust2_amd import _lib, api, synth
from tests import polish_weight_common as pw
from tests.align_ops_checks import revcomp
from tests.test_cli import run
from tests.test_cli_read_stats import K, _fastq_records, _files

pytestmark = pytest.mark.gpu

NAMES = {"polish": ["--polish"], "weighted": ["--polish", "--polish-weighted"], "depth1": ["--polish", "--polish-weighted", "--polish-min-depth", "1"],
         "all": ["--pileup", "--read-stats", "--polish", "--polish-weighted"], "reports": ["--pileup", "--read-stats"]}


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """The reads of test_cli_polish.py and the five of the closed-form case: sort, cluster (fast mode, no resident worker), dumps."""
    tmp = tmp_path_factory.mktemp("polish_weighted")
    fq = tmp / "reads.fq"
    T, edited, reads, quals = pw.closed_form(400, seed=400)
    with open(fq, "wb") as f:
        for tag, rs in ((b"r", synth.generate(60, 3, 400, 12, 21, seed=5)), (b"s", synth.generate(2, 1, 400, 12, 21, seed=9)),
                        (b"t", synth.generate(1, 1, 400, 12, 21, seed=10))):
            for i in range(rs.n):
                s, q = rs.read(i)
                f.write(b"@%s%d extra words\n" % (tag, i) + s + b"\n+\n" + q + b"\n")
        for i, (s, q) in enumerate(zip(reads, quals)):
            f.write(b"@w%d\n" % i + s + b"\n+\n" + q + b"\n")
    out = tmp / "sorted"
    r = run("sort", "-o", str(out), str(fq))
    assert r.returncode == 0, r.stderr
    r = run("cluster", "-l", str(out / "batches" / "isONbatch_0.cer"), "-o", str(tmp / "c.cer"), "-x", "fast", env=dict(os.environ, ISONCLUST2_SERVE="0"))
    assert r.returncode == 0, r.stderr
    for name, extra in NAMES.items():
        r = run("dump", "-i", str(out / "sorted_reads_idx.cer"), "-o", str(tmp / name), *extra, str(tmp / "c.cer"))
        assert r.returncode == 0, r.stderr
    return {name: tmp / name for name in NAMES}


def test_only_the_polished_file_changes(dumps):
    files = {name: _files(d) for name, d in dumps.items()}
    polish, weighted = files["polish"], files["weighted"]
    assert set(polish) == set(weighted) and "cluster_polished.fq" in polish
    assert [f for f in polish if polish[f] != weighted[f]] == ["cluster_polished.fq"]
    assert b"weighted" not in polish["cluster_polished.fq"]
    # beside the other reports: each is that of its option alone, and the polished file the weighted one
    assert files["all"]["cluster_polished.fq"] == weighted["cluster_polished.fq"]
    for f in ("read_stats.tsv", "cluster_pileup.tsv"):
        assert files["all"][f] == files["reports"][f]
    assert set(files["all"]) == set(files["reports"]) | {"cluster_polished.fq"}


def test_the_option_alone_is_refused(tmp_path):
    r = run("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--polish-weighted", "nothing.cer")
    assert r.returncode != 0 and "polish-weighted" in r.stderr


def test_every_record_recomputed_from_the_written_files(dumps):
    d = dumps["weighted"]
    L = _lib.load()
    cons = {}
    for head, seq, qual in _fastq_records(d / "cluster_cons.fq"):
        cons[int(head.split(b" ")[0][8:])] = (seq, qual)
    assert list(cons) == sorted(cons) and len(cons) >= 5
    reads = {cid: (_fastq_records(d / "cluster_fastq" / f"{cid}.fq") if os.path.exists(d / "cluster_fastq" / f"{cid}.fq") else []) for cid in cons}
    lines = [q for _, q in cons.values()] + [q for cid in cons for _, _, q in reads[cid]]
    offs = np.zeros(len(lines) + 1, np.int64)
    offs[1:] = np.cumsum([len(q) for q in lines])
    ctx = api.Context(0)
    _, err = ctx.qual_scores(offs, np.frombuffer(b"".join(lines), np.uint8), K)
    ctx.close()
    err = [float(e) for e in err]
    cons_err, read_err = dict(zip(cons, err)), iter(err[len(cons):])

    want, plain = {1: [], 3: []}, []
    for cid, (ref, _) in cons.items():
        cols, ins = np.zeros(len(ref) + 1, api.PILEUP_DTYPE), np.zeros(len(ref) + 1, api.PILEUP_INS_DTYPE)
        wcols, wins = np.zeros_like(cols), np.zeros_like(ins)
        for _, q, ql in reads[cid]:
            ops, _ = api.host_align_ops(q, ref, gap_open=L.ioc_host_gap_open(next(read_err) + cons_err[cid]))
            api.ops_pileup(ops, q, len(ref), cols=cols)
            api.ops_pileup_ins(ops, q, len(ref), ins=ins)
            api.ops_pileup_weighted(ops, q, ql, len(ref), wcols=wcols, wins=wins)
        for md in (1, 3):
            seq, qual, st = api.pileup_call_weighted(cols, wcols, wins, ref, md)
            head = b"cluster_%d reads=%d subs=%d dels=%d ins=%d low=%d weighted=1" % (cid, len(reads[cid]), st["n_sub"], st["n_del"], st["n_ins"], st["n_low"])
            want[md].append((head, seq, qual))
        plain.append(api.pileup_call(cols, ins, ref, 3)[0])
    assert _fastq_records(d / "cluster_polished.fq") == want[3]
    assert _fastq_records(dumps["depth1"] / "cluster_polished.fq") == want[1]
    assert [seq for _, seq, _ in _fastq_records(dumps["polish"] / "cluster_polished.fq")] == plain
    # the fixture condition: the weighting matters for at least one record, and not for all of them
    differ = [cid for cid, (_, seq, _), p in zip(cons, want[3], plain) if seq != p]
    assert differ and len(differ) < len(cons), differ
    # ... and it matters where it provably must: the cluster of the closed-form reads is called as T by weight, as the three
    # doubtful reads have it by count
    T, edited, _, _ = pw.closed_form(400, seed=400)
    mine = [x for x, cid in enumerate(cons) if any(h.startswith(b"w") for h, _, _ in reads[cid])]
    assert len(mine) == 1 and len(reads[list(cons)[mine[0]]]) == 5
    assert {want[3][mine[0]][1], plain[mine[0]]} in ({T, edited}, {revcomp(T), revcomp(edited)}) and want[3][mine[0]][1] in (T, revcomp(T))
