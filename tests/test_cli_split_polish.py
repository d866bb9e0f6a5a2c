"""`dump --split --split-polish`: cluster_split_polished.fq (ioc_align_pairs_split_polish on the GPU).  The option is parsed and
refused without a GPU.  On the read set of test_cli_split.py — the two-haplotype case of tests/sites_common.py among ordinary
transcripts — the file is recomputed from the files `dump` wrote alone through Context.align_pairs_split_polish: one record per
group that has reads of every cluster that has a split, in cluster order; the haplotypes' cluster comes back as its two
haplotypes; and the other report files do not change by one byte when the option stands beside them."""
import os

import numpy as np
import pytest

from isonclust2_amd import api, synth
from tests import sites_common as sc
from tests.test_cli import run
from tests.test_cli_read_stats import K, _fastq_records, _files

NAMES = {"split": ["--split"], "sp": ["--split", "--split-polish"], "all": ["--split", "--sites", "--read-stats", "--pileup"],
         "sp_all": ["--split", "--split-polish", "--sites", "--read-stats", "--pileup"],
         "sp_depth": ["--split", "--split-polish", "--split-polish-min-depth", "6"]}
DEPTH = {"sp": 3, "sp_depth": 6}


def test_the_flag_without_split_dies_with_its_message(tmp_path):
    r = run("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--split-polish", "nothing.cer")
    assert r.returncode == 1 and "--split-polish asks for --split" in r.stderr
    r = run("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--split", "--split-polish", "--split-polish-min-depth", "0", "nothing.cer")
    assert r.returncode == 1 and "--split-polish-min-depth" in r.stderr and "must be" in r.stderr
    r = run("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--split", "--split-polish", "--split-polish-min-depth", "4", "nothing.cer")
    assert r.returncode == 1 and "--split-polish" not in r.stderr and "must be" not in r.stderr   # (as far as the batch)
    h = run("dump", "--help")
    assert h.returncode == 0 and all(w in h.stderr for w in ("--split-polish ", "--split-polish-min-depth", "cluster_split_polished.fq"))


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """3 transcripts x 10 reads of ~400 bases and the 6 + 5 reads of the two haplotypes: sort, cluster (fast mode), the dumps."""
    tmp = tmp_path_factory.mktemp("split_polish")
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
    new = {"cluster_split_polished.fq"}
    assert set(files["sp"]) == set(files["split"]) | new and set(files["sp_all"]) == set(files["all"]) | new
    for f in files["split"]:
        assert files["sp"][f] == files["split"][f] == files["sp_depth"][f], f
    for f in files["all"]:
        assert files["sp_all"][f] == files["all"][f], f
    assert files["sp_all"]["cluster_split_polished.fq"] == files["sp"]["cluster_split_polished.fq"]


@pytest.mark.gpu
def test_the_records_are_the_library_calls(dumps):
    d = dumps["sp"]
    cons = {int(head.split(b" ")[0][8:]): (seq, qual) for head, seq, qual in _fastq_records(d / "cluster_cons.fq")}
    reads = {cid: (_fastq_records(d / "cluster_fastq" / f"{cid}.fq") if os.path.exists(d / "cluster_fastq" / f"{cid}.fq") else []) for cid in cons}
    lines = [q for _, q in cons.values()] + [q for cid in cons for _, _, q in reads[cid]]
    offs = np.zeros(len(lines) + 1, np.int64)
    offs[1:] = np.cumsum([len(q) for q in lines])
    ctx = api.Context(0)
    _, err = ctx.qual_scores(offs, np.frombuffer(b"".join(lines), np.uint8), K)
    err = [float(e) for e in err]
    cons_err, read_err = dict(zip(cons, err)), iter(err[len(cons):])
    seqs, pairs, sop, segs, seg_cid = [], [], [], [], []
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
    ctx.align_set_pool(seqs)
    hap = next(cid for cid in cons if any(h.startswith(b"h") for h, _, _ in reads[cid]))
    T, B, _ = sc.haplotypes()
    for name, depth in DEPTH.items():
        got = ctx.align_pairs_split_polish(pairs, K, segs, sop, polish_min_depth=depth)
        want = []
        for cid in cons:   # (cluster order)
            if cid not in seg_cid:
                continue
            g = seg_cid.index(cid)
            z = got["seg"][g]
            if int(z["seed"]) < 0:
                continue
            for h, n in ((0, int(z["n_group0"])), (1, int(z["n_group1"]))):
                if n > 0:
                    st = got["gpolish"][g, h]
                    head = f"cluster_{cid}/{h} reads={n} subs={int(st['n_sub'])} dels={int(st['n_del'])} ins={int(st['n_ins'])} low={int(st['n_low'])}"
                    want.append((head.encode(), got["gseq"][g][h], got["gqual"][g][h]))
        assert _fastq_records(dumps[name] / "cluster_split_polished.fq") == want, name
        # the haplotypes' cluster: two records, of 6 and of 5 reads, and nothing else in the file
        assert [w[0].split(b" ")[:2] for w in want] == [[b"cluster_%d/0" % hap, b"reads=6"], [b"cluster_%d/1" % hap, b"reads=5"]]
        if name == "sp":
            # ... each called as its haplotype (in the representative's frame, whichever strand that is), unanimously
            rc = lambda s: bytes(reversed(s.translate(bytes.maketrans(b"ACGT", b"TGCA"))))
            assert {want[0][1], want[1][1]} in ({T, B}, {rc(T), rc(B)})
            assert all(set(w[2]) == {ord("I")} for w in want)
        else:
            # under a depth of 6 the group of five reads keeps the representative, quality '!'
            assert want[1][1] == cons[hap][0] and set(want[1][2]) == {ord("!")} and set(want[0][2]) == {ord("I")}
    ctx.close()
