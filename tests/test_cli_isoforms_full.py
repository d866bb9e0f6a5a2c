"""`dump --isoforms --isoforms-inserts --isoforms-inserts-seq --isoforms-full`: cluster_isoforms_full.fq
(ioc_align_pairs_isoforms_full on the GPU).  The options are parsed, refused and in the help without a GPU.  The read set is that of
test_cli_isoforms_inserts_seq.py: the planted cluster's representative lacks [150, 190), so the cluster has one block and one site and
more isoforms over both than over the block alone — a record each, whose sequence must be nearer its own transcript than any other isoform's, the carriers' by
at least 20 bases nearer than the same record with the representative's rows in the window's place.  Every other report file does
not change by one byte when the option stands beside them."""
import os
import re

import pytest

from isonclust2_amd import synth
from tests import blocks_common as bc
from tests import iso_polish_common as ipc
from tests.test_cli import run
from tests.test_cli_read_stats import _fastq_records, _files
from tests.test_cli_isoforms_inserts_seq import REPRESENTATIVE

SEQ = ["--isoforms", "--isoforms-inserts", "--isoforms-inserts-seq"]
NAMES = {"seq": SEQ, "full": SEQ + ["--isoforms-full"], "full_2": SEQ + ["--isoforms-full", "--isoforms-full-max", "2"]}
# (blocks signature, sites signature) -> the true isoform of blocks_common.property_case: '=' keeps the block [400, 520) / lacks the
# exon [150, 190), '-' skips the block, '+' carries the exon
TRUE_OF_KEY = {(b"=", b"+"): 0, (b"=", b"="): 1, (b"-", b"="): 2, (b"-", b"+"): 3}
MARGIN = 20   # half the exon's 40 bases


def test_the_options_are_parsed_refused_and_in_the_help(tmp_path):
    base = ("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"))
    r = run(*base, *SEQ, "--isoforms-full", "--isoforms-full-max", "3", "nothing.cer")
    assert r.returncode == 1 and "--isoforms" not in r.stderr and "must be" not in r.stderr   # (as far as the batch)
    for bad in ("0", "-1", "all"):
        r = run(*base, *SEQ, "--isoforms-full", "--isoforms-full-max", bad, "nothing.cer")
        assert r.returncode == 1 and "--isoforms-full-max" in r.stderr and "must be" in r.stderr, bad
    for without in (["--isoforms", "--isoforms-inserts"], ["--isoforms"], []):
        r = run(*base, *without, "--isoforms-full", "nothing.cer")
        assert r.returncode == 1 and "--isoforms-full asks for --isoforms-inserts-seq" in r.stderr, without
    r = run(*base, *SEQ, "--isoforms-full", "--isoforms-polish", "nothing.cer")
    assert r.returncode == 1 and "not offered together with --isoforms-polish" in r.stderr   # the refusal stays
    h = run("dump", "--help")
    assert h.returncode == 0 and all(w in h.stderr for w in ("--isoforms-full ", "--isoforms-full-max N", "cluster_isoforms_full.fq", "(default 16)"))


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("isoforms_full")
    fq = tmp / "reads.fq"
    T, reads, _ = bc.property_case(bc.SEED, rate=0.01)
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
    return T, {name: tmp / name for name in NAMES}


@pytest.mark.gpu
def test_the_other_reports_do_not_change(dumps):
    _, dirs = dumps
    files = {name: _files(d) for name, d in dirs.items()}
    for with_ in ("full", "full_2"):
        assert set(files[with_]) == set(files["seq"]) | {"cluster_isoforms_full.fq"}, with_
        for f in files["seq"]:
            assert files[with_][f] == files["seq"][f], (with_, f)


@pytest.mark.gpu
def test_a_record_per_combined_isoform_each_nearest_its_own_transcript(dumps):
    T, dirs = dumps
    every = _fastq_records(dirs["full"] / "cluster_isoforms_full.fq")
    ins = _fastq_records(dirs["full"] / "cluster_inserts.fq")
    cid, lo, hi = (int(x) for x in re.search(rb"cluster_(\d+)/ins0 rows=(\d+)-(\d+)", ins[0][0]).groups())
    # (the fast mode puts some of the planted reads into a cluster of their own, which has blocks and no site: its records carry no splice)
    recs = [r for r in every if r[0].startswith(b"cluster_%d/" % cid)]
    rows = [ln.split("\t") for ln in open(dirs["full"] / "read_inserts.tsv").read().split("\n")[1:] if ln]
    n_iso = 1 + max(int(r[3]) for r in rows if int(r[0]) == cid and r[3] != ".")   # the combined isoforms of the cluster, as read_inserts.tsv has them
    assert len(recs) == n_iso >= 3 and len(ins) == 1, [r[0] for r in every]
    assert all(re.search(rb" key=[=\-~.]+/\* ", r[0]) and b"@" not in r[0] for r in every if r not in recs), [r[0] for r in every]
    cons = {int(h.split(b" ")[0][8:]): s for h, s, _ in _fastq_records(dirs["full"] / "cluster_cons.fq")}
    iso = ipc.true_isoforms(T)
    seen = []
    for h, (head, seq, qual) in enumerate(recs):
        m = re.fullmatch(rb"cluster_(\d+)/iso(\d) key=([=\-~.]+)/([=+?.]+) reads=(\d+) subs=\d+ dels=\d+ ins=\d+ low=\d+((?: ins\d+@\d+\+\d+)*)", head)
        assert m and int(m.group(2)) == h and len(seq) == len(qual) and int(m.group(5)) >= 3, head
        own = TRUE_OF_KEY[(m.group(3), m.group(4))]
        dist = [ipc.edit_distance(seq, t) for t in iso]
        print(head, dist)
        assert dist[own] < min(d for x, d in enumerate(dist) if x != own), (head, dist)
        seen.append(own)
        spliced = re.findall(rb" ins(\d+)@(\d+)\+(\d+)", m.group(6))
        assert (len(spliced) == 1) == (m.group(4) == b"+"), head
        if spliced:   # a carrier: the window stands where the record says, and without it the record is at least 20 bases further
            b, at, ln = (int(x) for x in spliced[0])
            assert b == 0 and seq[at:at + ln] == ins[0][1]
            without = seq[:at] + cons[int(m.group(1))][lo:hi] + seq[at + ln:]
            d_without = ipc.edit_distance(without, iso[own])
            print("   without the splice", d_without)
            assert d_without - dist[own] >= MARGIN
    assert len(set(seen)) == n_iso and {0, 3} & set(seen) and {1, 2} & set(seen)   # each another transcript; carriers and others
    # --isoforms-full-max 2: the first two isoforms of every cluster
    assert _fastq_records(dirs["full_2"] / "cluster_isoforms_full.fq") == [r for r in every if re.match(rb"cluster_\d+/iso[01] ", r[0])]
