"""`dump --isoforms --isoforms-inserts --isoforms-inserts-seq`: cluster_inserts.fq (ioc_align_pairs_blocks_inserts_seq on the GPU).
The options are parsed and refused without a GPU.  The read set is that of test_cli_isoforms_inserts.py: the read that represents the
planted cluster lacks [150, 190), so the first exon is an insertion site — and cluster_inserts.fq must hold one record, whose
sequence is the carriers' stretch between the two anchor rows, exon included.  Every other report file does not change by one byte
when the option stands beside them."""
import os
import re

import pytest

from isonclust2_amd import synth
from tests import blocks_common as bc
from tests import iso_polish_common as ipc
from tests.test_cli import run
from tests.test_cli_read_stats import _fastq_records, _files

NAMES = {"inserts": ["--isoforms", "--isoforms-inserts"], "seq": ["--isoforms", "--isoforms-inserts", "--isoforms-inserts-seq"],
         "seq_short": ["--isoforms", "--isoforms-inserts", "--isoforms-inserts-seq", "--isoforms-inserts-max-win", "30"]}
REPRESENTATIVE = bc.SIZES[0]   # the first read of the isoform without [150, 190)
EXON = bc.CUTS[0]


def test_the_options_are_parsed_and_in_the_help(tmp_path):
    base = ("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--isoforms", "--isoforms-inserts", "--isoforms-inserts-seq")
    for bad in ("0", "513", "all"):
        r = run(*base, "--isoforms-inserts-max-win", bad, "nothing.cer")
        assert r.returncode == 1 and "--isoforms-inserts-max-win" in r.stderr and "must be" in r.stderr, bad
    r = run(*base, "--isoforms-inserts-max-win", "512", "nothing.cer")
    assert r.returncode == 1 and "--isoforms" not in r.stderr and "must be" not in r.stderr   # (as far as the batch)
    r = run("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--isoforms", "--isoforms-inserts-seq", "nothing.cer")
    assert r.returncode == 1 and "--isoforms-inserts-seq asks for --isoforms-inserts" in r.stderr
    r = run(*base, "--isoforms-polish", "nothing.cer")
    assert r.returncode == 1 and "not offered together with --isoforms-polish" in r.stderr   # the refusal stays
    h = run("dump", "--help")
    assert h.returncode == 0 and all(w in h.stderr for w in ("--isoforms-inserts-seq", "--isoforms-inserts-max-win", "cluster_inserts.fq", "(default 512)"))


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("isoforms_inserts_seq")
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
    for with_ in ("seq", "seq_short"):
        assert set(files[with_]) == set(files["inserts"]) | {"cluster_inserts.fq"}, with_
        for f in files["inserts"]:
            assert files[with_][f] == files["inserts"][f], (with_, f)


@pytest.mark.gpu
def test_one_record_that_holds_the_exon(dumps):
    T, dirs = dumps
    recs = _fastq_records(dirs["seq"] / "cluster_inserts.fq")
    assert len(recs) == 1, [r[0] for r in recs]
    head, seq, qual = recs[0]
    m = re.fullmatch(rb"cluster_(\d+)/ins0 rows=(\d+)-(\d+) voters=(\d+) template=(t\d+)", head)
    assert m, head
    cid, lo, hi, voters = (int(m.group(x)) for x in (1, 2, 3, 4))
    site = [ln.split("\t") for ln in open(dirs["seq"] / "cluster_inserts.tsv").read().split("\n")[1:] if ln and not ln.startswith("#")]
    assert len(site) == 1 and int(site[0][0]) == cid and lo == max(int(site[0][1]) - 8, 1) and hi == int(site[0][2]) + 8 and 3 <= voters <= int(site[0][3])
    assert len(qual) == len(seq) and lo < EXON[0] < hi
    cons = {int(h.split(b" ")[0][8:]): s for h, s, _ in _fastq_records(dirs["seq"] / "cluster_cons.fq")}
    # nearer to the transcript's stretch WITH the exon than to the representative's own rows, by at least half the exon's length
    # (the representative is a read at 1 % errors: its rows may stand a base or two beside the transcript's)
    with_exon, without = T[lo:hi + EXON[1] - EXON[0]], cons[cid][lo:hi]
    d_with, d_without = ipc.edit_distance(seq, with_exon), ipc.edit_distance(seq, without)
    print(head, "to the window with the exon", d_with, "to the representative's rows", d_without)
    assert d_without - d_with >= (EXON[1] - EXON[0]) // 2
    # a window of 17 rows and 40 inserted bases is longer than 30: nobody votes, no record
    assert _fastq_records(dirs["seq_short"] / "cluster_inserts.fq") == []
