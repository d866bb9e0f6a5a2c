"""`dump --correct`: corrected_reads.fq (ioc_align_pairs_correct on the GPU).  The options are parsed and refused without a GPU.
The read set is that of test_cli_split_polish.py — the two-haplotype case of tests/sites_common.py among ordinary transcripts —
with two more reads of the first haplotype: one carries an insertion of 9 bases, one stands between 15 foreign bases at either
end.  The file is recomputed through Context.align_pairs_correct from the files `dump` wrote alone: one record per row of
clusters.tsv, in its order, with the ends the alignment leaves free attached as they are.  The read with the long insertion comes
back as it is, marked.  The other report files do not change by one byte when the option stands beside them."""
import os

import numpy as np
import pytest

from isonclust2_amd import api, synth
from tests import sites_common as sc
from tests.test_cli import run
from tests.test_cli_read_stats import K, _fastq_records, _files

NAMES = {"plain": [], "correct": ["--correct"], "all": ["--split", "--split-polish", "--sites", "--read-stats", "--pileup", "--polish"],
         "correct_all": ["--correct", "--split", "--split-polish", "--sites", "--read-stats", "--pileup", "--polish"],
         "stats": ["--read-stats", "--pileup"], "correct_stats": ["--correct", "--read-stats", "--pileup"],
         "correct_rule": ["--correct", "--correct-min-depth", "2", "--correct-min-alt", "2", "--correct-min-pct", "40", "--correct-max-run", "2"]}
RULES = {"correct": dict(min_depth=3, min_alt=3, min_pct=25, max_run=10), "correct_rule": dict(min_depth=2, min_alt=2, min_pct=40, max_run=2)}
INSERTED = b"GATTACAGA"
ENDS = (b"CCCCCCCCCCCCCCC", b"GGGGGGGGGGGGGGG")


def test_the_options_are_parsed_and_in_the_help(tmp_path):
    base = ("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--correct")
    for flag, bad in (("--correct-min-depth", "0"), ("--correct-min-alt", "0"), ("--correct-min-pct", "0"), ("--correct-min-pct", "51"),
                      ("--correct-max-run", "-1"), ("--correct-max-run", "65"), ("--correct-max-run", "ten")):
        r = run(*base, flag, bad, "nothing.cer")
        assert r.returncode == 1 and flag in r.stderr and "must be" in r.stderr, (flag, bad)
    r = run(*base, "--correct-min-depth", "4", "--correct-min-alt", "2", "--correct-min-pct", "50", "--correct-max-run", "0", "nothing.cer")
    assert r.returncode == 1 and "--correct" not in r.stderr and "must be" not in r.stderr   # (as far as the batch)
    h = run("dump", "--help")
    assert h.returncode == 0 and all(w in h.stderr for w in ("--correct ", "--correct-min-depth", "--correct-min-alt", "--correct-min-pct",
                                                             "--correct-max-run", "corrected_reads.fq", "default 10"))
    assert "not measured on real data" in " ".join(h.stderr.split())   # (the default of --correct-max-run is a choice, and says so)


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """3 transcripts x 10 reads of ~400 bases, the 6 + 5 reads of the two haplotypes, a read of T with 9 bases inserted in front
    of T[250] (h11) and a read of T between 15 foreign bases at either end (h12): sort, cluster (fast mode), the dumps."""
    tmp = tmp_path_factory.mktemp("correct")
    fq = tmp / "reads.fq"
    T, B, reads = sc.haplotypes()
    with open(fq, "wb") as f:
        rs = synth.generate(30, 3, 400, 12, 21, seed=5)
        for i in range(rs.n):
            s, q = rs.read(i)
            f.write(b"@r%d extra words\n" % i + s + b"\n+\n" + q + b"\n")
        for i, s in enumerate(reads + [T[:250] + INSERTED + T[250:], ENDS[0] + T + ENDS[1]]):
            # (the planted reads at a lower quality than any other: neither becomes its cluster's representative)
            f.write(b"@h%d\n" % i + s + b"\n+\n" + bytes([33 + (30 + i % 3 if i < len(reads) else 20)]) * len(s) + b"\n")
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
    new = {"corrected_reads.fq"}
    for with_, without in (("correct", "plain"), ("correct_all", "all"), ("correct_stats", "stats"), ("correct_rule", "plain")):
        assert set(files[with_]) == set(files[without]) | new, with_
        for f in files[without]:
            assert files[with_][f] == files[without][f], (with_, f)
    assert files["correct_all"]["corrected_reads.fq"] == files["correct"]["corrected_reads.fq"] == files["correct_stats"]["corrected_reads.fq"]
    assert files["correct_rule"]["corrected_reads.fq"] != files["correct"]["corrected_reads.fq"]


@pytest.mark.gpu
def test_the_records_are_the_library_call(dumps):
    d = dumps["correct"]
    cons = {int(head.split(b" ")[0][8:]): (seq, qual) for head, seq, qual in _fastq_records(d / "cluster_cons.fq")}
    reads = {cid: (_fastq_records(d / "cluster_fastq" / f"{cid}.fq") if os.path.exists(d / "cluster_fastq" / f"{cid}.fq") else []) for cid in cons}
    lines = [q for _, q in cons.values()] + [q for cid in cons for _, _, q in reads[cid]]
    offs = np.zeros(len(lines) + 1, np.int64)
    offs[1:] = np.cumsum([len(q) for q in lines])
    ctx = api.Context(0)
    _, err = ctx.qual_scores(offs, np.frombuffer(b"".join(lines), np.uint8), K)
    err = [float(e) for e in err]
    cons_err, read_err = dict(zip(cons, err)), iter(err[len(cons):])
    seqs, pairs, sop, segs, pair_of = [], [], [], [], {}
    for cid, (ref, _) in cons.items():
        if not reads[cid]:
            continue
        seqs.append(ref)
        segs.append((len(seqs) - 1, 0))
        for head, s, q in reads[cid]:
            seqs.append(s)
            pair_of[head] = (len(pairs), cid, s, q)
            pairs.append((len(seqs) - 1, segs[-1][0], 0, next(read_err) + cons_err[cid]))
            sop.append(len(segs) - 1)
    ctx.align_set_pool(seqs)
    rows = [ln.split(b"\t") for ln in open(d / "clusters.tsv", "rb").read().split(b"\n")[1:] if ln]
    rows = [(int(c), rid) for c, _, rid in rows if int(c) in cons]
    assert len(rows) == len(pairs) >= 40
    rc = lambda s: bytes(reversed(s.translate(bytes.maketrans(b"ACGT", b"TGCA"))))
    for name, rule in RULES.items():
        got = ctx.align_pairs_correct(pairs, K, segs, sop, stats=True, **rule)
        want, clipped, marked = [], {}, []
        for cid, rid in rows:   # (the order of clusters.tsv)
            x, cid_x, s, q = pair_of[rid]
            a, z = got["stats"][x], got["correct"][x]
            assert cid_x == cid
            if int(a["longest_ins"]) > 6:
                head = b"%s cluster=%d subs=0 fills=0 removes=0 ins_add=0 ins_drop=0 low=0 guarded=0 uncorrected=long_insertion" % (rid, cid)
                want.append((head, s, q))
                marked.append(rid)
                continue
            lead, trail = int(a["lead_i"]), int(a["trail_i"])
            clipped[rid] = lead + trail
            head = b"%s cluster=%d subs=%d fills=%d removes=%d ins_add=%d ins_drop=%d low=%d guarded=%d" % (
                rid, cid, *(int(z[f]) for f in ("n_sub", "n_fill", "n_remove", "n_ins_add", "n_ins_drop", "n_low", "n_guarded")))
            want.append((head, s[:lead] + got["seq"][x] + s[len(s) - trail:], q[:lead] + got["qual"][x] + q[len(q) - trail:]))
        assert _fastq_records(dumps[name] / "corrected_reads.fq") == want, name
        # the planted reads: the one as it is (in its cluster's frame, whichever strand that is), the other with its ends attached
        assert marked == [b"h11"] and (INSERTED in pair_of[b"h11"][2] or rc(INSERTED) in pair_of[b"h11"][2]), marked
        assert clipped[b"h12"] >= 20, clipped[b"h12"]
        ends = [w for w in want if w[0].startswith(b"h12 ")][0][1]
        assert (ends[:10], ends[-10:]) in ((ENDS[0][:10], ENDS[1][-10:]), (rc(ENDS[1])[:10], rc(ENDS[0])[-10:]))
    ctx.close()
