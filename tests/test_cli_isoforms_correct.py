"""`dump --isoforms --isoforms-correct`: corrected_reads_isoforms.fq (ioc_align_pairs_blocks_correct on the GPU).  The option is parsed
and refused without a GPU.  The read set: ordinary synthetic transcripts and the planted isoforms of
iso_correct_common.planted_isoforms — a representative, a minority isoform that skips 20 rows of it, three carriers of an exon of 40
bases it lacks, at 1 % errors and below.  The file is recomputed through Context.align_pairs_blocks_correct from the files `dump`
wrote alone: one record per row of clusters.tsv, in its order, corrected_reads.fq's layout with isoform=, table=, long_runs= and
long_bases= in the header.  The other report files do not change by one byte when the option stands beside them, and --correct
stays what it is."""
import os

import numpy as np
import pytest

from isonclust2_amd import api, synth
from tests import iso_correct_common as ic
from tests.test_cli import run
from tests.test_cli_read_stats import K, _fastq_records, _files

ISO = ["--isoforms", "--isoforms-min-gap", "10", "--isoforms-min-block", "10", "--isoforms-min-pct", "15"]
RUN = ["--correct-max-run", "24"]
NAMES = {"isoforms": ISO + RUN, "correct": ISO + RUN + ["--isoforms-correct"],
         "isoforms_all": ISO + RUN + ["--correct", "--read-stats", "--pileup", "--polish"],
         "correct_all": ISO + RUN + ["--isoforms-correct", "--correct", "--read-stats", "--pileup", "--polish"],
         "correct_rule": ISO + ["--isoforms-correct", "--correct-min-depth", "5", "--correct-max-run", "2"]}
RULES = {"correct": dict(correct_min_depth=3, correct_min_alt=3, correct_min_pct=25, correct_max_run=24),
         "correct_rule": dict(correct_min_depth=5, correct_min_alt=3, correct_min_pct=25, correct_max_run=2)}
BLOCKS = dict(min_gap=10, min_block=10, min_pct=15)
NEW = {"corrected_reads_isoforms.fq"}


def test_the_option_is_parsed_refused_and_in_the_help(tmp_path):
    base = ("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"))
    r = run(*base, "--isoforms-correct", "nothing.cer")
    assert r.returncode == 1 and "--isoforms-correct asks for --isoforms" in r.stderr
    for other, extra in (("--isoforms-inserts", []), ("--isoforms-ends", []), ("--isoforms-polish", [])):
        r = run(*base, "--isoforms", "--isoforms-correct", other, *extra, "nothing.cer")
        assert r.returncode == 1 and f"--isoforms-correct is not offered together with {other}" in r.stderr and "one fused call a run" in r.stderr, other
    r = run(*base, "--isoforms", "--isoforms-correct", "--correct-max-run", "65", "nothing.cer")
    assert r.returncode == 1 and "--correct-max-run" in r.stderr and "must be" in r.stderr
    r = run(*base, "--isoforms", "--isoforms-correct", "--correct-min-depth", "4", "--correct-max-run", "30", "nothing.cer")
    assert r.returncode == 1 and "--isoforms" not in r.stderr and "must be" not in r.stderr   # (as far as the batch)
    h = run("dump", "--help")
    words = " ".join(h.stderr.split())
    assert h.returncode == 0 and all(w in words for w in ("--isoforms-correct", "corrected_reads_isoforms.fq", "isoform=<h or ->", "table=<isoform|cluster>",
                                                          "long_runs=", "long_bases=", "uncorrected=unresolved_insertion"))


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("isoforms_correct")
    fq = tmp / "reads.fq"
    _, reads, _ = ic.planted_isoforms(q=(20.0, 25.0))   # (at 1 % errors and below: the clustering keeps the three isoforms together)
    with open(fq, "wb") as f:
        rs = synth.generate(30, 3, 400, 12, 21, seed=5)
        for i in range(rs.n):
            s, q = rs.read(i)
            f.write(b"@r%d extra words\n" % i + s + b"\n+\n" + q + b"\n")
        for i, s in enumerate(reads):   # (the first read of the representative's isoform at the highest quality: it becomes the representative)
            f.write(b"@t%d\n" % i + s + b"\n+\n" + bytes([33 + (30 if i == 0 else 18 + i % 3)]) * len(s) + b"\n")
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
    for with_, without in (("correct", "isoforms"), ("correct_all", "isoforms_all")):
        assert set(files[with_]) == set(files[without]) | NEW, with_
        for f in files[without]:
            assert files[with_][f] == files[without][f], (with_, f)
    assert "corrected_reads.fq" in files["correct_all"] and "corrected_reads.fq" not in files["correct"]
    assert files["correct_all"]["corrected_reads_isoforms.fq"] == files["correct"]["corrected_reads_isoforms.fq"]
    assert files["correct_rule"]["corrected_reads_isoforms.fq"] != files["correct"]["corrected_reads_isoforms.fq"]


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
    for name, rule in RULES.items():
        got = ctx.align_pairs_blocks_correct(pairs, K, segs, sop, stats=True, rows=False, **rule, **BLOCKS)
        want, seen = [], {}
        for cid, rid in rows:   # (the order of clusters.tsv)
            x, cid_x, s, q = pair_of[rid]
            a, z, h = got["stats"][x], got["correct"][x], int(got["reads"][x]["group"])
            assert cid_x == cid
            head = b"%s cluster=%d subs=%d fills=%d removes=%d ins_add=%d ins_drop=%d low=%d guarded=%d isoform=%s table=%s long_runs=%d long_bases=%d" % (
                rid, cid, *(int(z[f]) for f in ("n_sub", "n_fill", "n_remove", "n_ins_add", "n_ins_drop", "n_low", "n_guarded")),
                b"%d" % h if h >= 0 else b"-", b"isoform" if int(z["table"]) >= 0 else b"cluster", int(z["n_long_runs"]), int(z["n_long_bases"]))
            seen[rid] = (h, int(z["table"]), int(z["n_long_bases"]), int(z["n_fill"]))
            if int(z["flags"]) & 1:
                want.append((head + b" uncorrected=unresolved_insertion", s, q))
                continue
            lead, trail = int(a["lead_i"]), int(a["trail_i"])
            want.append((head, s[:lead] + got["seq"][x] + s[len(s) - trail:], q[:lead] + got["qual"][x] + q[len(q) - trail:]))
        assert _fastq_records(dumps[name] / "corrected_reads_isoforms.fq") == want, name
        if name == "correct":   # the planted cluster: the minority has a table of its own and nothing is pasted in; the carriers are of the other isoform
            n_major, n_minor, n_carry = ic.PLANTED_SIZES
            minor = [seen[b"t%d" % i] for i in range(n_major, n_major + n_minor)]
            carry = [seen[b"t%d" % i] for i in range(n_major + n_minor, n_major + n_minor + n_carry)]
            assert len({m[0] for m in minor}) == 1 and minor[0][0] >= 0 and all(m[1] >= 0 and m[3] < 12 for m in minor), minor
            assert all(c[0] >= 0 and c[0] != minor[0][0] for c in carry), carry
    ctx.close()
