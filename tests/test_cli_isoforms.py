"""`dump --isoforms`: cluster_blocks.tsv, cluster_isoforms.tsv and read_isoforms.tsv (ioc_align_pairs_blocks on the GPU).  The
options are parsed and refused without a GPU.  The read set: ordinary synthetic transcripts and the four isoforms of
blocks_common.property_case — 12 + 10 + 10 + 6 reads of one 1000-base transcript without [150, 190), [400, 520), both or neither,
and three truncated reads — at 1 % errors and qualities that say so (at 3 % under uniform qualities the fast mode leaves most of them
alone), the first full-length read at the highest quality so that it represents its cluster.
The three files are recomputed through Context.align_pairs_blocks from the files `dump` wrote alone.  The other report files do not
change by one byte when the option stands beside them."""
import os

import numpy as np
import pytest

from isonclust2_amd import api, synth
from tests import blocks_common as bc
from tests.test_cli import run
from tests.test_cli_read_stats import K, _fastq_records, _files

NAMES = {"plain": [], "isoforms": ["--isoforms"], "all": ["--sites", "--read-stats", "--pileup", "--polish", "--correct"],
         "isoforms_all": ["--isoforms", "--sites", "--read-stats", "--pileup", "--polish", "--correct"],
         "stats": ["--read-stats", "--pileup"], "isoforms_stats": ["--isoforms", "--read-stats", "--pileup"],
         "isoforms_rule": ["--isoforms", "--isoforms-min-gap", "30", "--isoforms-min-depth", "2", "--isoforms-min-alt", "2", "--isoforms-min-pct", "10",
                           "--isoforms-min-block", "50", "--isoforms-max", "1"]}
RULES = {"isoforms": {}, "isoforms_rule": dict(min_gap=30, min_depth=2, min_alt=2, min_pct=10, min_block=50, max_blocks=1)}
NEW = {"cluster_blocks.tsv", "cluster_isoforms.tsv", "read_isoforms.tsv"}


def test_the_options_are_parsed_and_in_the_help(tmp_path):
    base = ("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--isoforms")
    for flag, bad in (("--isoforms-min-gap", "0"), ("--isoforms-min-depth", "0"), ("--isoforms-min-alt", "0"), ("--isoforms-min-pct", "0"),
                      ("--isoforms-min-pct", "51"), ("--isoforms-min-block", "0"), ("--isoforms-max", "0"), ("--isoforms-max", "33"), ("--isoforms-max", "all")):
        r = run(*base, flag, bad, "nothing.cer")
        assert r.returncode == 1 and flag in r.stderr and "must be" in r.stderr, (flag, bad)
    r = run(*base, "--isoforms-min-gap", "25", "--isoforms-min-depth", "4", "--isoforms-min-alt", "2", "--isoforms-min-pct", "50", "--isoforms-min-block", "5",
            "--isoforms-max", "32", "nothing.cer")
    assert r.returncode == 1 and "--isoforms" not in r.stderr and "must be" not in r.stderr   # (as far as the batch)
    h = run("dump", "--help")
    assert h.returncode == 0 and all(w in h.stderr for w in ("--isoforms ", "--isoforms-min-gap", "--isoforms-min-depth", "--isoforms-min-alt", "--isoforms-min-pct",
                                                             "--isoforms-min-block", "--isoforms-max", "cluster_blocks.tsv", "cluster_isoforms.tsv",
                                                             "read_isoforms.tsv", "default 20", "default 10"))
    assert " ".join(h.stderr.split()).count("not measured on real data") >= 3   # (the defaults of min-gap and min-block are choices, and say so)


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("isoforms")
    fq = tmp / "reads.fq"
    _, reads, _ = bc.property_case(bc.SEED, rate=0.01)
    with open(fq, "wb") as f:
        rs = synth.generate(30, 3, 400, 12, 21, seed=5)
        for i in range(rs.n):
            s, q = rs.read(i)
            f.write(b"@r%d extra words\n" % i + s + b"\n+\n" + q + b"\n")
        for i, s in enumerate(reads):
            f.write(b"@t%d\n" % i + s + b"\n+\n" + bytes([33 + (28 if i == 0 else 20 + i % 3)]) * len(s) + b"\n")
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
    for with_, without in (("isoforms", "plain"), ("isoforms_all", "all"), ("isoforms_stats", "stats"), ("isoforms_rule", "plain")):
        assert set(files[with_]) == set(files[without]) | NEW, with_
        for f in files[without]:
            assert files[with_][f] == files[without][f], (with_, f)
    for f in NEW:
        assert files["isoforms_all"][f] == files["isoforms"][f] == files["isoforms_stats"][f], f
    assert files["isoforms_rule"]["cluster_blocks.tsv"] != files["isoforms"]["cluster_blocks.tsv"]


@pytest.mark.gpu
def test_the_three_files_are_the_library_call(dumps):
    d = dumps["isoforms"]
    cons = {int(head.split(b" ")[0][8:]): (seq, qual) for head, seq, qual in _fastq_records(d / "cluster_cons.fq")}
    reads = {cid: (_fastq_records(d / "cluster_fastq" / f"{cid}.fq") if os.path.exists(d / "cluster_fastq" / f"{cid}.fq") else []) for cid in cons}
    lines = [q for _, q in cons.values()] + [q for cid in cons for _, _, q in reads[cid]]
    offs = np.zeros(len(lines) + 1, np.int64)
    offs[1:] = np.cumsum([len(q) for q in lines])
    ctx = api.Context(0)
    _, err = ctx.qual_scores(offs, np.frombuffer(b"".join(lines), np.uint8), K)
    err = [float(e) for e in err]
    cons_err, read_err = dict(zip(cons, err)), iter(err[len(cons):])
    seqs, pairs, sop, segs, seg_cls, pair_of = [], [], [], [], [], {}
    for cid, (ref, _) in cons.items():
        if not reads[cid]:
            continue
        seqs.append(ref)
        segs.append((len(seqs) - 1, 0))
        seg_cls.append(cid)
        for head, s, q in reads[cid]:
            seqs.append(s)
            pair_of[head] = len(pairs)
            pairs.append((len(seqs) - 1, segs[-1][0], 0, next(read_err) + cons_err[cid]))
            sop.append(len(segs) - 1)
    ctx.align_set_pool(seqs)
    rows = [ln.split(b"\t") for ln in open(d / "clusters.tsv", "rb").read().split(b"\n")[1:] if ln]
    rows = [(int(c), rid) for c, _, rid in rows if int(c) in cons]
    assert len(rows) == len(pairs) >= 60
    text = lambda path: open(path).read().split("\n")
    how = ("direct", "assigned", "rare", "ambiguous")
    for name, rule in RULES.items():
        got = ctx.align_pairs_blocks(pairs, K, segs, sop, rows=False, **rule)
        blocks, iso = ["ClusterId\tBlock\tFirst\tEnd\tKeep\tSkip\tPart\tNone"], ["ClusterId\tIsoform\tSignature\tDirect\tAssigned"]
        for g, cid in sorted(enumerate(seg_cls), key=lambda t: t[1]):   # (cluster order)
            z, mine = got["seg"][g], got["reads"][[x for x, s in enumerate(sop) if s == g]]
            if int(z["n_found"]) > int(z["n_blocks"]):
                blocks.append(f"# cluster {cid}: kept {int(z['n_blocks'])} of {int(z['n_found'])} blocks")
            for b, k in enumerate(got["blocks"][g]):
                blocks.append("\t".join(str(v) for v in (cid, b, int(k["first"]), int(k["end"]), int(k["n_keep"]), int(k["n_skip"]), int(k["n_part"]), int(k["n_none"]))))
            for x in range(int(z["n_groups"])):
                direct = mine[(mine["group"] == x) & (mine["how"] == api.ISO_DIRECT)]
                assigned = mine[(mine["group"] == x) & (mine["how"] == api.ISO_ASSIGNED)]
                iso.append("\t".join(str(v) for v in (cid, x, bc.signature(direct["key"][0], int(z["n_blocks"])), len(direct), len(assigned))))
        assert text(dumps[name] / "cluster_blocks.tsv") == blocks + [""], name
        assert text(dumps[name] / "cluster_isoforms.tsv") == iso + [""], name
        per_read = ["ClusterId\tRead\tIsoform\tHow\tSignature\tFirst\tEnd\tGaps\tGapRows"]
        for cid, rid in rows:   # (the order of clusters.tsv)
            x = pair_of[rid]
            r, nb = got["reads"][x], int(got["seg"][sop[x]]["n_blocks"])
            per_read.append("\t".join(str(v) for v in (cid, rid.decode(), "." if r["group"] < 0 else int(r["group"]), how[int(r["how"])], bc.signature(r["key"], nb),
                                                        int(r["first_row"]), int(r["end_row"]), int(r["n_gaps"]), int(r["gap_rows"]))))
        assert text(dumps[name] / "read_isoforms.tsv") == per_read + [""], name
        if name == "isoforms":   # the planted transcript: a cluster with two blocks and four isoforms, whatever else there is
            assert any(int(z["n_blocks"]) == 2 and int(z["n_groups"]) == 4 for z in got["seg"]), got["seg"]
            assert len(blocks) >= 3 and len(iso) >= 5
        else:
            assert int(got["seg"]["n_blocks"].max()) == 1
    ctx.close()
