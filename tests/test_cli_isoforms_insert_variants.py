"""`dump --isoforms --isoforms-inserts --isoforms-inserts-seq --isoforms-inserts-variants`: cluster_insert_variants.fq and
read_insert_variants.tsv (ioc_align_pairs_blocks_inserts_variants on the GPU).  The options are parsed and refused without a GPU.  The
read set plants one cluster whose representative lacks an exon at row 150 where half of the other reads hold a 60-base exon and half
a different one of 45 bases (1 % errors): the site must split, cluster_insert_variants.fq must hold a record for each exon, each
nearer to its own true stretch than to the other's by at least half the shorter exon, every carrier's variant in
read_insert_variants.tsv must be its planted exon, and the isoforms counted again must tell the two apart where read_inserts.tsv has
one.  Both files are rebuilt line for line on the host path from the files `dump` wrote alone — the host aligner, the host
projections, the block and insert definitions, ioc_host_insert_window_variants and ioc_host_key_isoforms over every dumped cluster —
at the default agreement and at --isoforms-inserts-variants-min-agree 100.  Every other report file does not change by one byte when
the option stands beside them."""
import os
import random
import re

import numpy as np
import pytest

from isonclust2_amd import api, synth
from tests import iso_polish_common as ipc
from tests import polish_common as pc
from tests.test_cli import run
from tests.test_cli_read_stats import K, _fastq_records, _files

SEQ = ["--isoforms", "--isoforms-inserts", "--isoforms-inserts-seq"]
NAMES = {"seq": SEQ, "variants": SEQ + ["--isoforms-inserts-variants"], "strict": SEQ + ["--isoforms-inserts-variants", "--isoforms-inserts-variants-min-agree", "100"]}
AT, EXONS, SIZES = 150, (60, 45), (8, 8, 6)   # the junction; the two exons; the reads that hold the first, the second, neither


def test_the_options_are_parsed_and_in_the_help(tmp_path):
    base = ("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), *SEQ, "--isoforms-inserts-variants")
    for bad in ("0", "101", "all"):
        r = run(*base, "--isoforms-inserts-variants-min-agree", bad, "nothing.cer")
        assert r.returncode == 1 and "--isoforms-inserts-variants-min-agree" in r.stderr and "must be" in r.stderr, bad
    r = run(*base, "--isoforms-inserts-variants-min-agree", "45", "nothing.cer")
    assert r.returncode == 1 and "--isoforms" not in r.stderr and "must be" not in r.stderr   # (as far as the batch)
    r = run("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--isoforms", "--isoforms-inserts", "--isoforms-inserts-variants", "nothing.cer")
    assert r.returncode == 1 and "--isoforms-inserts-variants asks for --isoforms-inserts-seq" in r.stderr
    r = run(*base, "--isoforms-full", "nothing.cer")
    assert r.returncode == 1 and "not offered together with --isoforms-full" in r.stderr
    h = run("dump", "--help")
    assert h.returncode == 0 and all(w in h.stderr for w in ("--isoforms-inserts-variants ", "--isoforms-inserts-variants-min-agree N", "cluster_insert_variants.fq",
                                                            "read_insert_variants.tsv", "(default 45"))


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("isoforms_insert_variants")
    fq = tmp / "reads.fq"
    rng = random.Random(4)
    frame = bytes(rng.choice(b"ACGT") for _ in range(800))
    exons = [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in EXONS]
    iso = [frame[:AT] + exons[0] + frame[AT:], frame[:AT] + exons[1] + frame[AT:], frame]
    planted = {}
    with open(fq, "wb") as f:
        rs = synth.generate(30, 3, 400, 12, 21, seed=5)
        for i in range(rs.n):
            s, q = rs.read(i)
            f.write(b"@r%d extra words\n" % i + s + b"\n+\n" + q + b"\n")
        f.write(b"@t0\n" + frame + b"\n+\n" + bytes([33 + 28]) * len(frame) + b"\n")   # the best read: the cluster's representative, which lacks the exon
        i = 1
        for x, n in enumerate(SIZES):
            for _ in range(n):
                s = pc.mutate(rng, iso[x], 0.01)
                f.write(b"@t%d\n" % i + s + b"\n+\n" + bytes([33 + 16 + i % 2]) * len(s) + b"\n")
                planted["t%d" % i] = x
                i += 1
    out = tmp / "sorted"
    r = run("sort", "-o", str(out), str(fq))
    assert r.returncode == 0, r.stderr
    r = run("cluster", "-l", str(out / "batches" / "isONbatch_0.cer"), "-o", str(tmp / "c.cer"), "-x", "fast", env=dict(os.environ, ISONCLUST2_SERVE="0"))
    assert r.returncode == 0, r.stderr
    for name, extra in NAMES.items():
        r = run("dump", "-i", str(out / "sorted_reads_idx.cer"), "-o", str(tmp / name), *extra, str(tmp / "c.cer"))
        assert r.returncode == 0, r.stderr
    return frame, exons, planted, {name: tmp / name for name in NAMES}


@pytest.mark.gpu
def test_the_other_reports_do_not_change(dumps):
    *_, dirs = dumps
    files = {name: _files(d) for name, d in dirs.items()}
    for with_ in ("variants", "strict"):
        assert set(files[with_]) == set(files["seq"]) | {"cluster_insert_variants.fq", "read_insert_variants.tsv"}, with_
        for f in files["seq"]:
            assert files[with_][f] == files["seq"][f], (with_, f)


@pytest.mark.gpu
def test_a_record_per_exon_and_every_read_with_its_own(dumps):
    frame, exons, planted, dirs = dumps
    recs = _fastq_records(dirs["variants"] / "cluster_insert_variants.fq")
    old = _fastq_records(dirs["variants"] / "cluster_inserts.fq")
    assert len(old) == 1 and len(recs) == 2, [r[0] for r in recs]
    heads = [re.fullmatch(rb"cluster_(\d+)/ins0/([AB]) rows=(\d+)-(\d+) voters=(\d+) template=(t\d+) split=1", r[0]) for r in recs]
    assert all(heads) and [m.group(2) for m in heads] == [b"A", b"B"], [r[0] for r in recs]
    cid, lo, hi = (int(heads[0].group(x)) for x in (1, 3, 4))
    assert lo < AT < hi and sorted(int(m.group(5)) for m in heads) == [SIZES[0], SIZES[1]]
    true = [frame[lo:AT] + e + frame[AT:hi] for e in exons]
    # variant A is the exon of the site's template: each record stands for the exon its template read was given
    of = [planted[m.group(6).decode()] for m in heads]
    assert sorted(of) == [0, 1]
    for (head, seq, qual), x in zip(recs, of):
        own, other = ipc.edit_distance(seq, true[x]), ipc.edit_distance(seq, true[1 - x])
        print(head, "to its own exon's stretch", own, "to the other's", other)
        assert len(seq) == len(qual) and 2 * (other - own) >= min(EXONS)
    # the window stage has one record for the site, which cannot stand for both exons: the second one is in the new file alone
    assert max(ipc.edit_distance(old[0][1], t) for t in true) >= min(EXONS) // 2
    rows = [ln.split("\t") for ln in open(dirs["variants"] / "read_insert_variants.tsv").read().split("\n")[1:] if ln]
    plain = [ln.split("\t") for ln in open(dirs["variants"] / "read_inserts.tsv").read().split("\n")[1:] if ln]
    assert [r[:2] for r in rows] == [r[:2] for r in plain]   # a row per row of read_inserts.tsv, in that order
    letter = {of[0]: "A", of[1]: "B", 2: "."}
    mine = {r[1]: r for r in rows if int(r[0]) == cid}
    assert set(planted) <= set(mine)   # the planted reads are one cluster
    for name, x in planted.items():
        assert mine[name][2] == letter[x] and mine[name][3] == (letter[x] if x < 2 else "="), mine[name]
    iso_of = lambda x: {mine[name][4] for name, y in planted.items() if y == x}
    assert all(len(iso_of(x)) == 1 for x in range(3)) and len(iso_of(0) | iso_of(1) | iso_of(2)) == 3 and all(mine[name][5] == "direct" for name in planted)
    before = {r[1]: r for r in plain if int(r[0]) == cid}
    assert len({before[name][3] for name, x in planted.items() if x < 2}) == 1   # one isoform to the insert stage


def _host_files(d, min_agree):
    """(the lines of cluster_insert_variants.fq, the lines of read_insert_variants.tsv) on the host path, from the dump directory d"""
    cons = {int(head.split(b" ")[0][8:]): (seq, qual) for head, seq, qual in _fastq_records(d / "cluster_cons.fq")}
    reads = {cid: (_fastq_records(d / "cluster_fastq" / f"{cid}.fq") if os.path.exists(d / "cluster_fastq" / f"{cid}.fq") else []) for cid in cons}
    lines = [q for _, q in cons.values()] + [q for cid in cons for _, _, q in reads[cid]]
    offs = np.zeros(len(lines) + 1, np.int64)
    offs[1:] = np.cumsum([len(q) for q in lines])
    ctx = api.Context(0)
    _, err = ctx.qual_scores(offs, np.frombuffer(b"".join(lines), np.uint8), K)   # (what the pairs' gap penalties come from)
    ctx.close()
    err = [float(e) for e in err]
    cons_err, read_err = dict(zip(cons, err)), iter(err[len(cons):])
    how = ("direct", "assigned", "rare", "ambiguous")
    fq, per_read = [], {}
    for cid in sorted(cons):   # (cluster order)
        ref, rds = cons[cid][0], reads[cid]
        if not rds:
            continue
        base, ilen, qpos = [], [], []
        for _, rd, _ in rds:
            ops, _ = api.host_align_ops(rd, ref, gap_open=pc.gap_open(next(read_err) + cons_err[cid]))
            base.append(api.ops_project(ops, rd, len(ref))[0]), ilen.append(api.ops_project_ilen(ops, len(ref))), qpos.append(api.ops_project_qpos(ops, len(ref)))
        base, ilen, qpos = np.array(base, np.uint8), np.array(ilen, np.uint8), np.array(qpos, np.uint32)
        blocks = api.planes_blocks(base)
        nb = len(blocks["blocks"])
        pk = blocks["reads"]["key"].copy()
        pm = np.array([sum(3 << (2 * b) for b in range(nb) if (int(k) >> (2 * b)) & 3 != api.BLOCK_NONE) for k in pk], np.uint64)
        pre = dict(pre_key=pk, pre_mask=pm, pre_full=(1 << (2 * nb)) - 1)
        ins = api.planes_inserts(base, ilen, **pre)
        S = len(ins["sites"])
        v = api.insert_window_variants(base, qpos, [len(rd) for _, rd, _ in rds], ins["sites"], ins["reads"]["key"], [rd for _, rd, _ in rds], min_agree=min_agree)
        grp, hw, _ = api.key_isoforms(v["key2"], v["mask2"], (1 << (2 * S)) - 1, api.INSERTS_RULE["min_alt"], **pre)
        for a in range(S):
            w, r = v["win"][a], v["var"][a]
            for h in range(2):
                t = int(r["template_pair_b"] if h else w["template_pair"])
                if t < 0 or not v["seq"][2 * a + h]:
                    continue
                fq += [f"@cluster_{cid}/ins{a}/{'AB'[h]} rows={int(w['lo'])}-{int(w['hi'])} voters={int(r['n_b'] if h else r['n_a'])} "
                       f"template={rds[t][0].decode()} split={int(r['split'])}", v["seq"][2 * a + h].decode(), "+", v["qual"][2 * a + h].decode()]
        for i, (head, _, _) in enumerate(rds):
            per_read[(cid, head)] = "\t".join(str(x) for x in (cid, head.decode(), "".join(".ABo"[int(x)] for x in v["variant"][i]) or "*",
                                                               "".join("=AB."[(int(v["key2"][i]) >> (2 * b)) & 3] for b in range(S)) or "*",
                                                               "." if grp[i] < 0 else int(grp[i]), how[int(hw[i])]))
    rows = [ln.split(b"\t") for ln in open(d / "clusters.tsv", "rb").read().split(b"\n")[1:] if ln]
    rows = [(int(c), rid) for c, _, rid in rows if int(c) in cons]
    assert len(rows) == len(per_read) >= 50
    return fq + [""], ["ClusterId\tRead\tVariants\tInserts\tIsoform\tHow"] + [per_read[r] for r in rows] + [""]   # (the order of clusters.tsv)


@pytest.mark.gpu
@pytest.mark.parametrize("name,min_agree", [("variants", 45), ("strict", 100)])
def test_the_two_files_are_the_host_path(dumps, name, min_agree):
    """every byte of both files, every cluster: the records' heads, sequences and qualities, and every read's row"""
    *_, dirs = dumps
    fq, tsv = _host_files(dirs[name], min_agree)
    assert open(dirs[name] / "cluster_insert_variants.fq").read().split("\n") == fq
    assert open(dirs[name] / "read_insert_variants.tsv").read().split("\n") == tsv


@pytest.mark.gpu
def test_the_threshold_reaches_the_library(dumps):
    *_, dirs = dumps
    files = {name: _files(dirs[name]) for name in ("variants", "strict")}
    assert files["variants"]["cluster_insert_variants.fq"] != files["strict"]["cluster_insert_variants.fq"]
