"""`dump --isoforms --isoforms-polish`: cluster_isoforms.fq (ioc_align_pairs_blocks_polish on the GPU).  The options are parsed and
refused without a GPU.  The read set is that of test_cli_isoforms.py, rebuilt here: ordinary synthetic transcripts and the four
isoforms of blocks_common.property_case at 1 % errors.  cluster_isoforms.fq is recomputed through Context.align_pairs_blocks_polish
from the files `dump` wrote alone.  Every other report file does not change by one byte when the option stands beside it."""
import os

import numpy as np
import pytest

from isonclust2_amd import api, synth
from tests import blocks_common as bc
from tests.test_cli import run
from tests.test_cli_read_stats import K, _fastq_records, _files

ALL = ["--sites", "--read-stats", "--pileup", "--polish", "--correct"]
NAMES = {"isoforms": ["--isoforms"], "polish": ["--isoforms", "--isoforms-polish"],
         "isoforms_all": ["--isoforms"] + ALL, "polish_all": ["--isoforms", "--isoforms-polish"] + ALL,
         "isoforms_stats": ["--isoforms", "--read-stats", "--pileup"], "polish_stats": ["--isoforms", "--isoforms-polish", "--read-stats", "--pileup"],
         "polish_rule": ["--isoforms", "--isoforms-polish", "--isoforms-polish-min-depth", "1", "--isoforms-polish-max", "2"]}
CALLS = {"polish": dict(polish_min_depth=3, max_iso=16), "polish_rule": dict(polish_min_depth=1, max_iso=2)}
NEW = {"cluster_isoforms.fq"}


def test_the_options_are_parsed_and_in_the_help(tmp_path):
    base = ("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--isoforms", "--isoforms-polish")
    for flag, bad in (("--isoforms-polish-min-depth", "0"), ("--isoforms-polish-min-depth", "x"), ("--isoforms-polish-max", "0"), ("--isoforms-polish-max", "all")):
        r = run(*base, flag, bad, "nothing.cer")
        assert r.returncode == 1 and flag in r.stderr and "must be" in r.stderr, (flag, bad)
    r = run(*base, "--isoforms-polish-min-depth", "2", "--isoforms-polish-max", "40", "nothing.cer")
    assert r.returncode == 1 and "--isoforms" not in r.stderr and "must be" not in r.stderr   # (as far as the batch)
    r = run("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--isoforms-polish", "nothing.cer")
    assert r.returncode == 1 and "--isoforms-polish asks for --isoforms" in r.stderr
    s = run("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"), "--split-polish", "nothing.cer")
    assert s.returncode == 1 and "--split-polish asks for --split" in s.stderr            # (it dies as that one does)
    h = run("dump", "--help")
    words = " ".join(h.stderr.split())
    assert h.returncode == 0 and all(w in h.stderr for w in ("--isoforms-polish ", "--isoforms-polish-min-depth", "--isoforms-polish-max", "cluster_isoforms.fq"))
    assert "default 16: a choice" in words and "--isoforms-polish-min-depth N positions covered by fewer than N reads of the isoform" in words and "(default 3)" in words


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("isoforms_polish")
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
    for with_, without in (("polish", "isoforms"), ("polish_all", "isoforms_all"), ("polish_stats", "isoforms_stats"), ("polish_rule", "isoforms")):
        assert set(files[with_]) == set(files[without]) | NEW, with_
        for f in files[without]:
            assert files[with_][f] == files[without][f], (with_, f)
    assert files["polish_all"]["cluster_isoforms.fq"] == files["polish"]["cluster_isoforms.fq"] == files["polish_stats"]["cluster_isoforms.fq"]
    assert files["polish_rule"]["cluster_isoforms.fq"] != files["polish"]["cluster_isoforms.fq"]


@pytest.mark.gpu
def test_the_file_is_the_library_call(dumps):
    d = dumps["polish"]
    cons = {int(head.split(b" ")[0][8:]): (seq, qual) for head, seq, qual in _fastq_records(d / "cluster_cons.fq")}
    reads = {cid: (_fastq_records(d / "cluster_fastq" / f"{cid}.fq") if os.path.exists(d / "cluster_fastq" / f"{cid}.fq") else []) for cid in cons}
    lines = [q for _, q in cons.values()] + [q for cid in cons for _, _, q in reads[cid]]
    offs = np.zeros(len(lines) + 1, np.int64)
    offs[1:] = np.cumsum([len(q) for q in lines])
    ctx = api.Context(0)
    _, err = ctx.qual_scores(offs, np.frombuffer(b"".join(lines), np.uint8), K)
    err = [float(e) for e in err]
    cons_err, read_err = dict(zip(cons, err)), iter(err[len(cons):])
    seqs, pairs, sop, segs, seg_cls = [], [], [], [], []
    for cid, (ref, _) in cons.items():
        if not reads[cid]:
            continue
        seqs.append(ref)
        segs.append((len(seqs) - 1, 0))
        seg_cls.append(cid)
        for head, s, q in reads[cid]:
            seqs.append(s)
            pairs.append((len(seqs) - 1, segs[-1][0], 0, next(read_err) + cons_err[cid]))
            sop.append(len(segs) - 1)
    ctx.align_set_pool(seqs)
    assert len(pairs) >= 60
    for name, call in CALLS.items():
        got = ctx.align_pairs_blocks_polish(pairs, K, segs, sop, rows=False, **call)
        want, planted = [], 0
        for g, cid in sorted(enumerate(seg_cls), key=lambda t: t[1]):   # (cluster order)
            z, mine = got["seg"][g], got["reads"][[x for x, s in enumerate(sop) if s == g]]
            if int(z["n_blocks"]) < 1:
                continue
            assert len(got["gseq"][g]) == min(int(z["n_groups"]), call["max_iso"])
            for h, (seq, qual, st) in enumerate(zip(got["gseq"][g], got["gqual"][g], got["gpolish"][g])):
                direct = mine[(mine["group"] == h) & (mine["how"] == api.ISO_DIRECT)]
                n = len(direct) + int(((mine["group"] == h) & (mine["how"] == api.ISO_ASSIGNED)).sum())
                head = (f"@cluster_{cid}/iso{h} key={bc.signature(direct['key'][0], int(z['n_blocks']))} reads={n} subs={int(st['n_sub'])} dels={int(st['n_del'])} "
                        f"ins={int(st['n_ins'])} low={int(st['n_low'])}")
                want += [head.encode(), seq, b"+", qual]
            if int(z["n_blocks"]) == 2 and int(z["n_groups"]) == 4:
                planted += 1
                if name == "polish":   # the planted transcript: an isoform that skips a block is shorter by about the block
                    lens = {bc.signature(mine[(mine["group"] == h) & (mine["how"] == api.ISO_DIRECT)]["key"][0], 2): len(q) for h, q in enumerate(got["gseq"][g])}
                    assert set(lens) == {"==", "-=", "=-", "--"} and lens["=="] > lens["-="] > lens["=-"] > lens["--"], lens
        assert open(dumps[name] / "cluster_isoforms.fq", "rb").read().split(b"\n") == want + [b""], name
        assert planted >= 1 and len(want) >= 4 * (4 if name == "polish" else 2)
    ctx.close()
