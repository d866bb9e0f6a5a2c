"""`dump ... --isoforms-inserts-variants --isoforms-full-variants`: cluster_isoforms_full_variants.fq
(ioc_align_pairs_isoforms_full_variants on the GPU).  The option is parsed, refused and in the help without a GPU.  The read set is that
of test_cli_isoforms_insert_variants.py: an 800-base representative that lacks an exon at row 150 where 8 reads hold a 60-base exon, 8
a different one of 45 bases and 6 none, at 1 % errors — three isoforms once the variants are told apart.  The new file must hold a
record for each, each nearer its own transcript than the other two; every record of every cluster is rebuilt line for line on the host
path from the files `dump` wrote alone; and every other file of the run is byte for byte the --isoforms-inserts-variants run's."""
import os
import random
import re

import numpy as np
import pytest

from isonclust2_amd import api, synth
from tests import iso_polish_common as ipc
from tests import polish_common as pc
from tests.test_cli import run
from tests.test_cli_isoforms_insert_variants import AT, EXONS, SIZES, SEQ
from tests.test_cli_read_stats import K, _fastq_records, _files

VAR = SEQ + ["--isoforms-inserts-variants"]
NAMES = {"variants": VAR, "full": VAR + ["--isoforms-full-variants"], "full_2": VAR + ["--isoforms-full-variants", "--isoforms-full-max", "2"]}
NEW = "cluster_isoforms_full_variants.fq"


def test_the_option_is_parsed_refused_and_in_the_help(tmp_path):
    base = ("dump", "-i", "nowhere.cer", "-o", str(tmp_path / "x"))
    r = run(*base, *VAR, "--isoforms-full-variants", "--isoforms-full-max", "3", "nothing.cer")
    assert r.returncode == 1 and "--isoforms" not in r.stderr and "must be" not in r.stderr   # (as far as the batch)
    for without in (SEQ, ["--isoforms", "--isoforms-inserts"], []):
        r = run(*base, *without, "--isoforms-full-variants", "nothing.cer")
        assert r.returncode == 1 and "--isoforms-full-variants asks for --isoforms-inserts-variants" in r.stderr, without
    for order in (["--isoforms-full-variants", "--isoforms-full"], ["--isoforms-full", "--isoforms-full-variants"]):
        r = run(*base, *VAR, *order, "nothing.cer")
        assert r.returncode == 1 and "--isoforms-full-variants is not offered together with --isoforms-full" in r.stderr and "one fused call a run" in r.stderr
    r = run(*base, *VAR, "--isoforms-full", "nothing.cer")   # the refusal that existed stays
    assert r.returncode == 1 and "--isoforms-inserts-variants is not offered together with --isoforms-full" in r.stderr
    r = run(*base, *VAR, "--isoforms-full-variants", "--isoforms-full-max", "0", "nothing.cer")
    assert r.returncode == 1 and "--isoforms-full-max" in r.stderr and "must be" in r.stderr
    h = run("dump", "--help")
    assert h.returncode == 0 and all(w in h.stderr for w in ("--isoforms-full-variants ", NEW, "ins<b>/<A|B>@<at>+<len>", "one fused call a run"))


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("isoforms_full_variants")
    fq = tmp / "reads.fq"
    rng = random.Random(4)
    frame = bytes(rng.choice(b"ACGT") for _ in range(800))
    exons = [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in EXONS]
    iso = [frame[:AT] + exons[0] + frame[AT:], frame[:AT] + exons[1] + frame[AT:], frame]
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
                i += 1
    out = tmp / "sorted"
    r = run("sort", "-o", str(out), str(fq))
    assert r.returncode == 0, r.stderr
    r = run("cluster", "-l", str(out / "batches" / "isONbatch_0.cer"), "-o", str(tmp / "c.cer"), "-x", "fast", env=dict(os.environ, ISONCLUST2_SERVE="0"))
    assert r.returncode == 0, r.stderr
    for name, extra in NAMES.items():
        r = run("dump", "-i", str(out / "sorted_reads_idx.cer"), "-o", str(tmp / name), *extra, str(tmp / "c.cer"))
        assert r.returncode == 0, r.stderr
    return iso, {name: tmp / name for name in NAMES}


@pytest.mark.gpu
def test_every_other_file_is_the_variants_run(dumps):
    _, dirs = dumps
    files = {name: _files(d) for name, d in dirs.items()}
    for with_ in ("full", "full_2"):
        assert set(files[with_]) == set(files["variants"]) | {NEW}, with_
        for f in files["variants"]:
            assert files[with_][f] == files["variants"][f], (with_, f)


HEAD = rb"cluster_(\d+)/iso(\d+) key=([=\-~.*]+)/([=AB.*]+) reads=(\d+) subs=\d+ dels=\d+ ins=\d+ low=\d+((?: ins\d+/[AB]@\d+\+\d+)*)"


@pytest.mark.gpu
def test_a_record_per_isoform_each_nearest_its_own_transcript(dumps):
    iso, dirs = dumps
    every = _fastq_records(dirs["full"] / NEW)
    var = _fastq_records(dirs["full"] / "cluster_insert_variants.fq")
    assert len(var) == 2
    slot = {re.match(rb"cluster_\d+/ins0/([AB]) ", h).group(1): s for h, s, _ in var}
    cid = int(re.match(rb"cluster_(\d+)/", var[0][0]).group(1))
    recs = [r for r in every if r[0].startswith(b"cluster_%d/" % cid)]
    assert len(recs) == 3, [r[0] for r in every]
    # which exon each letter stands for: the one its record of cluster_insert_variants.fq holds
    exon_of = {v: min((0, 1), key=lambda x: ipc.edit_distance(s, iso[x][AT - 20:AT + EXONS[x] + 20])) for v, s in slot.items()}
    assert sorted(exon_of.values()) == [0, 1]
    seen = []
    for h, (head, seq, qual) in enumerate(recs):
        m = re.fullmatch(HEAD, head)
        assert m and int(m.group(2)) == h and len(seq) == len(qual) and int(m.group(5)) >= 3, head
        sites = m.group(4).decode()
        own = 2 if sites == "=" else exon_of[sites.encode()]
        dist = [ipc.edit_distance(seq, t) for t in iso]
        print(head, dist)
        assert dist[own] < min(d for x, d in enumerate(dist) if x != own), (head, dist)
        seen.append(own)
        spliced = re.findall(rb" ins(\d+)/([AB])@(\d+)\+(\d+)", m.group(6))
        assert (len(spliced) == 1) == (sites in "AB"), head
        if spliced:   # the record of cluster_insert_variants.fq that the tail names stands where it says
            b, v, at, ln = int(spliced[0][0]), spliced[0][1], int(spliced[0][2]), int(spliced[0][3])
            assert b == 0 and v.decode() == sites and seq[at:at + ln] == slot[v]
    # each another transcript; the reads are the planted ones, and the representative itself among those that lack the exon
    assert sorted(seen) == [0, 1, 2] and [int(re.fullmatch(HEAD, r[0]).group(5)) for r in recs] == [SIZES[2] + 1 if x == 2 else SIZES[x] for x in seen]
    # --isoforms-full-max 2: the first two isoforms of every cluster
    assert _fastq_records(dirs["full_2"] / NEW) == [r for r in every if re.match(rb"cluster_\d+/iso[01] ", r[0])]


def _host_file(d, max_iso=16):
    """the lines of cluster_isoforms_full_variants.fq on the host path, from the dump directory d: the host aligner, the host
    projections, the block, insert and variant definitions, ioc_host_key_isoforms, ioc_host_planes_pile and
    ioc_host_isoform_splice_variants over every dumped cluster"""
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
    out = []
    for cid in sorted(cons):   # (cluster order)
        ref, rds = cons[cid][0], reads[cid]
        if not rds:
            continue
        base, slots, ilen, qpos = [], [], [], []
        for _, rd, _ in rds:
            ops, _ = api.host_align_ops(rd, ref, gap_open=pc.gap_open(next(read_err) + cons_err[cid]))
            base.append(api.ops_project(ops, rd, len(ref))[0]), slots.append(api.ops_project_ins(ops, rd, len(ref)))
            ilen.append(api.ops_project_ilen(ops, len(ref))), qpos.append(api.ops_project_qpos(ops, len(ref)))
        ba, la, qa = np.array(base, np.uint8), np.array(ilen, np.uint8), np.array(qpos, np.uint32)
        blocks = api.planes_blocks(ba)
        nb = len(blocks["blocks"])
        pk = blocks["reads"]["key"].copy()
        pm = np.array([sum(3 << (2 * b) for b in range(nb) if (int(k) >> (2 * b)) & 3 != api.BLOCK_NONE) for k in pk], np.uint64)
        pre = dict(pre_key=pk, pre_mask=pm, pre_full=(1 << (2 * nb)) - 1)
        ins = api.planes_inserts(ba, la, **pre)
        S = len(ins["sites"])
        if nb < 1 and S < 1:
            continue
        v = api.insert_window_variants(ba, qa, [len(rd) for _, rd, _ in rds], ins["sites"], ins["reads"]["key"], [rd for _, rd, _ in rds])
        grp, hw, counts = api.key_isoforms(v["key2"], v["mask2"], (1 << (2 * S)) - 1, api.INSERTS_RULE["min_alt"], **pre)
        for h in range(min(counts["n_groups"], max_iso)):
            members = [i for i in range(len(rds)) if int(grp[i]) == h]
            first = [i for i in members if int(hw[i]) == api.ISO_DIRECT][0]
            cols, tins = np.zeros(len(ref) + 1, api.PILEUP_DTYPE), np.zeros(len(ref) + 1, api.PILEUP_INS_DTYPE)
            for i in members:
                api.planes_pile(base[i], slots[i], cols=cols, ins=tins)
            key2 = int(v["key2"][first])
            seq, qual, st, sites, _ = api.isoform_splice_variants(cols, tins, ref, key2, v["win"], v["var"], list(zip(v["seq"], v["qual"])), 3)
            bsig = "".join("=-~."[(int(pk[first]) >> (2 * b)) & 3] for b in range(nb)) or "*"
            vsig = "".join("=AB."[(key2 >> (2 * b)) & 3] for b in range(S)) or "*"
            tail = "".join(f" ins{b}/{'AB'[((key2 >> (2 * b)) & 3) == api.INS_CARRY_B]}@{int(sites[b]['at'])}+{int(sites[b]['len'])}" for b in range(S)
                           if int(sites[b]["state"]) == api.SPLICE_DONE)
            out += [f"@cluster_{cid}/iso{h} key={bsig}/{vsig} reads={len(members)} subs={st['n_sub']} dels={st['n_del']} ins={st['n_ins']} low={st['n_low']}{tail}",
                    seq.decode(), "+", qual.decode()]
    return out + [""]


@pytest.mark.gpu
@pytest.mark.parametrize("name,max_iso", [("full", 16), ("full_2", 2)])
def test_the_file_is_the_host_path(dumps, name, max_iso):
    """every byte, every cluster: the records' heads, sequences and qualities"""
    _, dirs = dumps
    want = _host_file(dirs[name], max_iso)
    assert len(want) >= 4 * min(3, max_iso) + 1 and open(dirs[name] / NEW).read().split("\n") == want
