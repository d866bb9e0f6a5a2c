"""Every file the command line writes, against the bytes the binary wrote before main.cpp was split into per-command stages.

tests/golden/cli_parent_outputs.json holds the sha256 of every file of one small chain, recorded twice with that earlier binary
(both recordings equal: no file is left out).  The chain runs in its own directory under relative paths, because the archives
record the paths they were given."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

from isonclust2_amd import synth
from tests.test_cli import CLI, _short_dir, _write_fastq

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_parent_outputs.json")
ALL_REPORTS = ("--read-stats", "--pileup", "--polish", "--sites", "--split", "--split-polish")


def produce(cli, work):
    """sort into two batches, cluster each leaf and merge them in `fast` and in `sahlin` (the read sets of
    test_sort_cluster_merge_dump_matches_oracle), one consensus-mode chain, dump with every report, dump with the weighted polish,
    and the sahlin merge once more through the resident worker.  Returns {path under work: sha256} of every file there."""
    srv = _short_dir()
    # (IOC_NO_PREWARM: a fresh context loads each code object at its first launch instead of on threads beside it — on reads this
    # few the first launch and those threads ask the runtime for the same kernel in the same instant; no file depends on it)
    env = dict(os.environ, ISONCLUST2_SERVE="0", IOC_NO_PREWARM="1")
    env.pop("ISONCLUST2_STATS_JSON", None)

    def run(*args, served=False):
        e = dict(env, ISONCLUST2_SERVE="1", ISONCLUST2_SERVE_DIR=srv, ISONCLUST2_SERVE_IDLE_S="30") if served else env
        r = subprocess.run([cli, *args], capture_output=True, text=True, timeout=300, cwd=str(work), env=e)
        assert r.returncode == 0, (args, r.stderr)

    def chain(name, mode, *sort_flags):
        half = str(reads[name].n // 2)
        run("sort", "-B", "1000000", "-M", half, *sort_flags, "-o", name, name + ".fq")
        for i in ("0", "1"):
            run("cluster", "-l", f"{name}/batches/isONbatch_{i}.cer", "-o", f"{name}_c{i}.cer", "-x", mode)
        run("cluster", "-l", name + "_c0.cer", "-r", name + "_c1.cer", "-o", name + "_m.cer", "-x", mode)

    reads = {"fast": synth.generate(360, 30, 700, 9, 21, seed=21), "sahlin": synth.generate(160, 16, 450, 9, 20, seed=22)}
    reads["cons"] = reads["sahlin"]
    for name, rs in reads.items():
        _write_fastq(rs, os.path.join(work, name + ".fq"))
    try:
        chain("fast", "fast")
        chain("sahlin", "sahlin")
        chain("cons", "fast", "-g", "3", "-c", "8", "-P", "400")
        run("dump", "-i", "sahlin/sorted_reads_idx.cer", "-o", "sahlin_dump", *ALL_REPORTS, "sahlin_m.cer")
        run("dump", "-i", "fast/sorted_reads_idx.cer", "-o", "fast_dump", "--polish", "--polish-weighted", "fast_m.cer")
        run("dump", "-i", "cons/sorted_reads_idx.cer", "-o", "cons_dump", "cons_m.cer")
        run("cluster", "-l", "sahlin_c0.cer", "-r", "sahlin_c1.cer", "-o", "sahlin_m_served.cer", "-x", "sahlin", served=True)
    finally:
        subprocess.run([cli, "serve", "stop"], capture_output=True, timeout=60, env=dict(env, ISONCLUST2_SERVE_DIR=srv))
        shutil.rmtree(srv, ignore_errors=True)
    out = {}
    for d, _, files in os.walk(work):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, work)] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    return out


@pytest.mark.gpu
def test_every_written_file_is_what_the_unsplit_command_line_wrote(tmp_path):
    want = json.load(open(GOLDEN))["files"]
    got = produce(CLI, tmp_path)
    assert sorted(got) == sorted(want)
    assert any(p.startswith("sahlin_dump/cluster_split_polished.fq") for p in got) and "cons_" in open(tmp_path / "cons_dump" / "cluster_cons.fq").read()
    differing = sorted(p for p in want if got[p] != want[p])
    assert not differing, differing
