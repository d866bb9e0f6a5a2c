"""`cluster -A 0|1|2` (src/main.cpp:292-324): the consensus engine's alignment type on the command line.  Without -A, with
-A 0 and with a value the reference's switch does not know the engine aligns locally, as it did before -A was read.  Under
-A 1 and -A 2 the whole command-line path (sort, two leaves, their merge, dump) is held to the oracle with its own POA of the
same type behind its hook, as tests/test_cli.py does without -A."""
import os
import shutil
import subprocess
import tempfile

import pytest

from isonclust2_amd import synth
from tests.test_cli import CLI, _write_fastq, consensus_mode_sort_cluster_merge_dump_vs_oracle, run


def test_help_names_the_option():
    r = subprocess.run([CLI, "cluster", "-h"], capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, ISONCLUST2_SERVE="0"))
    assert r.returncode == 0
    assert "[-A 0|1|2]" in r.stderr and "semi-global" in r.stderr


@pytest.mark.gpu
def test_cluster_A_selects_the_consensus_alignment(tmp_path):
    rs = synth.generate(240, 20, 600, 9, 21, seed=41)
    fq = tmp_path / "reads.fq"
    _write_fastq(rs, fq)
    assert run("sort", "-B", "1000000", "-M", "120", "-g", "3", "-c", "8", "-P", "400", "-o", str(tmp_path / "sorted"), str(fq)).returncode == 0
    b0 = str(tmp_path / "sorted" / "batches" / "isONbatch_0.cer")
    srv = tempfile.mkdtemp(prefix="iocs", dir="/tmp")   # (a unix socket's path holds 107 characters)
    env = dict(os.environ, ISONCLUST2_SERVE_DIR=srv, ISONCLUST2_SERVE_IDLE_S="60")
    off = dict(env, ISONCLUST2_SERVE="0")
    try:
        def cluster(name, *args, e=env):
            out = tmp_path / (name + ".cer")
            r = run("cluster", "-l", b0, "-x", "fast", *args, "-o", str(out), env=e)
            assert r.returncode == 0, r.stderr
            return out.read_bytes(), r.stderr

        local, err = cluster("none", "-v")
        assert "Generating consensus using spoa algorithm: local" in err
        assert cluster("a0", "-A", "0")[0] == local
        assert cluster("a9", "-A", "9")[0] == local          # (the reference's switch leaves kSW for other values)
        for a, name in (("1", "global"), ("2", "semi-global")):
            x, err = cluster("a" + a, "-v", "-A", a)
            assert "Generating consensus using spoa algorithm: " + name in err
            assert x != local, a
            assert cluster("a%s_again" % a, "-A", a)[0] == x, a
            assert cluster("a%s_direct" % a, "-A", a, e=off)[0] == x, a
        assert cluster("a1_b", "-A", "1")[0] != cluster("a2_b", "-A", "2")[0]
        assert cluster("none_again")[0] == local            # (the worker's next job without -A: local again)
    finally:
        run("serve", "stop", env=env)
        shutil.rmtree(srv, ignore_errors=True)


@pytest.mark.gpu
@pytest.mark.parametrize("poa_type", [0, 1, 2])
def test_consensus_mode_sort_cluster_merge_dump_under_A(tmp_path, poa_type):
    """test_cli.test_consensus_mode_sort_cluster_merge_dump with `-A <type>` on the three `cluster` calls and the oracle's POA
    of that type: the assignments after the merge, which hang on every consensus string on the way (a representative replaced
    by a different consensus is re-minimized differently)"""
    consensus_mode_sort_cluster_merge_dump_vs_oracle(tmp_path, poa_type)
