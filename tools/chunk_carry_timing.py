#!/usr/bin/env python3
"""What the step between two chunks of a chunked ioc_cluster_merge costs.

The config-2 fast-mode batch (3000 reads, seed 1) goes through ioc_cluster_merge with IOC_MERGE_CHUNK=500 under IOC_TRACE.  The
library's trace has a line at the end of a chunk's resolve ("resolve + decisions") and one where the next chunk's left state
is in place and its index build starts ("left state load"); this tool runs the clustering in a child process, stamps every
trace line as it arrives (the library writes them unbuffered) and reports the time between those two lines: the carry, plus
the next chunk's gates and query upload, which do not depend on how the left state travels.  The same tool measures any
build of the package: --package-root names the tree whose isonclust2_amd is imported.

    python tools/chunk_carry_timing.py [--package-root DIR] [--runs 12] [--warmup 3] [--chunk 500]

Prints one line per gap of every measured run and a summary (median, quartiles, min, max over all gaps; per run the sum)."""
import argparse
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))


def child(a):
    sys.path.insert(0, a.package_root)
    from isonclust2_amd import api, pipeline, synth
    ctx = api.Context(0)
    rs = synth.generate_config("config2", seed=1)
    sb, _ = pipeline.sort_stage(ctx, rs, 11, 15)
    p = api.default_params(11, 15, "fast")
    view = {k: v for k, v in sb.view.items() if k not in ("raw_seq", "raw_off")}
    ref = None
    for r in range(a.warmup + a.runs):
        sys.stderr.write(f"[carry] run {r} {'warmup' if r < a.warmup else 'measured'}\n")
        sys.stderr.flush()
        cls, strand, st = ctx.cluster_batch(p, view)
        sys.stderr.write("[carry] end\n")
        sys.stderr.flush()
        if ref is None:
            ref = (cls.copy(), int(st["n_clusters"]))
        assert (cls == ref[0]).all() and int(st["n_clusters"]) == ref[1]
    sys.stderr.write(f"[carry] clusters {ref[1]}\n")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package-root", default=os.path.dirname(HERE))
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=500)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    a.package_root = os.path.abspath(a.package_root)
    if a.child:
        return child(a)
    env = dict(os.environ, IOC_TRACE="1", IOC_MERGE_CHUNK=str(a.chunk), PYTHONUNBUFFERED="1")
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--package-root", a.package_root, "--runs", str(a.runs), "--warmup", str(a.warmup)]
    pr = subprocess.Popen(cmd, env=env, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, bufsize=0)
    measured, t_resolve, gaps, runs, clusters = False, None, [], [], None
    for raw in iter(pr.stderr.readline, b""):
        t = time.perf_counter()
        line = raw.decode(errors="replace").rstrip()
        if line.startswith("[carry] run"):
            measured, t_resolve = line.endswith("measured"), None
            if measured:
                runs.append([])
        elif line.startswith("[carry] clusters"):
            clusters = int(line.split()[-1])
        elif line.startswith("[carry] end"):
            t_resolve = None
        elif not line.startswith("[ioc]"):
            sys.stderr.write(line + "\n")          # (a traceback of the child, a warning of the runtime)
        elif measured and line.startswith("[ioc] resolve + decisions"):
            t_resolve = t
        elif measured and line.startswith("[ioc] left state load") and t_resolve is not None:
            runs[-1].append((t - t_resolve) * 1e3)
            t_resolve = None
    if pr.wait() != 0:
        sys.exit(f"the measured process ended with status {pr.returncode}")
    for i, r in enumerate(runs):
        print(f"run {i:2d}: {len(r)} carries, sum {sum(r):8.3f} ms: " + " ".join(f"{x:.3f}" for x in r))
        gaps += r
    q = statistics.quantiles(gaps, n=4)
    sums = [sum(r) for r in runs]
    print(f"package {a.package_root}: {clusters} clusters, chunk {a.chunk}, {len(runs)} runs after {a.warmup} warm-up runs")
    print(f"carry per chunk boundary [ms]: median {statistics.median(gaps):.3f}, quartiles {q[0]:.3f} .. {q[2]:.3f}, min {min(gaps):.3f}, max {max(gaps):.3f} ({len(gaps)} gaps)")
    print(f"carries of one call [ms]: median {statistics.median(sums):.3f}, min {min(sums):.3f}, max {max(sums):.3f}")


if __name__ == "__main__":
    main()
