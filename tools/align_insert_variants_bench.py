#!/usr/bin/env python3
"""What telling two exons at one junction apart costs (align_pairs_blocks_inserts_variants), on the four batches of
tools/align_inserts_bench.py — where no site holds two exons and the stage has only to find that out — and on a batch that plants
them, beside the call it extends.

    tools/align_insert_variants_bench.py [CALLS=7] [--seq-only]

Per batch, after two warm-up calls of each route, CALLS rounds of the calls in turn; wall milliseconds per call of the Python
wrapper as median (min - max): align_pairs_blocks_inserts_seq (the call the fused one extends; --seq-only measures it alone: run
from the root of a checkout of the parent commit it gives the parent's figure) and align_pairs_blocks_inserts_variants.  Then the
device times from the IOC_TRACE lines of both calls, every kernel of the window stage and of the variant stage on its own
(k_win_align is round A, k_win_align_b round B; in the fused call k_win_group_pile piles the slots and the window call's own sites,
k_win_pile_call calls both), and the share of the voters that reach round B.  profiles/insert_variants.txt holds the tables."""
import random
import re
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from isonclust2_amd import api  # noqa: E402
from align_blocks_bench import four_isoforms  # noqa: E402
from align_inserts_bench import short_representative  # noqa: E402
from align_split_bench import sliced, traced  # noqa: E402
from align_split_polish_bench import two_variants  # noqa: E402

WINDOW = ("k_win_bounds", "k_win_template", "k_win_align", "k_win_group_pile", "k_win_pile_call")
VARIANTS = ("k_win_agree", "k_win_template_far", "k_win_align_b", "k_win_decide", "k_win_rekey", "k_winvar_support", "k_winvar_isoforms", "k_winvar_record")


def two_exons(n_segs=4, n_each=(60, 60, 40), rate=0.08, seed=3):
    """n_segs clusters of 1000-base representatives that lack an exon at 300 where 60 reads hold one of 60 bases, 60 another of 45 and
    40 none, 8 % errors: (name, seqs, pairs, segs, seg_of_pair, None) as the other batches are"""
    rng = random.Random(seed)
    rand = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))

    def mutate(s):
        out = bytearray()
        for b in s:
            u = rng.random()
            if u < rate / 3:
                continue
            if u < 2 * rate / 3:
                out.append(rng.choice(b"ACGT"))
            out.append(rng.choice(b"ACGT") if u > 1 - rate / 3 else b)
        return bytes(out)

    frames = [rand(1000) for _ in range(n_segs)]
    seqs, pairs = list(frames), []
    for g, f in enumerate(frames):
        iso = [f[:300] + rand(60) + f[300:], f[:300] + rand(45) + f[300:], f]
        for x, n in enumerate(n_each):
            for _ in range(n):
                pairs.append((len(seqs), g, 0, 0.1))
                seqs.append(mutate(iso[x]))
    return "two exons at one junction", seqs, pairs, [(g, 0) for g in range(n_segs)], [p[1] for p in pairs], None


def device_times(fn, calls):
    dev = {k: [] for k in WINDOW + VARIANTS}
    share = None
    for _ in range(calls):
        _, text = traced(fn)
        line = " ".join(ln.strip() for ln in text.splitlines() if "aligner: blocks inserts seq:" in ln or "aligner: window variants:" in ln)
        for k in dev:
            m = re.search(re.escape(k) + r" ([0-9.]+) ms", line)
            if m:
                dev[k].append(float(m.group(1)))
        m = re.search(r"(\d+) voters, (\d+) of them in round B", line)
        if m:
            share = (int(m.group(1)), int(m.group(2)))
    return dev, share


def main(calls, seq_only):
    ctx = api.Context(0)
    for name, seqs, pairs, segs, sop, _ in (sliced(), two_variants(), four_isoforms(), short_representative(), two_exons()):
        ctx.align_set_pool(seqs)
        routes = {"align_pairs_blocks_inserts_seq": lambda: ctx.align_pairs_blocks_inserts_seq(pairs, 11, segs, sop)}
        if not seq_only:
            routes["align_pairs_blocks_inserts_variants"] = lambda: ctx.align_pairs_blocks_inserts_variants(pairs, 11, segs, sop)
        for fn in routes.values():
            fn(), fn()
        ms = {k: [] for k in routes}
        for _ in range(calls):
            for k, fn in routes.items():
                t0 = time.perf_counter()
                fn()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        print(f"{name}: {len(pairs)} pairs")
        print(f"  wall ms per call: median (min - max) over {calls} calls, the calls in turn")
        for k, v in ms.items():
            print(f"  {k:<40} {statistics.median(v):9.3f} ({min(v):.3f} - {max(v):.3f})")
        for k, fn in routes.items():
            dev, share = device_times(fn, calls)
            print(f"  device ms of {k}: median (min - max) over {calls} calls")
            for kernel, v in dev.items():
                if v:
                    print(f"    {kernel:<20} {statistics.median(v):8.3f} ({min(v):.3f} - {max(v):.3f})")
            if share:
                print(f"    voters {share[0]}, in round B {share[1]} ({100.0 * share[1] / max(share[0], 1):.1f} %)")
        if not seq_only:
            v = routes["align_pairs_blocks_inserts_variants"]()["insert_variants"]
            print("  variants:", [tuple(int(x) for x in r)[:7] for r in v["var"]][:6], "groups", [int(x) for x in v["seg"]["n_groups"]][:6])
    ctx.close()
    return 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--seq-only"]
    sys.exit(main(int(args[0]) if args else 7, "--seq-only" in sys.argv[1:]))
