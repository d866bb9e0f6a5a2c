"""What the tests of the full-length sequence by variant share: py_splice_variants, ioc_host_isoform_splice_variants restated over
splice_common.py_splice — the key with every 2 turned into 1, the window records with tlen replaced, the chosen slot of every site as
that site's window —; random plans with variant records; the definition of the device entry group-segment by group-segment from the
host functions; the six slot planes of a variants_common.plant segment; and the property case of variants_common, two exons at the
first junction, carried on to the isoforms' transcripts."""
import random

import numpy as np

from isonclust2_amd import api
from tests import blocks_common as bc
from tests import inserts_common as ic
from tests import iso_polish_common as ipc
from tests import polish_common as pc
from tests import splice_common as sc
from tests import variants_common as vc
from tests import windows_common as wc

CARRY, CARRY_B = api.INS_CARRY, api.INS_CARRY_B


def as_windows(key2, win, var, slot_seq):
    """(key, win, win_seq) of the splice that key2 asks for: what ioc_host_isoform_splice is to be run over"""
    key, w, ws = 0, np.array(win, api.INSERT_WINDOW_DTYPE), []
    for b in range(len(win)):
        s = (int(key2) >> (2 * b)) & 3
        which = 1 if s == CARRY_B else 0
        if which:
            w[b]["tlen"] = int(var[b]["tlen_b"]) if int(var[b]["split"]) else 0
        key |= (CARRY if s == CARRY_B else s) << (2 * b)
        ws.append(slot_seq[2 * b + which])
    return key | (int(key2) >> (2 * len(win)) << (2 * len(win))), w, ws


def py_splice_variants(cols, ins, frame, key2, win, var, slot_seq, min_depth):
    """ioc_host_isoform_splice_variants as api.isoform_splice_variants returns it, from the rules through py_splice"""
    return sc.py_splice(cols, ins, frame, *as_windows(key2, win, var, slot_seq), min_depth)


def variants(split, tlen_b=None):
    """WINDOW_VARIANT_DTYPE records of a split flag a site; tlen_b 1 where it splits unless given"""
    v = np.zeros(len(split), api.WINDOW_VARIANT_DTYPE)
    v["template_pair_b"] = -1
    for b, s in enumerate(split):
        v[b]["split"], v[b]["tlen_b"] = s, (int(s) if tlen_b is None else tlen_b[b])
        v[b]["template_pair_b"] = 0 if s else -1
    return v


def random_plan(rng, rlen, n_sites, lens=(0, 1, 8, 40)):
    """(key2, win, var, slot_seq): splice_common.random_plan's key (every state at every site), windows and A slots, and beside them
    variant records with split 0 and 1 and B slots of the same lengths — empty where the site does not split"""
    key, win, a = sc.random_plan(rng, rlen, n_sites, lens)
    split = [int(x) for x in rng.integers(0, 2, n_sites)]
    var = variants(split, [5 * s for s in split])
    slot_seq = []
    for b in range(n_sites):
        slot_seq += [a[b], sc.random_string(rng, int(rng.choice(lens)) if split[b] else 0)]
    return key, win, var, slot_seq


def host_isoforms_full_variants(frames, seg_of_pair, group, n_groups, base, slots, iso_key, win, var, slot_seq, slot_qual, min_depth):
    """The definition of ioc_planes_isoforms_full_variants from the host functions: api.isoform_splice_variants over the tables
    api.planes_pile adds up from every group's pairs.  A dict like splice_common.host_isoforms_full's."""
    ns = len(frames)
    gseg_off, gmem_off, gmembers = ipc.py_group_member_lists(ns, seg_of_pair, group, n_groups)
    out = {"gseq": [], "gqual": [], "gpolish": [], "gseg_off": np.array(gseg_off, np.int64), "splice": [], "grow0": []}
    gcols, gins, sst, off, spoff, rows = [], [], [], [0], [0], 0
    for g, frame in enumerate(frames):
        out["gseq"].append([]), out["gqual"].append([])
        pol = np.zeros(int(n_groups[g]), api.POLISH_STATS_DTYPE)
        for h in range(int(n_groups[g])):
            x = gseg_off[g] + h
            cols, ins = np.zeros(len(frame) + 1, api.PILEUP_DTYPE), np.zeros(len(frame) + 1, api.PILEUP_INS_DTYPE)
            for i in gmembers[gmem_off[x]:gmem_off[x + 1]]:
                api.planes_pile(base[i], slots[i], cols=cols, ins=ins)
            s, q, st, sites, ss = api.isoform_splice_variants(cols, ins, frame, int(iso_key[x]), win[g], var[g], list(zip(slot_seq[g], slot_qual[g])), min_depth)
            out["gseq"][g].append(s), out["gqual"][g].append(q), out["splice"].append(sites), out["grow0"].append(rows)
            for f in api.POLISH_STATS_FIELDS:
                pol[h][f] = st[f]
            rec = np.zeros(1, api.SPLICE_STATS_DTYPE)[0]
            for f in api.SPLICE_STATS_FIELDS:
                rec[f] = ss[f]
            sst.append(rec), gcols.append(cols), gins.append(ins), off.append(off[-1] + len(s)), spoff.append(spoff[-1] + len(sites))
            rows += len(frame) + 1
        out["gpolish"].append(pol)
    cat = lambda parts, dt: np.concatenate([np.zeros(0, dt)] + parts)
    out.update(off=np.array(off, np.int64), splice_off=np.array(spoff, np.int64), sstats=np.array(sst, api.SPLICE_STATS_DTYPE).reshape(-1),
               gcols=cat(gcols, api.PILEUP_DTYPE), gins=cat(gins, api.PILEUP_INS_DTYPE), grow0=np.array(out["grow0"], np.int64))
    return out


def plant_slots(reads, qpos):
    """The six slot planes (api.ops_project_ins) of every read of a variants_common.plant segment.  Such a read is its frame with runs
    inserted, so its operation string follows from its position plane: the run in front of row r holds qpos[r + 1] - qpos[r] - 1
    bases, the one behind the last row what is left of the read."""
    out = []
    for rd, q in zip(reads, qpos):
        rlen = len(q) - 1
        ops = b"".join(b"I" * (int(q[r + 1]) - int(q[r]) - 1) + b"=" for r in range(rlen)) + b"I" * (len(rd) - int(q[rlen]))
        assert api.ops_project_qpos(ops, rlen).tolist() == [int(x) for x in q]
        out.append(api.ops_project_ins(ops, rd, rlen))
    return out


def regroup(key2, mask2, n_sites, **pre):
    """the isoforms counted again (rule 7 of the variant stage): (group, how, n_groups)"""
    g, h, c = api.key_isoforms(key2, mask2, (1 << (2 * n_sites)) - 1, api.INSERTS_RULE["min_alt"], **pre)
    return g, h, int(c["n_groups"])


def group_keys2(group, how, key2, n_groups):
    """key2 of the lowest-numbered DIRECT read of every group of one segment (0 for a group without one)"""
    keys = np.zeros(n_groups, np.uint64)
    for h in range(n_groups):
        mine = [i for i in range(len(group)) if int(group[i]) == h and int(how[i]) == api.ISO_DIRECT]
        keys[h] = key2[mine[0]] if mine else 0
    return keys


# ---- the property case ----
# variants_common.property_reads: 10 + 10 + 6 + 6 reads at 8 % errors of four true isoforms — exon A (60 bases) or exon B (45) at the
# first junction with [400, 520) behind it, [400, 520) alone, neither — against representative A, through the host aligner, the host
# projections and the definitions.  Counted again the variant stage finds four isoforms where the insert stage found three; each is
# spliced by variant and measured (edit distance) against the four true transcripts, in the order of property_reads' `iso` list.
# The conditions: four isoforms, each of another true isoform and nearer its own transcript than any other; every isoform that
# carries an exon nearer its transcript than the unspliced call of the same tables by at least half the carried exons' length
# (splice_common.property_holds' conditions); and the isoform whose key2 has CARRY_B at the first site at least min(EXONS) / 2
# nearer its own transcript than ioc_host_isoform_splice of the same tables under the same key, which drops that exon.
SECOND = bc.CUTS[1][1] - bc.CUTS[1][0]   # the exon [400, 520) of the transcript, which the representative lacks as well
# measured on the host path at variants_common.SEED; pinned as equalities in tests/test_iso_splice_variants_host.py: per isoform
# counted again, in the library's order, (its key2, its reads, its true isoform, the distances of its sequence by variant to the four
# true transcripts, those of the parent's splice of the same tables under the same key2, those of the unspliced call)
PINNED = ((0, 7, 3, (180, 165, 120, 0), (180, 165, 120, 0), (180, 165, 120, 0)),
          (4, 5, 2, (60, 45, 0, 120), (60, 45, 0, 120), (174, 159, 114, 6)),
          (5, 10, 1, (34, 1, 44, 164), (33, 4, 47, 167), (172, 157, 116, 8)),
          (6, 8, 0, (0, 34, 60, 180), (60, 45, 0, 120), (174, 159, 114, 6)))


def true_transcripts(seed=None):
    """the four true transcripts of variants_common.property_reads, in the order of its `iso` list (the transcript T is the first
    thousand draws of the seed's generator, as there)"""
    seed = vc.SEED if seed is None else seed
    frame, (ea, eb), _, _ = vc.property_reads(seed)
    rng = random.Random(seed)
    T = bytes(rng.choice(b"ACGT") for _ in range(1000))
    assert ic.representative(T, "A") == frame
    a0, j2, second = bc.CUTS[0][0], ic.JUNCTIONS_A[1], T[bc.CUTS[1][0]:bc.CUTS[1][1]]
    return [frame[:a0] + ea + frame[a0:j2] + second + frame[j2:], frame[:a0] + eb + frame[a0:j2] + second + frame[j2:], frame[:j2] + second + frame[j2:], frame]


def carried(true_iso):
    """the total length of the exons true isoform x holds and the representative lacks"""
    return (vc.EXONS[0] + SECOND, vc.EXONS[1] + SECOND, SECOND, 0)[true_iso]


def host_case(seed=None, min_depth=3):
    """the property case on the host path: frame, reads, the planes per read, the insert stage's result, the variant stage's, the
    isoforms counted again and their keys"""
    frame, exons, reads, planted = vc.property_reads(vc.SEED if seed is None else seed)
    base, slots, ilen, qpos = [], [], [], []
    for rd in reads:
        ops, _ = api.host_align_ops(rd, frame, gap_open=pc.gap_open(0.1))
        base.append(api.ops_project(ops, rd, len(frame))[0]), slots.append(api.ops_project_ins(ops, rd, len(frame)))
        ilen.append(api.ops_project_ilen(ops, len(frame))), qpos.append(api.ops_project_qpos(ops, len(frame)))
    ba, la, qa = np.array(base, np.uint8), np.array(ilen, np.uint8), np.array(qpos, np.uint32)
    ins = api.planes_inserts(ba, la)
    var = api.insert_window_variants(ba, qa, [len(x) for x in reads], ins["sites"], ins["reads"]["key"], reads, min_depth=min_depth)
    win = wc.host_windows(reads, ba, qa, ins["sites"], ins["reads"]["key"], min_depth=min_depth)   # the window call's: all carriers of a site vote together
    group, how, ng = regroup(var["key2"], var["mask2"], len(ins["sites"]))
    return dict(frame=frame, exons=exons, reads=reads, planted=planted, base=base, slots=slots, ins=ins, var=var, win=win, group=group, how=how, n_groups=ng,
                keys=group_keys2(group, how, var["key2"], ng))


def host_isoforms(case, min_depth=3):
    """per isoform counted again: (by variant, the parent's splice — ioc_host_isoform_splice of the same tables under the same key2
    over the window call's windows —, the unspliced call): the first as api.isoform_splice_variants returns it, the others sequences"""
    frame, var, n = case["frame"], case["var"], len(case["reads"])
    got = host_isoforms_full_variants([frame], [0] * n, [int(g) for g in case["group"]], [case["n_groups"]], case["base"], case["slots"], case["keys"], [var["win"]],
                                      [var["var"]], [var["seq"]], [var["qual"]], min_depth)
    out = []
    for h in range(case["n_groups"]):
        r0 = int(got["grow0"][h])
        cols, tins = got["gcols"][r0:r0 + len(frame) + 1], got["gins"][r0:r0 + len(frame) + 1]
        parent = api.isoform_splice(cols, tins, frame, int(case["keys"][h]), case["win"]["win"], list(zip(case["win"]["seq"], case["win"]["qual"])), min_depth)[0]
        out.append(((got["gseq"][0][h], got["gqual"][0][h], got["splice"][h], got["sstats"][h]), parent, api.pileup_call(cols, tins, frame, min_depth)[0]))
    return out


def true_of_groups(case):
    """the true isoform of every isoform counted again: the one more than half of its direct reads are of (-1 without).  Not "all of
    them": at 8 % errors a read may miss an exon it holds — at SEED read 21 holds [400, 520) and is keyed as lacking it, a direct read
    of the isoform that lacks both."""
    truth = [x for x, n in enumerate(vc.SIZES) for _ in range(n)]
    out = []
    for h in range(case["n_groups"]):
        mine = [truth[i] for i in range(len(truth)) if int(case["group"][i]) == h and int(case["how"][i]) == api.ISO_DIRECT]
        top = max(set(mine), key=mine.count) if mine else -1
        out.append(top if mine and 2 * mine.count(top) > len(mine) else -1)
    return out


def measure(case, seqs, parents, unspliced, seed=None):
    """per isoform counted again, what PINNED holds"""
    iso = true_transcripts(seed)
    d = lambda s: tuple(ipc.edit_distance(s, t) for t in iso)
    reads = [int(((case["group"] == h)).sum()) for h in range(case["n_groups"])]
    return tuple((int(k), n, x, d(s), d(p), d(u)) for k, n, x, s, p, u in zip(case["keys"], reads, true_of_groups(case), seqs, parents, unspliced))


def property_holds(measured):
    """(four isoforms of four true isoforms; each nearer its own transcript; the carriers' gain over the unspliced call; the gain of
    the isoform with CARRY_B at the first site over the parent's splice)"""
    four = len(measured) == 4 and sorted(m[2] for m in measured) == [0, 1, 2, 3]
    if not four:
        return False, False, False, False
    nearer = all(d[x] < min(d[y] for y in range(4) if y != x) for _, _, x, d, _, _ in measured)
    gained = all(u[x] - d[x] >= carried(x) / 2 for _, _, x, d, _, u in measured if carried(x) > 0)
    b = [m for m in measured if m[0] & 3 == CARRY_B]
    over_parent = len(b) == 1 and all(p[x] - d[x] >= min(vc.EXONS) / 2 for _, _, x, d, p, _ in b)
    return four, nearer, gained, over_parent


def host_measure(seed=None):
    case = host_case(seed)
    iso = host_isoforms(case)
    return case, iso, measure(case, [i[0][0] for i in iso], [i[1] for i in iso], [i[2] for i in iso], seed)
