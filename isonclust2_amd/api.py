"""Python mirror of the host interface of the path (names follow the reference's C++ seam).

Everything here calls the C ABI of libisonclust2_hip.so; numpy arrays are only the carriers of
the flat SoA the ABI takes.  No compute happens in Python and nothing falls back to the CPU.
"""
import ctypes as C
import types

import numpy as np

from . import _lib
from ._lib import BatchView, ClusterStats, IocError, LeftView, Params, Timings

MODE = {"sahlin": 0, "fast": 1, "furious": 2, "none": 3}
TIE_SLOTS = 16                 # keys per query ioc_get_ties returns (IOC_TIE_SLOTS)
CUT_NONE = 2 ** 31 - 1         # ioc_get_cuts of a query without a walk
NO_VERDICT = -2 ** 31          # ioc_set_aln_verdicts: no verdict for this query


def default_params(k=11, w=15, mode="fast"):
    """CmdArgs defaults (src/args.h:9-37) restricted to what the path reads."""
    return Params(k=k, w=w, min_shared=5, mode=MODE[mode], min_fraction=0.8, mapped_threshold=0.65,
                  min_prob_no_hits=0.1, aligned_threshold=0.2)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def host_gap_limits(k, w, min_prob_no_hits=0.1, table=_lib.TABLE_PATH):
    L = _lib.load()
    g = np.zeros(225, np.int32)
    p = np.zeros(225, np.float64)
    rc = L.ioc_host_gap_limits(table.encode(), k, w, min_prob_no_hits, _p(g, C.c_int32), _p(p, C.c_double))
    if rc != 0:
        raise IocError(rc, f"no table rows for k={k}, w={w}")
    return g.reshape(15, 15), p.reshape(15, 15)


def host_err_cell(e):
    return int(_lib.load().ioc_host_err_cell(float(e)))


def host_min_total(hpc_len, thr=0.65):
    return int(_lib.load().ioc_host_min_total(int(hpc_len), float(thr)))


def host_align_ops(query, ref, match=2, mismatch=-2, gap_open=3, gap_extend=1):
    """ioc_host_align_ops: (operation bytes, score) of the host aligner — '=' 'X' 'I' 'D', free end gaps 'i' 'd'."""
    buf, sc = C.create_string_buffer(len(query) + len(ref) + 1), C.c_int32(0)
    n = _lib.load().ioc_host_align_ops(query, len(query), ref, len(ref), match, mismatch, gap_open, gap_extend, buf,
                                       len(query) + len(ref) + 1, C.byref(sc))
    if n < 0:
        raise RuntimeError(f"ioc_host_align_ops failed ({n})")
    return buf.raw[:n], sc.value


def ops_to_cigar(ops):
    """ioc_host_ops_to_cigar: run-length text of an operation string, e.g. b"==X=II" -> "2=1X1=2I"."""
    out = C.create_string_buffer(2 * len(ops) + 1)
    n = _lib.load().ioc_host_ops_to_cigar(bytes(ops), len(ops), out, len(out))
    if n < 0:
        raise ValueError(f"ioc_host_ops_to_cigar failed ({n})")
    return out.raw[:n].decode()


# ioc_aln_stats as a numpy record (Context.align_pairs_stats returns an array of them)
ALN_STATS_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.AlnStats._fields_[:-1]] + [("reserved", np.int32, (2,))])
ALN_STATS_FIELDS = tuple(n for n, _ in _lib.AlnStats._fields_[:-1])


def ops_stats(ops):
    """ioc_host_ops_stats: what an operation string says about its alignment, as a dict — length, columns, matches, mismatches,
    ins, del, ins_runs, del_runs, longest_ins, longest_del and the end gaps lead_i, lead_d, trail_i, trail_d."""
    st = _lib.AlnStats()
    rc = _lib.load().ioc_host_ops_stats(bytes(ops), len(ops), C.byref(st))
    if rc != 0:
        raise ValueError(f"ioc_host_ops_stats failed ({rc})")
    return {n: int(getattr(st, n)) for n in ALN_STATS_FIELDS}


# ioc_pileup_col as a numpy record (ops_pileup and Context.align_pairs_pileup return arrays of them, one per row)
PILEUP_DTYPE = np.dtype([(n, np.uint32) for n, _ in _lib.PileupCol._fields_])
PILEUP_FIELDS = PILEUP_DTYPE.names


def ops_pileup(ops, query, rlen, cols=None):
    """ioc_host_ops_pileup: the pileup of one operation string and its query on a reference of rlen bases — rlen + 1 rows
    (PILEUP_DTYPE), row p what the query says at reference position p, insertions at the position they stand in front of.  ADDED
    to `cols` where given (a contiguous array of rlen + 1 rows, returned), else to a fresh table of zeros.  ValueError, with
    cols untouched, for a byte that is no operation or a string that does not consume exactly len(query) and rlen bases."""
    if cols is None:
        cols = np.zeros(rlen + 1, PILEUP_DTYPE)
    if cols.dtype != PILEUP_DTYPE or cols.shape != (rlen + 1,) or not cols.flags["C_CONTIGUOUS"]:
        raise ValueError("cols must be a contiguous array of rlen + 1 rows of PILEUP_DTYPE")
    rc = _lib.load().ioc_host_ops_pileup(bytes(ops), len(ops), bytes(query), len(query), int(rlen), cols.ctypes.data)
    if rc != 0:
        raise ValueError(f"ioc_host_ops_pileup failed ({rc})")
    return cols


# ioc_pileup_ins / ioc_polish_stats as numpy records
PILEUP_INS_DTYPE = np.dtype([("slot", np.uint32, (_lib.PILE_INS_SLOTS, 5)), ("longer", np.uint32), ("reserved", np.uint32)])
POLISH_STATS_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.PolishStats._fields_[:-1]] + [("reserved", np.int32, (3,))])
POLISH_STATS_FIELDS = tuple(n for n, _ in _lib.PolishStats._fields_[:-1])
PILE_CALL_CHUNK = 256  # rows a workgroup of the call kernels takes per step (IOC_PILE_CALL_CHUNK; the tests place sizes around it)


def pileup_call_bound(rlen):
    """What a consensus call of a reference of rlen bases may write at most: rlen + IOC_PILE_INS_SLOTS * (rlen + 1)."""
    return int(rlen) + _lib.PILE_INS_SLOTS * (int(rlen) + 1)


def ops_pileup_ins(ops, query, rlen, ins=None):
    """ioc_host_ops_pileup_ins: what the 'I' bytes of one operation string insert, by the row they stand in front of, their index
    in their run and the query's base — rlen + 1 rows (PILEUP_INS_DTYPE), ADDED to `ins` where given (returned), else to zeros.
    ValueError, with ins untouched, for what ops_pileup refuses."""
    if ins is None:
        ins = np.zeros(rlen + 1, PILEUP_INS_DTYPE)
    if ins.dtype != PILEUP_INS_DTYPE or ins.shape != (rlen + 1,) or not ins.flags["C_CONTIGUOUS"]:
        raise ValueError("ins must be a contiguous array of rlen + 1 rows of PILEUP_INS_DTYPE")
    rc = _lib.load().ioc_host_ops_pileup_ins(bytes(ops), len(ops), bytes(query), len(query), int(rlen), ins.ctypes.data)
    if rc != 0:
        raise ValueError(f"ioc_host_ops_pileup_ins failed ({rc})")
    return ins


def _tables(cols, ins, n_rows):
    cols, ins = np.ascontiguousarray(cols, PILEUP_DTYPE), np.ascontiguousarray(ins, PILEUP_INS_DTYPE)
    if cols.shape != (n_rows,) or ins.shape != (n_rows,):
        raise ValueError(f"cols and ins must hold {n_rows} rows each")
    return cols, ins


def pileup_call(cols, ins, frame, min_depth=3, cap=None):
    """ioc_host_pileup_call: the majority call of one reference (`frame`, bytes) from its two tables (len(frame) + 1 rows each) —
    returns (sequence, qualities, stats), bytes, bytes and a dict of POLISH_STATS_FIELDS.  IocError for min_depth < 1 and for a
    `cap` (default: the bound) below the bound."""
    rlen = len(frame)
    cols, ins = _tables(cols, ins, rlen + 1)
    cap = pileup_call_bound(rlen) if cap is None else int(cap)
    seq, qual, st = C.create_string_buffer(max(cap, 1)), C.create_string_buffer(max(cap, 1)), _lib.PolishStats()
    n = _lib.load().ioc_host_pileup_call(cols.ctypes.data, ins.ctypes.data, bytes(frame), rlen, int(min_depth), seq, qual, cap, C.byref(st))
    if n < 0:
        raise IocError(int(n), "ioc_host_pileup_call")
    return seq.raw[:n], qual.raw[:n], {f: int(getattr(st, f)) for f in POLISH_STATS_FIELDS}


def qual_weight(b):
    """ioc_host_qual_weight: the weight a quality byte (0 .. 255, as a FASTQ line has it) gives its base in the weighted pileup —
    1 for b <= 34, else min(b - 33, 93)."""
    return int(_lib.load().ioc_host_qual_weight(int(b)))


def ops_pileup_weighted(ops, query, qual, rlen, wcols=None, wins=None):
    """ioc_host_ops_pileup_weighted: the pileup of one operation string by weight — `qual` one quality byte per base of `query`;
    sums of qual_weight ADDED to `wcols` (PILEUP_DTYPE; ins_runs / ins_bases untouched) and `wins` (PILEUP_INS_DTYPE), rlen + 1
    rows each, where given, else to zeros.  Returns (wcols, wins).  ValueError, with both untouched, for what ops_pileup refuses
    and for a `qual` that is not as long as `query`."""
    if wcols is None:
        wcols = np.zeros(rlen + 1, PILEUP_DTYPE)
    if wins is None:
        wins = np.zeros(rlen + 1, PILEUP_INS_DTYPE)
    if wcols.dtype != PILEUP_DTYPE or wcols.shape != (rlen + 1,) or not wcols.flags["C_CONTIGUOUS"]:
        raise ValueError("wcols must be a contiguous array of rlen + 1 rows of PILEUP_DTYPE")
    if wins.dtype != PILEUP_INS_DTYPE or wins.shape != (rlen + 1,) or not wins.flags["C_CONTIGUOUS"]:
        raise ValueError("wins must be a contiguous array of rlen + 1 rows of PILEUP_INS_DTYPE")
    if len(qual) != len(query):
        raise ValueError("qual must hold one byte per base of query")
    rc = _lib.load().ioc_host_ops_pileup_weighted(bytes(ops), len(ops), bytes(query), bytes(qual), len(query), int(rlen), wcols.ctypes.data,
                                                  wins.ctypes.data)
    if rc != 0:
        raise ValueError(f"ioc_host_ops_pileup_weighted failed ({rc})")
    return wcols, wins


def pileup_call_weighted(cols, wcols, wins, frame, min_depth=3, cap=None):
    """ioc_host_pileup_call_weighted: the call of one reference by weight — `cols` (the counts) for the depth gates, `wcols` and
    `wins` (sums of weights) for everything else.  Returns what pileup_call returns."""
    rlen = len(frame)
    cols, wins = _tables(cols, wins, rlen + 1)
    wcols = np.ascontiguousarray(wcols, PILEUP_DTYPE)
    if wcols.shape != (rlen + 1,):
        raise ValueError(f"wcols must hold {rlen + 1} rows")
    cap = pileup_call_bound(rlen) if cap is None else int(cap)
    seq, qual, st = C.create_string_buffer(max(cap, 1)), C.create_string_buffer(max(cap, 1)), _lib.PolishStats()
    n = _lib.load().ioc_host_pileup_call_weighted(cols.ctypes.data, wcols.ctypes.data, wins.ctypes.data, bytes(frame), rlen, int(min_depth),
                                                  seq, qual, cap, C.byref(st))
    if n < 0:
        raise IocError(int(n), "ioc_host_pileup_call_weighted")
    return seq.raw[:n], qual.raw[:n], {f: int(getattr(st, f)) for f in POLISH_STATS_FIELDS}


def ops_project_weights(ops, query, qual, rlen):
    """ioc_host_ops_project_weights: the weight of every vote one read casts, beside its planes — (wbase, wslots): wbase[r] the
    weight (qual_weight, 1 .. 93) of the read's base at row r or of its deletion there (the smaller of its neighbours' weights), 0
    where it does not cover the row; wslots[j, r] the weight of the j-th base of the insertion in front of r, 0 where there is
    none — laid out like ops_project's base and ops_project_ins' slots.  ValueError for what ops_pileup_weighted refuses."""
    if len(qual) != len(query):
        raise ValueError("qual must hold one byte per base of query")
    wbase, wslots = np.full(rlen + 1, 0xEE, np.uint8), np.full((_lib.PILE_INS_SLOTS, rlen + 1), 0xEE, np.uint8)
    rc = _lib.load().ioc_host_ops_project_weights(bytes(ops), len(ops), bytes(query), bytes(qual), len(query), int(rlen), wbase.ctypes.data, wslots.ctypes.data)
    if rc != 0:
        raise ValueError(f"ioc_host_ops_project_weights failed ({rc})")
    return wbase, wslots


def planes_pile_weighted(base, slots, wbase, wslots, wcols=None, wins=None):
    """ioc_host_planes_pile_weighted: one read's planes and weight planes ADDED to the tables of weights `wcols` (PILEUP_DTYPE;
    ins_runs / ins_bases untouched) and `wins` (PILEUP_INS_DTYPE; `longer` untouched), rlen + 1 rows each, where given, else to
    zeros.  Returns (wcols, wins): for a string with at most one insertion run per row what ops_pileup_weighted gives, except that
    `longer` stays 0.  ValueError, with both tables untouched, for a byte neither projection writes."""
    base, slots = np.ascontiguousarray(base, np.uint8), np.ascontiguousarray(slots, np.uint8)
    wbase, wslots = np.ascontiguousarray(wbase, np.uint8), np.ascontiguousarray(wslots, np.uint8)
    if base.ndim != 1 or len(base) < 1 or slots.shape != (_lib.PILE_INS_SLOTS, len(base)) or wbase.shape != base.shape or wslots.shape != slots.shape:
        raise ValueError("base and wbase must hold rlen + 1 bytes, slots and wslots PILE_INS_SLOTS x (rlen + 1)")
    rlen = len(base) - 1
    if wcols is None:
        wcols = np.zeros(rlen + 1, PILEUP_DTYPE)
    if wins is None:
        wins = np.zeros(rlen + 1, PILEUP_INS_DTYPE)
    if wcols.dtype != PILEUP_DTYPE or wcols.shape != (rlen + 1,) or not wcols.flags["C_CONTIGUOUS"]:
        raise ValueError("wcols must be a contiguous array of rlen + 1 rows of PILEUP_DTYPE")
    if wins.dtype != PILEUP_INS_DTYPE or wins.shape != (rlen + 1,) or not wins.flags["C_CONTIGUOUS"]:
        raise ValueError("wins must be a contiguous array of rlen + 1 rows of PILEUP_INS_DTYPE")
    rc = _lib.load().ioc_host_planes_pile_weighted(base.ctypes.data, slots.ctypes.data, wbase.ctypes.data, wslots.ctypes.data, rlen, wcols.ctypes.data,
                                                   wins.ctypes.data)
    if rc != 0:
        raise ValueError(f"ioc_host_planes_pile_weighted failed ({rc})")
    return wcols, wins


# ioc_pile_site as a numpy record, and the allele bytes
PILE_SITE_DTYPE = np.dtype([(n, np.int32) for n in ("row", "kind", "major", "minor")] + [(n, np.uint32) for n in ("depth", "n_major", "n_minor", "reserved")])
ALLELE_DEL, ALLELE_NONE = _lib.ALLELE_DEL, _lib.ALLELE_NONE
SITE_BASE, SITE_INS = _lib.SITE_BASE, _lib.SITE_INS


def pileup_sites_bound(rlen, max_sites):
    """What a site search of a reference of rlen bases may keep at most: min(max_sites, 2 * rlen + 1)."""
    return min(int(max_sites), 2 * int(rlen) + 1)


def ops_project(ops, query, rlen):
    """ioc_host_ops_project: what one read says at every row of its reference — (base, insf), two uint8 arrays of rlen + 1 bytes:
    base[r] the channel 0 .. 4 of the read's base at reference position r, ALLELE_DEL where it deletes it, ALLELE_NONE where it does
    not cover it; insf[r] 1 where it inserts in front of r.  ValueError for what ops_pileup refuses."""
    base, insf = np.full(rlen + 1, 0xEE, np.uint8), np.full(rlen + 1, 0xEE, np.uint8)
    rc = _lib.load().ioc_host_ops_project(bytes(ops), len(ops), bytes(query), len(query), int(rlen), base.ctypes.data, insf.ctypes.data)
    if rc != 0:
        raise ValueError(f"ioc_host_ops_project failed ({rc})")
    return base, insf


def ops_project_ins(ops, query, rlen):
    """ioc_host_ops_project_ins: which bases one read inserts in front of every row of its reference — a uint8 array of shape
    (PILE_INS_SLOTS, rlen + 1), slot-major: slots[j, r] is 1 + the channel (1 .. 5 for A C G T other) of the j-th base of the
    insertion in front of r, 0 where there is none; bases behind the sixth are not kept.  ValueError for what ops_pileup refuses."""
    slots = np.full((_lib.PILE_INS_SLOTS, rlen + 1), 0xEE, np.uint8)
    rc = _lib.load().ioc_host_ops_project_ins(bytes(ops), len(ops), bytes(query), len(query), int(rlen), slots.ctypes.data)
    if rc != 0:
        raise ValueError(f"ioc_host_ops_project_ins failed ({rc})")
    return slots


def planes_pile(base, slots, cols=None, ins=None):
    """ioc_host_planes_pile: one read's planes — `base` as ops_project writes it (rlen + 1 bytes), `slots` as ops_project_ins does
    (PILE_INS_SLOTS x (rlen + 1)) — ADDED to `cols` (PILEUP_DTYPE) and `ins` (PILEUP_INS_DTYPE), rlen + 1 rows each, where given,
    else to zeros.  Returns (cols, ins): for a string with at most one insertion run per row what ops_pileup and ops_pileup_ins
    give, except that ins_bases counts at most PILE_INS_SLOTS per run and `longer` stays 0.  ValueError, with both tables
    untouched, for a byte neither projection writes."""
    base, slots = np.ascontiguousarray(base, np.uint8), np.ascontiguousarray(slots, np.uint8)
    if base.ndim != 1 or len(base) < 1 or slots.shape != (_lib.PILE_INS_SLOTS, len(base)):
        raise ValueError("base must hold rlen + 1 bytes and slots PILE_INS_SLOTS x (rlen + 1)")
    rlen = len(base) - 1
    if cols is None:
        cols = np.zeros(rlen + 1, PILEUP_DTYPE)
    if ins is None:
        ins = np.zeros(rlen + 1, PILEUP_INS_DTYPE)
    if cols.dtype != PILEUP_DTYPE or cols.shape != (rlen + 1,) or not cols.flags["C_CONTIGUOUS"]:
        raise ValueError("cols must be a contiguous array of rlen + 1 rows of PILEUP_DTYPE")
    if ins.dtype != PILEUP_INS_DTYPE or ins.shape != (rlen + 1,) or not ins.flags["C_CONTIGUOUS"]:
        raise ValueError("ins must be a contiguous array of rlen + 1 rows of PILEUP_INS_DTYPE")
    rc = _lib.load().ioc_host_planes_pile(base.ctypes.data, slots.ctypes.data, rlen, cols.ctypes.data, ins.ctypes.data)
    if rc != 0:
        raise ValueError(f"ioc_host_planes_pile failed ({rc})")
    return cols, ins


# ioc_correct_stats as a numpy record
CORRECT_STATS_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.CorrectStats._fields_])
CORRECT_STATS_FIELDS = tuple(n for n, _ in _lib.CorrectStats._fields_)


def read_correct(base, slots, cols, ins, frame, min_depth=3, min_alt=3, min_pct=25, max_run=10, cap=None):
    """ioc_host_read_correct: one read corrected against the pileup of its reference — `base` and `slots` the read's planes as
    ops_project and ops_project_ins give them (len(frame) + 1 bytes, PILE_INS_SLOTS x (len(frame) + 1)), `cols` and `ins` the
    reference's tables (len(frame) + 1 rows each), `frame` the reference (bytes).  A base that at least need(depth) = max(min_alt,
    ceil(min_pct * depth / 100)) reads share is kept, anything else goes to the pileup's winner; runs of more than max_run filled or
    removed rows are left as the read has them.  Returns (sequence, qualities, stats): bytes, bytes and a dict of
    CORRECT_STATS_FIELDS.  IocError for a rule outside its ranges and for a `cap` (default: the bound) below the bound."""
    rlen = len(frame)
    cols, ins = _tables(cols, ins, rlen + 1)
    base, slots = np.ascontiguousarray(base, np.uint8), np.ascontiguousarray(slots, np.uint8)
    if base.shape != (rlen + 1,) or slots.shape != (_lib.PILE_INS_SLOTS, rlen + 1):
        raise ValueError("base must hold len(frame) + 1 bytes and slots PILE_INS_SLOTS x (len(frame) + 1)")
    cap = pileup_call_bound(rlen) if cap is None else int(cap)
    seq, qual, st = C.create_string_buffer(max(cap, 1)), C.create_string_buffer(max(cap, 1)), _lib.CorrectStats()
    n = _lib.load().ioc_host_read_correct(base.ctypes.data, slots.ctypes.data, rlen, cols.ctypes.data, ins.ctypes.data, bytes(frame), int(min_depth),
                                          int(min_alt), int(min_pct), int(max_run), seq, qual, cap, C.byref(st))
    if n < 0:
        raise IocError(int(n), "ioc_host_read_correct")
    return seq.raw[:n], qual.raw[:n], {f: int(getattr(st, f)) for f in CORRECT_STATS_FIELDS}


# ioc_iso_correct_stats as a numpy record
ISO_CORRECT_STATS_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.IsoCorrectStats._fields_])
ISO_CORRECT_STATS_FIELDS = tuple(n for n, _ in _lib.IsoCorrectStats._fields_)


def read_correct_long_bound(rlen, qlen):
    """what ioc_host_read_correct_long asks of cap: read_correct's bound and the read's length"""
    return pileup_call_bound(rlen) + int(qlen)


def read_correct_long(base, slots, ilen, qpos, cols, ins, frame, query, min_depth=3, min_alt=3, min_pct=25, max_run=10, cap=None):
    """ioc_host_read_correct_long: read_correct with a long insertion carried through — `ilen` and `qpos` the read's length and
    position planes as ops_project_ilen and ops_project_qpos give them (len(frame) + 1 entries each), `query` the read (bytes).  A
    row with ilen > PILE_INS_SLOTS emits query[qpos : qpos + ilen] at quality 0 in place of its slot rule; everything else is
    read_correct's.  Returns (sequence, qualities, stats): bytes, bytes and a dict of ISO_CORRECT_STATS_FIELDS; an unresolved pair
    (`flags` & ISOC_UNRESOLVED) comes back empty.  IocError for a rule outside its ranges and for a `cap` (default: the bound)
    below the bound."""
    rlen = len(frame)
    cols, ins = _tables(cols, ins, rlen + 1)
    base, slots = np.ascontiguousarray(base, np.uint8), np.ascontiguousarray(slots, np.uint8)
    ilen, qpos = np.ascontiguousarray(ilen, np.uint8), np.ascontiguousarray(qpos, np.uint32)
    if base.shape != (rlen + 1,) or slots.shape != (_lib.PILE_INS_SLOTS, rlen + 1) or ilen.shape != (rlen + 1,) or qpos.shape != (rlen + 1,):
        raise ValueError("base, ilen and qpos must hold len(frame) + 1 entries and slots PILE_INS_SLOTS x (len(frame) + 1)")
    query = bytes(query)
    cap = read_correct_long_bound(rlen, len(query)) if cap is None else int(cap)
    seq, qual, st = C.create_string_buffer(max(cap, 1)), C.create_string_buffer(max(cap, 1)), _lib.IsoCorrectStats()
    n = _lib.load().ioc_host_read_correct_long(base.ctypes.data, slots.ctypes.data, ilen.ctypes.data, qpos.ctypes.data, rlen, cols.ctypes.data, ins.ctypes.data,
                                               bytes(frame), query, len(query), int(min_depth), int(min_alt), int(min_pct), int(max_run), seq, qual, cap,
                                               C.byref(st))
    if n < 0:
        raise IocError(int(n), "ioc_host_read_correct_long")
    return seq.raw[:n], qual.raw[:n], {f: int(getattr(st, f)) for f in ISO_CORRECT_STATS_FIELDS}


# ioc_block_row, ioc_pile_block, ioc_read_blocks and ioc_blocks_seg as numpy records
BLOCK_ROW_DTYPE = np.dtype([("depth", np.uint32), ("in_gap", np.uint32)])
PILE_BLOCK_DTYPE = np.dtype([("first", np.int32), ("end", np.int32)] + [(n, np.uint32) for n in ("n_keep", "n_skip", "n_part", "n_none")] + [("reserved", np.uint32, 2)])
READ_BLOCKS_DTYPE = np.dtype([("key", np.uint64)] + [(n, np.int32) for n in ("group", "how", "first_row", "end_row", "n_gaps", "gap_rows")])
BLOCKS_SEG_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.BlocksSeg._fields_])
BLOCK_KEEP, BLOCK_SKIP, BLOCK_PART, BLOCK_NONE = _lib.BLOCK_KEEP, _lib.BLOCK_SKIP, _lib.BLOCK_PART, _lib.BLOCK_NONE
ISO_DIRECT, ISO_ASSIGNED, ISO_RARE, ISO_AMBIGUOUS = _lib.ISO_DIRECT, _lib.ISO_ASSIGNED, _lib.ISO_RARE, _lib.ISO_AMBIGUOUS
BLOCKS_RULE = dict(min_gap=20, min_depth=3, min_alt=3, min_pct=25, min_block=10, max_blocks=32)


def planes_blocks_bound(rlen, max_blocks):
    """What a block search of a reference of rlen bases may keep at most: min(max_blocks, rlen)."""
    return min(int(max_blocks), int(rlen))


def blocks_polish_bound(rlen, n_reads, max_iso):
    """What the isoform consensus of a block search may call at most of a reference of rlen bases with n_reads reads: (isoforms,
    bytes) — a segment has at most as many isoforms as reads, so min(max_iso, n_reads) of them, pileup_call_bound(rlen) bytes each.
    align_pairs_blocks_polish asks the sums over the segments of iso_cap and cap."""
    most = min(int(max_iso), int(n_reads))
    return most, most * pileup_call_bound(rlen)


def _blocks_rule(rule):
    unknown = set(rule) - set(BLOCKS_RULE)
    if unknown:
        raise TypeError(f"unknown rule parameters: {sorted(unknown)}")
    return [int({**BLOCKS_RULE, **rule}[n]) for n in BLOCKS_RULE]


def planes_blocks(base, rows=True, **rule):
    """ioc_host_planes_blocks: the exon blocks of one segment and every read's isoform — `base` the reads' base planes as ops_project
    gives them, n_reads x (rlen + 1) bytes; the rule as keywords (BLOCKS_RULE has the defaults).  A long gap is a run of at least
    min_gap deleted rows; a row is variable where enough reads have one and enough have none; a block is a run of at least
    min_block variable rows; a read's state at a block is keep, skip, part or none, its key the states two bits each, and the keys
    that at least min_alt complete reads carry are the isoforms, in ascending order.  Returns a dict: `rows` (BLOCK_ROW_DTYPE, rlen +
    1 rows; with rows=True), `blocks` (PILE_BLOCK_DTYPE, the kept ones), `reads` (READ_BLOCKS_DTYPE per read), `seg` (a
    BLOCKS_SEG_DTYPE record).  IocError for a rule outside its ranges."""
    base = np.ascontiguousarray(base, np.uint8)
    if base.ndim != 2 or base.shape[1] < 1:
        raise ValueError("base must hold n_reads x (rlen + 1) bytes")
    n, rlen = base.shape[0], base.shape[1] - 1
    r = _blocks_rule(rule)
    tab = np.zeros(rlen + 1, BLOCK_ROW_DTYPE)
    blocks, reads, seg = np.zeros(max(min(max(r[5], 0), rlen), 1), PILE_BLOCK_DTYPE), np.zeros(n, READ_BLOCKS_DTYPE), np.zeros(1, BLOCKS_SEG_DTYPE)
    rc = _lib.load().ioc_host_planes_blocks(base.ctypes.data if n else None, n, rlen, *r, tab.ctypes.data if rows else None, blocks.ctypes.data,
                                            reads.ctypes.data if n else None, seg.ctypes.data)
    if rc < 0:
        raise IocError(int(rc), "ioc_host_planes_blocks")
    out = {"blocks": blocks[:int(seg[0]["n_blocks"])], "reads": reads, "seg": seg[0]}
    if rows:
        out["rows"] = tab
    return out


def ops_project_ilen(ops, rlen):
    """ioc_host_ops_project_ilen: how many bases one read inserts in front of every row of its reference — a uint8 array of rlen + 1
    bytes: ilen[r] = min(n, 255) for the run of n 'I' in front of row r, 0 elsewhere; free-end 'i' bytes count for nothing.
    ValueError for a byte outside "=XIDid" and for a string that does not consume rlen reference bases."""
    ilen = np.full(int(rlen) + 1, 0xEE, np.uint8)
    rc = _lib.load().ioc_host_ops_project_ilen(bytes(ops), len(ops), int(rlen), ilen.ctypes.data)
    if rc != 0:
        raise ValueError(f"ioc_host_ops_project_ilen failed ({rc})")
    return ilen


# ioc_insert_row, ioc_pile_insert, ioc_read_inserts and ioc_inserts_seg as numpy records
INSERT_ROW_DTYPE = np.dtype([("span", np.uint32), ("in_ins", np.uint32)])
PILE_INSERT_DTYPE = np.dtype([("first", np.int32), ("end", np.int32)] + [(n, np.uint32) for n in ("n_carry", "n_lack", "n_none", "len_min", "len_max", "reserved")])
READ_INSERTS_DTYPE = np.dtype([("key", np.uint64)] + [(n, np.int32) for n in ("group", "how", "n_near", "ins_bases")] + [("reserved", np.uint32, 2)])
INSERTS_SEG_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.InsertsSeg._fields_])
INS_LACK, INS_CARRY, INS_NONE = _lib.INS_LACK, _lib.INS_CARRY, _lib.INS_NONE
# (20 bases within 8 junctions: choices made on simulated reads, not measured on real data)
INSERTS_RULE = dict(min_ins=20, slack=8, min_depth=3, min_alt=3, min_pct=25, max_sites=32)


def planes_inserts_bound(rlen, max_sites):
    """What a search for insertion sites of a reference of rlen bases may keep at most: min(max_sites, max(rlen - 1, 0))."""
    return min(int(max_sites), max(int(rlen) - 1, 0))


def _inserts_rule(rule):
    unknown = set(rule) - set(INSERTS_RULE)
    if unknown:
        raise TypeError(f"unknown rule parameters: {sorted(unknown)}")
    return [int({**INSERTS_RULE, **rule}[n]) for n in INSERTS_RULE]


def planes_inserts(base, ilen, pre_key=None, pre_mask=None, pre_full=0, rows=True, **rule):
    """ioc_host_planes_inserts: the insertion sites of one segment and every read's combined isoform — `base` and `ilen` the reads'
    base planes and length planes as ops_project and ops_project_ilen give them, n_reads x (rlen + 1) bytes each; the rule as
    keywords (INSERTS_RULE has the defaults).  A read spans a junction where it covers the rows on both sides, and is near an
    insertion there where its inserted bases within `slack` junctions sum to min_ins; a junction is variable where enough spanning
    reads are near one and enough are not; a site is a run of variable junctions; a read's state at a site is carry, lack or none.
    pre_key / pre_mask (per read) and pre_full: the block stage's keys, masks and complete mask, with which the isoforms are counted
    over blocks and sites together; without them the sites alone.  Returns a dict: `rows` (INSERT_ROW_DTYPE, rlen + 1 rows; with
    rows=True), `sites` (PILE_INSERT_DTYPE, the kept ones), `reads` (READ_INSERTS_DTYPE per read), `seg` (an INSERTS_SEG_DTYPE
    record).  IocError for a rule outside its ranges."""
    base, ilen = np.ascontiguousarray(base, np.uint8), np.ascontiguousarray(ilen, np.uint8)
    if base.ndim != 2 or base.shape[1] < 1 or ilen.shape != base.shape:
        raise ValueError("base and ilen must hold n_reads x (rlen + 1) bytes each")
    n, rlen = base.shape[0], base.shape[1] - 1
    if (pre_key is None) != (pre_mask is None):
        raise ValueError("pre_key and pre_mask: both or neither")
    pk = pm = None
    if pre_key is not None:
        pk, pm = np.ascontiguousarray(pre_key, np.uint64), np.ascontiguousarray(pre_mask, np.uint64)
        if pk.shape != (n,) or pm.shape != (n,):
            raise ValueError("pre_key and pre_mask must hold one word per read")
    r = _inserts_rule(rule)
    tab = np.zeros(rlen + 1, INSERT_ROW_DTYPE)
    sites, reads, seg = np.zeros(max(planes_inserts_bound(rlen, max(r[5], 0)), 1), PILE_INSERT_DTYPE), np.zeros(n, READ_INSERTS_DTYPE), np.zeros(1, INSERTS_SEG_DTYPE)
    rc = _lib.load().ioc_host_planes_inserts(base.ctypes.data if n else None, ilen.ctypes.data if n else None, n, rlen, *r,
                                             pk.ctypes.data if pk is not None and n else None, pm.ctypes.data if pm is not None and n else None,
                                             int(pre_full) if pk is not None else 0, tab.ctypes.data if rows else None, sites.ctypes.data,
                                             reads.ctypes.data if n else None, seg.ctypes.data)
    if rc < 0:
        raise IocError(int(rc), "ioc_host_planes_inserts")
    out = {"sites": sites[:int(seg[0]["n_sites"])], "reads": reads, "seg": seg[0]}
    if rows:
        out["rows"] = tab
    return out


# ioc_read_extent, ioc_end_site, ioc_end_variant, ioc_read_ends, ioc_ends_seg and ioc_end_row as numpy records
READ_EXTENT_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.ReadExtent._fields_])
END_SITE_DTYPE = np.dtype([("first", np.int32), ("end", np.int32), ("n_reads", np.uint32), ("n_over", np.uint32), ("peak_row", np.int32),
                           ("peak_reads", np.uint32), ("kind", np.int32), ("reserved", np.uint32)])
END_VARIANT_DTYPE = np.dtype([(n, np.int32) for n in ("pre_group", "start_site", "stop_site")] + [("n_reads", np.uint32)])
READ_ENDS_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.ReadEnds._fields_])
ENDS_SEG_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.EndsSeg._fields_])
END_ROW_DTYPE = np.dtype([(n, np.uint32) for n, _ in _lib.EndRow._fields_])
END_START, END_STOP = _lib.END_START, _lib.END_STOP
# (ends within 10 rows of each other, 20 bases beyond the representative, a tenth of the reads: choices made on simulated reads, not
# measured on real data)
ENDS_RULE = dict(slack=10, min_over=20, min_depth=3, min_alt=3, min_pct=10, max_sites=32, max_variants=64)


def reads_ends_bound(rlen, n_reads, max_sites=ENDS_RULE["max_sites"], max_variants=ENDS_RULE["max_variants"]):
    """What a search for ends may keep at most of a reference of rlen bases with n_reads reads: (sites, variants) — min(max_sites,
    rlen + 1) start sites and as many stop sites, min(max_variants, n_reads) variants.  Context.reads_ends and
    Context.align_pairs_blocks_ends ask the sums over the segments of sites_cap and variants_cap."""
    return 2 * min(int(max_sites), int(rlen) + 1), min(int(max_variants), int(n_reads))


def _ends_rule(rule):
    unknown = set(rule) - set(ENDS_RULE)
    if unknown:
        raise TypeError(f"unknown rule parameters: {sorted(unknown)}")
    return [int({**ENDS_RULE, **rule}[n]) for n in ENDS_RULE]


def host_ops_extent(ops, rlen):
    """ioc_host_ops_extent: the extent of one read on its reference from its operation string — a READ_EXTENT_DTYPE record:
    first_row / end_row the first row its base plane covers and one past the last ((0, 0): none), head / tail the free-end 'i' bytes
    before and behind the walk.  ValueError for a byte outside "=XIDid" and for a string that does not consume rlen reference bases."""
    e = _lib.ReadExtent(-0x11111112, -0x11111112, -0x11111112, -0x11111112)
    rc = _lib.load().ioc_host_ops_extent(bytes(ops), len(ops), int(rlen), C.byref(e))
    if rc != 0:
        raise ValueError(f"ioc_host_ops_extent failed ({rc})")
    return np.array([(e.first_row, e.end_row, e.head, e.tail)], READ_EXTENT_DTYPE)[0]


def _extents(extents):
    ext = np.ascontiguousarray(extents, READ_EXTENT_DTYPE)
    if ext.ndim != 1:
        raise ValueError("extents must hold one READ_EXTENT_DTYPE record per read")
    return ext


def host_reads_ends(extents, rlen, pre_group=None, rows=True, **rule):
    """ioc_host_reads_ends: the alternative ends of one segment — `extents` a READ_EXTENT_DTYPE record per read (host_ops_extent),
    rlen the reference's length, pre_group (optional, >= -1 per read) the isoform of an earlier stage; the rule as keywords
    (ENDS_RULE has the defaults).  A row is a start row where at least need(N) of the N reads that cover anything start within
    `slack` rows of it; a start site is a run of start rows, a read's start site the nearest within `slack`; stop sites likewise; the
    (pre_group, start site, stop site) triples that at least min_alt reads carry are the variants, in ascending order.  Returns a
    dict: `starts` and `stops` (END_SITE_DTYPE, the kept ones), `variants` (END_VARIANT_DTYPE), `reads` (READ_ENDS_DTYPE per read),
    `seg` (an ENDS_SEG_DTYPE record) and, with rows=True, `rows` (END_ROW_DTYPE, rlen + 1 rows).  IocError for a rule, an extent or
    a pre_group outside its range."""
    ext = _extents(extents)
    n, rlen = len(ext), int(rlen)
    pg = None
    if pre_group is not None:
        pg = np.ascontiguousarray(pre_group, np.int32)
        if pg.shape != (n,):
            raise ValueError("pre_group must hold one entry per read")
    r = _ends_rule(rule)
    most_s, most_v = reads_ends_bound(max(rlen, 0), n, max(r[5], 0), max(r[6], 0))
    tab = np.zeros(max(rlen, 0) + 1, END_ROW_DTYPE)
    starts, stops = np.zeros(max(most_s // 2, 1), END_SITE_DTYPE), np.zeros(max(most_s // 2, 1), END_SITE_DTYPE)
    variants, reads, seg = np.zeros(max(most_v, 1), END_VARIANT_DTYPE), np.zeros(n, READ_ENDS_DTYPE), np.zeros(1, ENDS_SEG_DTYPE)
    rc = _lib.load().ioc_host_reads_ends(ext.ctypes.data if n else None, pg.ctypes.data if pg is not None and n else None, n, rlen, *r,
                                         tab.ctypes.data if rows else None, starts.ctypes.data, stops.ctypes.data, variants.ctypes.data,
                                         reads.ctypes.data if n else None, seg.ctypes.data)
    if rc < 0:
        raise IocError(int(rc), "ioc_host_reads_ends")
    out = {"starts": starts[:int(seg[0]["n_starts"])], "stops": stops[:int(seg[0]["n_stops"])], "variants": variants[:int(seg[0]["n_variants"])],
           "reads": reads, "seg": seg[0]}
    if rows:
        out["rows"] = tab
    return out


def ops_project_qpos(ops, rlen):
    """ioc_host_ops_project_qpos: where every row of the reference lies in the read — a uint32 array of rlen + 1 words: qpos[0] = 0,
    qpos[r] the bytes of "=XIi" up to and including the byte that consumes row r - 1, so that the run of 'I' in front of row r
    begins at query[qpos[r]].  ValueError for what ops_project_ilen refuses."""
    qpos = np.full(int(rlen) + 1, 0xEEEEEEEE, np.uint32)
    rc = _lib.load().ioc_host_ops_project_qpos(bytes(ops), len(ops), int(rlen), qpos.ctypes.data)
    if rc != 0:
        raise ValueError(f"ioc_host_ops_project_qpos failed ({rc})")
    return qpos


# ioc_insert_window as a numpy record, and what a window call is run with where nothing else is said: the insert stage's slack, the
# aligner's match and mismatch, and a gap that costs what a mismatch does
INSERT_WINDOW_DTYPE = np.dtype([(n, np.int32) for n in ("lo", "hi", "template_pair", "tlen")] + [(n, np.uint32) for n in ("n_voters", "n_short", "n_long", "reserved")])
WIN_MAX = _lib.WIN_MAX
WIN_NONE, WIN_VOTER, WIN_SHORT, WIN_LONG = _lib.WIN_NONE, _lib.WIN_VOTER, _lib.WIN_SHORT, _lib.WIN_LONG
WINDOWS_RULE = dict(slack=INSERTS_RULE["slack"], max_win=WIN_MAX, match=2, mismatch=-2, gap=2)


def align_global_ops(query, ref, match=2, mismatch=-2, gap=2):
    """ioc_host_align_global_ops: the global alignment of two short strings, both ends anchored, linear gaps — (ops, score), ops the
    bytes "=XID" in forward order.  The walk prefers the diagonal, then 'D' (a reference base alone), then 'I': the tie order is
    part of the definition.  IocError for a negative gap, a parameter above 2^20 and strings of more than 2^26 cells."""
    query, ref = bytes(query), bytes(ref)
    ops, score = np.zeros(max(len(query) + len(ref), 1), np.uint8), C.c_int32(0)
    n = _lib.load().ioc_host_align_global_ops(query, len(query), ref, len(ref), int(match), int(mismatch), int(gap), ops.ctypes.data, len(query) + len(ref),
                                              C.byref(score))
    if n < 0:
        raise IocError(int(n), "ioc_host_align_global_ops")
    return ops[:n].tobytes(), int(score.value)


def insert_windows_bound(n_sites, max_win=WIN_MAX):
    """What the windows of n_sites sites may call at most, in bytes of sequence (and of qualities): n_sites (7 max_win + 6).  For the
    fused call n_sites is the sum over the segments of planes_inserts_bound(rlen, max_sites): known before the call."""
    return int(n_sites) * pileup_call_bound(int(max_win))


def insert_windows(base, qpos, qlen, sites, keys, slack=WINDOWS_RULE["slack"], max_win=WIN_MAX):
    """ioc_host_insert_windows: the windows of one segment's carriers at its kept sites — `base` / `qpos` the reads' base planes and
    position planes (n_reads x (rlen + 1)), qlen the reads' lengths, `sites` and `keys` as planes_inserts returned them.  Returns a
    dict: `win` (INSERT_WINDOW_DTYPE per site; template_pair is the read), `cls` (n_reads x n_sites bytes, WIN_*), `start` and `len`
    (where a voter's window begins in its read and how long it is)."""
    base, qpos = np.ascontiguousarray(base, np.uint8), np.ascontiguousarray(qpos, np.uint32)
    if base.ndim != 2 or base.shape[1] < 1 or qpos.shape != base.shape:
        raise ValueError("base and qpos must hold n_reads x (rlen + 1) entries each")
    n, rlen = base.shape[0], base.shape[1] - 1
    ql, ky, st = np.ascontiguousarray(qlen, np.int32), np.ascontiguousarray(keys, np.uint64), np.ascontiguousarray(sites, PILE_INSERT_DTYPE)
    if ql.shape != (n,) or ky.shape != (n,) or st.ndim != 1:
        raise ValueError("qlen and keys must hold one entry per read")
    S = len(st)
    win = np.zeros(max(S, 1), INSERT_WINDOW_DTYPE)
    cls, start, ln = np.zeros((n, S), np.uint8), np.zeros((n, S), np.uint32), np.zeros((n, S), np.uint32)
    rc = _lib.load().ioc_host_insert_windows(base.ctypes.data if n else None, qpos.ctypes.data if n else None, ql.ctypes.data if n else None, n, rlen,
                                             st.ctypes.data if S else None, S, ky.ctypes.data if n else None, int(slack), int(max_win), win.ctypes.data,
                                             cls.ctypes.data if cls.size else None, start.ctypes.data if cls.size else None, ln.ctypes.data if cls.size else None)
    if rc < 0:
        raise IocError(int(rc), "ioc_host_insert_windows")
    return {"win": win[:S], "cls": cls, "start": start, "len": ln}


# ioc_window_variant / ioc_read_variants / ioc_variants_seg as numpy records, and the rule of a variant call beside the window rule:
# min_agree 45 is a choice made on simulated windows (8 % errors, exons of 45 bases and more), not measured on real data
WINDOW_VARIANT_DTYPE = np.dtype([(n, np.int32) for n in ("split", "template_pair_b", "tlen_b")] + [(n, np.uint32) for n in ("n_a", "n_b", "n_other", "n_far", "reserved")])
READ_VARIANTS_DTYPE = np.dtype([("key2", np.uint64), ("group", np.int32), ("how", np.int32)])
VARIANTS_SEG_DTYPE = np.dtype([(n, np.int32) for n in ("n_sites", "n_split", "n_groups", "n_reads", "n_direct", "n_assigned", "n_rare", "n_ambiguous")])
INS_CARRY_B = _lib.INS_CARRY_B
WINVAR_NONE, WINVAR_A, WINVAR_B, WINVAR_OTHER = _lib.WINVAR_NONE, _lib.WINVAR_A, _lib.WINVAR_B, _lib.WINVAR_OTHER
VARIANTS_RULE = dict(min_agree=_lib.WINVAR_MIN_AGREE, min_alt=INSERTS_RULE["min_alt"], min_pct=INSERTS_RULE["min_pct"])
NO_AGREEMENT = -2 ** 31


def ops_agreement(ops):
    """ioc_host_ops_agreement: #'=' - #'X' - #'D' - #'I' over the bytes of an alignment ('i' and 'd' count for nothing).  ValueError
    for a byte outside "=XIDid"."""
    out = C.c_int32(0)
    rc = _lib.load().ioc_host_ops_agreement(bytes(ops), len(ops), C.byref(out))
    if rc != 0:
        raise ValueError(f"ioc_host_ops_agreement failed ({rc})")
    return int(out.value)


def key_isoforms(key, mask, full, min_alt, pre_key=None, pre_mask=None, pre_full=0):
    """ioc_host_key_isoforms: the isoforms of a segment's reads from two-word keys (step 9 of ioc_host_planes_inserts) — (group, how,
    counts), counts a dict of n_groups, n_direct, n_assigned, n_rare and n_ambiguous."""
    ky, mk = np.ascontiguousarray(key, np.uint64), np.ascontiguousarray(mask, np.uint64)
    n = len(ky)
    if mk.shape != (n,) or (pre_key is None) != (pre_mask is None):
        raise ValueError("key and mask must hold one entry per read; pre_key and pre_mask: both or neither")
    pk = None if pre_key is None else np.ascontiguousarray(pre_key, np.uint64)
    pm = None if pre_mask is None else np.ascontiguousarray(pre_mask, np.uint64)
    if pk is not None and (pk.shape != (n,) or pm.shape != (n,)):
        raise ValueError("pre_key and pre_mask must hold one entry per read")
    group, how, counts = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(5, np.int32)
    pad = lambda a: None if a is None else np.concatenate([a, np.zeros(1, a.dtype)])
    ky, mk, pk, pm = pad(ky), pad(mk), pad(pk), pad(pm)
    rc = _lib.load().ioc_host_key_isoforms(pk.ctypes.data if pk is not None else None, pm.ctypes.data if pm is not None else None, int(pre_full),
                                           ky.ctypes.data, mk.ctypes.data, int(full), n, int(min_alt), group.ctypes.data, how.ctypes.data, counts.ctypes.data)
    if rc < 0:
        raise IocError(int(rc), "ioc_host_key_isoforms")
    return group[:n], how[:n], dict(zip(("n_groups", "n_direct", "n_assigned", "n_rare", "n_ambiguous"), (int(x) for x in counts)))


def insert_window_variants_bound(n_sites, max_win=WIN_MAX):
    """What the variants of n_sites sites may call at most, in bytes of sequence (and of qualities): two slots a site."""
    return 2 * insert_windows_bound(n_sites, max_win)


def _variants_rule(rule):
    unknown = set(rule) - set(WINDOWS_RULE) - set(VARIANTS_RULE)
    if unknown:
        raise TypeError(f"unknown rule parameters: {sorted(unknown)}")
    return [int({**WINDOWS_RULE, **rule}[n]) for n in WINDOWS_RULE], [int({**VARIANTS_RULE, **rule}[n]) for n in VARIANTS_RULE]


def insert_window_variants(base, qpos, qlen, sites, keys, reads, min_depth=3, call=True, cap=None, **rule):
    """ioc_host_insert_window_variants: the variants of one segment's kept sites — insert_windows' inputs, `reads` the reads' bytes (a
    list), slack, max_win, match, mismatch, gap, min_agree, min_alt and min_pct as keywords (WINDOWS_RULE and VARIANTS_RULE have the
    defaults).  Returns a dict: `win` (INSERT_WINDOW_DTYPE), `var` (WINDOW_VARIANT_DTYPE), `variant` (n_reads x n_sites bytes,
    WINVAR_*), `agree` (n_reads x n_sites x 2, NO_AGREEMENT where a round did not align the read), `key2`, `mask2` and, with call=True,
    `seq` / `qual` (2 n_sites slots: 2 x is site x's variant A, 2 x + 1 its B), `off` and `polish`."""
    w, v = _variants_rule(rule)
    base, qpos = np.ascontiguousarray(base, np.uint8), np.ascontiguousarray(qpos, np.uint32)
    if base.ndim != 2 or base.shape[1] < 1 or qpos.shape != base.shape:
        raise ValueError("base and qpos must hold n_reads x (rlen + 1) entries each")
    n, rlen = base.shape[0], base.shape[1] - 1
    ql, ky, st = np.ascontiguousarray(qlen, np.int32), np.ascontiguousarray(keys, np.uint64), np.ascontiguousarray(sites, PILE_INSERT_DTYPE)
    if ql.shape != (n,) or ky.shape != (n,) or st.ndim != 1 or len(reads) != n:
        raise ValueError("qlen, keys and reads must hold one entry per read")
    S = len(st)
    blob = b"".join(bytes(r) for r in reads) + b"\0"
    roff = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    cap = insert_window_variants_bound(S, w[1]) if cap is None else int(cap)
    win, var = np.zeros(max(S, 1), INSERT_WINDOW_DTYPE), np.zeros(max(S, 1), WINDOW_VARIANT_DTYPE)
    variant, agree = np.zeros((n, S), np.uint8), np.zeros((n, S, 2), np.int32)
    seq, qual = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint8)
    off, pol = np.zeros(2 * S + 1, np.int64), np.zeros(max(2 * S, 1), POLISH_STATS_DTYPE)
    key2, mask2 = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
    pad = lambda a: np.concatenate([a.reshape(-1), np.zeros(1, a.dtype)])  # (never an empty array's pointer)
    fb, fq, ql, ky, st, variant_f, agree_f = (pad(x) for x in (base, qpos, ql, ky, st, variant, agree))
    rc = _lib.load().ioc_host_insert_window_variants(fb.ctypes.data, fq.ctypes.data, ql.ctypes.data, n, rlen, st.ctypes.data, S, ky.ctypes.data, blob,
                                                     roff.ctypes.data, *w, int(min_depth), *v, win.ctypes.data, var.ctypes.data, variant_f.ctypes.data,
                                                     agree_f.ctypes.data, seq.ctypes.data if call else None, qual.ctypes.data if call else None, cap,
                                                     off.ctypes.data, pol.ctypes.data, key2.ctypes.data, mask2.ctypes.data)
    if rc < 0:
        raise IocError(int(rc), "ioc_host_insert_window_variants")
    out = {"win": win[:S], "var": var[:S], "variant": variant_f[:-1].reshape(n, S), "agree": agree_f[:-1].reshape(n, S, 2), "key2": key2[:n], "mask2": mask2[:n]}
    if call:
        out.update(seq=[seq[off[x]:off[x + 1]].tobytes() for x in range(2 * S)], qual=[qual[off[x]:off[x + 1]].tobytes() for x in range(2 * S)], off=off,
                   polish=pol[:2 * S])
    return out


# ioc_splice_site / ioc_splice_stats as numpy records
SPLICE_SITE_DTYPE = np.dtype([(n, np.int32) for n in ("state", "at", "len", "reserved")])
SPLICE_STATS_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.SpliceStats._fields_[:-1]] + [("reserved", np.int32, (3,))])
SPLICE_STATS_FIELDS = tuple(n for n, _ in _lib.SpliceStats._fields_[:-1])
SPLICE_LACK, SPLICE_DONE, SPLICE_UNCALLED, SPLICE_OVERLAP = _lib.SPLICE_LACK, _lib.SPLICE_DONE, _lib.SPLICE_UNCALLED, _lib.SPLICE_OVERLAP


def isoform_splice_bound(rlen, win_bytes):
    """What the full-length sequence of one isoform may hold at most: the call's bound of its segment plus the bytes of the segment's
    windows."""
    return pileup_call_bound(rlen) + int(win_bytes)


def isoforms_full_bound(rlen, n_reads, max_iso, max_sites=INSERTS_RULE["max_sites"], max_win=WIN_MAX):
    """What the fused call may write, known before it runs — (bytes of sequence, group-segments, site records) over segments of rlen[g]
    bases and n_reads[g] reads: an isoform of segment g holds at most the call's bound plus min(max_sites, max(rlen - 1, 0)) windows of
    7 max_win + 6 bytes each.  A caller keeps it small with max_sites and max_win as the data allow, and with batches of segments."""
    iso = [min(int(max_iso), int(m)) for m in n_reads]
    sites = [planes_inserts_bound(m, max_sites) for m in rlen]
    return (sum(k * isoform_splice_bound(m, s * pileup_call_bound(max_win)) for k, m, s in zip(iso, rlen, sites)), sum(iso),
            sum(k * s for k, s in zip(iso, sites)))


def isoform_splice(cols, ins, frame, key, win, win_seq, min_depth=3, cap=None):
    """ioc_host_isoform_splice: the full-length sequence of one isoform — pileup_call over its tables with, for every site its key
    carries (`key`: the insert key of its direct reads), the site's called window in place of the rows [lo, hi) it stands for.  `win`:
    the segment's INSERT_WINDOW_DTYPE records; win_seq: a (sequence, qualities) pair of bytes per site.  Returns (sequence,
    qualities, stats, sites, sstats): stats a dict of POLISH_STATS_FIELDS, sites a SPLICE_SITE_DTYPE array (state, and for a DONE site
    where its window begins in the sequence and how long it is), sstats a dict of SPLICE_STATS_FIELDS.  IocError for what the
    definition refuses."""
    rlen = len(frame)
    cols, ins = _tables(cols, ins, rlen + 1)
    w = np.ascontiguousarray(win, INSERT_WINDOW_DTYPE)
    S = len(w)
    if len(win_seq) != S or any(len(s) != len(q) for s, q in win_seq):
        raise ValueError("win_seq must hold a (sequence, qualities) pair of equal lengths per site")
    woff = np.concatenate([[0], np.cumsum([len(s) for s, _ in win_seq])]).astype(np.int64)
    wseq, wqual = b"".join(bytes(s) for s, _ in win_seq), b"".join(bytes(q) for _, q in win_seq)
    cap = isoform_splice_bound(rlen, woff[-1]) if cap is None else int(cap)
    seq, qual, st, ss = C.create_string_buffer(max(cap, 1)), C.create_string_buffer(max(cap, 1)), _lib.PolishStats(), _lib.SpliceStats()
    rec = np.full(max(S, 1), -7, SPLICE_SITE_DTYPE)
    n = _lib.load().ioc_host_isoform_splice(cols.ctypes.data, ins.ctypes.data, bytes(frame), rlen, int(min_depth), int(key), w.ctypes.data if S else None, S,
                                            wseq, wqual, woff.ctypes.data, seq, qual, cap, C.byref(st), rec.ctypes.data, C.byref(ss))
    if n < 0:
        raise IocError(int(n), "ioc_host_isoform_splice")
    return (seq.raw[:n], qual.raw[:n], {f: int(getattr(st, f)) for f in POLISH_STATS_FIELDS}, rec[:S],
            {f: int(getattr(ss, f)) for f in SPLICE_STATS_FIELDS})


def isoform_splice_variants(cols, ins, frame, key2, win, var, slot_seq, min_depth=3, cap=None):
    """ioc_host_isoform_splice_variants: isoform_splice by variant — `key2` a read's second key (READ_VARIANTS_DTYPE), `var` the
    segment's WINDOW_VARIANT_DTYPE records beside `win`, slot_seq a (sequence, qualities) pair of bytes per SLOT, 2 b site b's variant
    A and 2 b + 1 its B, as insert_window_variants returns them.  A site whose state is INS_CARRY takes slot 2 b, one whose state is
    INS_CARRY_B slot 2 b + 1 (UNCALLED where the site did not split).  Returns what isoform_splice returns."""
    rlen = len(frame)
    cols, ins = _tables(cols, ins, rlen + 1)
    w, v = np.ascontiguousarray(win, INSERT_WINDOW_DTYPE), np.ascontiguousarray(var, WINDOW_VARIANT_DTYPE)
    S = len(w)
    if len(v) != S or len(slot_seq) != 2 * S or any(len(s) != len(q) for s, q in slot_seq):
        raise ValueError("var must hold a record per site and slot_seq a (sequence, qualities) pair of equal lengths per slot, two a site")
    soff = np.concatenate([[0], np.cumsum([len(s) for s, _ in slot_seq])]).astype(np.int64)
    sseq, squal = b"".join(bytes(s) for s, _ in slot_seq), b"".join(bytes(q) for _, q in slot_seq)
    cap = isoform_splice_bound(rlen, soff[-1]) if cap is None else int(cap)
    seq, qual, st, ss = C.create_string_buffer(max(cap, 1)), C.create_string_buffer(max(cap, 1)), _lib.PolishStats(), _lib.SpliceStats()
    rec = np.full(max(S, 1), -7, SPLICE_SITE_DTYPE)
    n = _lib.load().ioc_host_isoform_splice_variants(cols.ctypes.data, ins.ctypes.data, bytes(frame), rlen, int(min_depth), int(key2), w.ctypes.data if S else None,
                                                     v.ctypes.data if S else None, S, sseq, squal, soff.ctypes.data, seq, qual, cap, C.byref(st), rec.ctypes.data,
                                                     C.byref(ss))
    if n < 0:
        raise IocError(int(n), "ioc_host_isoform_splice_variants")
    return (seq.raw[:n], qual.raw[:n], {f: int(getattr(st, f)) for f in POLISH_STATS_FIELDS}, rec[:S],
            {f: int(getattr(ss, f)) for f in SPLICE_STATS_FIELDS})


def pileup_sites(cols, min_depth=3, min_alt=3, min_pct=25, max_sites=4096):
    """ioc_host_pileup_sites: the variable sites of one reference from its table of counts (rlen + 1 rows of PILEUP_DTYPE) —
    returns (sites, n_found): the first max_sites sites (PILE_SITE_DTYPE), insertion site before base site row by row, and how
    many there are in all.  IocError for thresholds outside their ranges."""
    cols = np.ascontiguousarray(cols, PILEUP_DTYPE)
    if cols.ndim != 1 or len(cols) < 1:
        raise ValueError("cols must hold rlen + 1 rows")
    rlen = len(cols) - 1
    out, found = np.zeros(max(pileup_sites_bound(rlen, max(int(max_sites), 1)), 1), PILE_SITE_DTYPE), C.c_int64(0)
    n = _lib.load().ioc_host_pileup_sites(cols.ctypes.data, rlen, int(min_depth), int(min_alt), int(min_pct), int(max_sites), out.ctypes.data,
                                          C.byref(found))
    if n < 0:
        raise IocError(int(n), "ioc_host_pileup_sites")
    return out[:n].copy(), int(found.value)


def site_alleles(base, insf, sites):
    """ioc_host_site_alleles: the alleles of one read (its projection, ops_project) at `sites` (PILE_SITE_DTYPE) — one uint8 per
    site: the channel, ALLELE_DEL or ALLELE_NONE at a base site; 0 / 1 at an insertion site the read spans, else ALLELE_NONE."""
    base, insf = np.ascontiguousarray(base, np.uint8), np.ascontiguousarray(insf, np.uint8)
    sites = np.ascontiguousarray(sites, PILE_SITE_DTYPE)
    if base.shape != insf.shape or base.ndim != 1 or len(base) < 1:
        raise ValueError("base and insf must hold rlen + 1 bytes each")
    out = np.zeros(max(len(sites), 1), np.uint8)
    rc = _lib.load().ioc_host_site_alleles(base.ctypes.data, insf.ctypes.data, len(base) - 1, sites.ctypes.data, len(sites), out.ctypes.data)
    if rc != 0:
        raise ValueError(f"ioc_host_site_alleles failed ({rc})")
    return out[:len(sites)]


# ioc_split_seg as a numpy record, and the group byte of a read on neither side
SPLIT_SEG_DTYPE = np.dtype([(n, np.int32) for n in ("seed", "n_linked", "n_reads", "n_group0", "n_group1", "n_none")] + [("seed_link", np.int64)])
SPLIT_NONE = _lib.SPLIT_NONE


def alleles_split(sites, alleles, min_link=3, min_margin=1, rounds=2):
    """ioc_host_alleles_split: the split of one segment's reads in two by its linked sites — sites: PILE_SITE_DTYPE (minor and
    major are read), alleles: uint8 of shape (n_reads, n_sites), read-major, as site_alleles writes a read's.  Returns a dict:
    `link` (int64 per site), `phase` (int8 per site), `group` (uint8 per read: 0, 1 or SPLIT_NONE), `vote` (int32 per read) and
    `seg` (one SPLIT_SEG_DTYPE record).  IocError for min_link < 1, min_margin < 1 and rounds outside 0 .. 64."""
    sites = np.ascontiguousarray(sites, PILE_SITE_DTYPE)
    alleles = np.ascontiguousarray(alleles, np.uint8)
    if sites.ndim != 1 or alleles.ndim != 2 or alleles.shape[1] != len(sites):
        raise ValueError("alleles must have one row per read and one column per site")
    nr, ns = alleles.shape
    link, phase = np.zeros(max(ns, 1), np.int64), np.zeros(max(ns, 1), np.int8)
    group, vote, seg = np.zeros(max(nr, 1), np.uint8), np.zeros(max(nr, 1), np.int32), np.zeros(1, SPLIT_SEG_DTYPE)
    rc = _lib.load().ioc_host_alleles_split(sites.ctypes.data, ns, alleles.ctypes.data, nr, int(min_link), int(min_margin), int(rounds),
                                            link.ctypes.data, phase.ctypes.data, group.ctypes.data, vote.ctypes.data, seg.ctypes.data)
    if rc != 0:
        raise IocError(int(rc), "ioc_host_alleles_split")
    return {"link": link[:ns], "phase": phase[:ns], "group": group[:nr], "vote": vote[:nr], "seg": seg[0]}


def ops_to_comp(ops):
    """The comparison string of an operation string: '|' where the bases are equal, ' ' in every other column."""
    return bytes(ops).translate(bytes(0x7C if b == 0x3D else 0x20 for b in range(256)))


class Context:
    """One context per GPU (ioc_ctx)."""

    def __init__(self, device=0):
        self.L = _lib.load()
        h = C.c_void_p()
        rc = self.L.ioc_ctx_create(device, C.byref(h))
        if rc != 0:
            raise IocError(rc, "ioc_ctx_create failed (no MI355X visible?)")
        self.h = h
        self.device = int(device)   # (the HIP device is per THREAD: helpers that allocate through torch pass this explicitly)
        self._keep = []

    @property
    def serial(self):
        """Generation of the context's queries, kept by the LIBRARY (ioc_queries_generation): it changes with every call
        that replaces them, whichever method made it."""
        return int(self.L.ioc_queries_generation(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.L.ioc_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _chk(self, rc):
        if rc < 0:
            raise IocError(rc, self.L.ioc_last_error(self.h).decode(errors="replace"))
        return rc

    # ---- low level -------------------------------------------------------------------------
    def set_params(self, params: Params, table=_lib.TABLE_PATH):
        g, _ = host_gap_limits(params.k, params.w, params.min_prob_no_hits, table)
        g = np.ascontiguousarray(g.reshape(-1))
        self._chk(self.L.ioc_set_params(self.h, C.byref(params), _p(g, C.c_int32)))
        self.params = params

    def queries_upload(self, off_fwd, off_rev, min_val, min_pos, hpc_len, err_cell, min_total):
        off_fwd = np.ascontiguousarray(off_fwd, np.int64)
        off_rev = np.ascontiguousarray(off_rev, np.int64)
        min_val = np.ascontiguousarray(min_val, np.uint32)
        min_pos = np.ascontiguousarray(min_pos, np.uint32)
        hpc_len = np.ascontiguousarray(hpc_len, np.uint32)
        err_cell = np.ascontiguousarray(err_cell, np.uint8)
        min_total = np.ascontiguousarray(min_total, np.uint32)
        n = len(off_fwd) - 1
        self._chk(self.L.ioc_queries_upload(self.h, n, _p(off_fwd, C.c_int64), _p(off_rev, C.c_int64),
                                            _p(min_val, C.c_uint32), _p(min_pos, C.c_uint32), len(min_val),
                                            _p(hpc_len, C.c_uint32), _p(err_cell, C.c_uint8),
                                            _p(min_total, C.c_uint32)))
        self.n = n

    def left_load(self, n_clusters, cls_err_cell, keys, offs, postings):
        if n_clusters == 0:
            self._chk(self.L.ioc_left_load(self.h, 0, None, 0, None, None, None))
            return
        cls_err_cell = np.ascontiguousarray(cls_err_cell, np.uint8)
        keys = np.ascontiguousarray(keys, np.uint32)
        offs = np.ascontiguousarray(offs, np.int64)
        postings = np.ascontiguousarray(postings, np.uint32)
        self._chk(self.L.ioc_left_load(self.h, n_clusters, _p(cls_err_cell, C.c_uint8), len(keys),
                                       _p(keys, C.c_uint32), _p(offs, C.c_int64), _p(postings, C.c_uint32)))

    def index_update(self, cls, old_min, new_min, new_err_cell=0):
        """UpdateMinDB (src/minimizer.cpp:124-160) for left cluster `cls` on the device."""
        old_min = np.ascontiguousarray(old_min, np.uint32)
        new_min = np.ascontiguousarray(new_min, np.uint32)
        self._chk(self.L.ioc_index_update(self.h, int(cls), _p(old_min, C.c_uint32), len(old_min),
                                          _p(new_min, C.c_uint32), len(new_min), int(new_err_cell)))

    def left_export(self):
        """The left MinDB as it stands on the device: (keys, offs, postings), empty lists included."""
        nk, npost = C.c_int64(0), C.c_int64(0)
        self._chk(self.L.ioc_left_export(self.h, C.byref(nk), C.byref(npost), None, None, None))
        keys = np.zeros(nk.value, np.uint32)
        offs = np.zeros(nk.value + 1, np.int64)
        post = np.zeros(max(1, npost.value), np.uint32)
        self._chk(self.L.ioc_left_export(self.h, C.byref(nk), C.byref(npost), _p(keys, C.c_uint32),
                                         _p(offs, C.c_int64), _p(post, C.c_uint32)))
        return keys, offs, post[:npost.value]

    def left_adopt(self):
        """ioc_left_adopt: the clustering just resolved (left clusters + every query that opened one) becomes the left
        state, on the device.  Returns the new cluster count; the next call runs against it with left = dict(resident=True,
        cls_hpc_err=...)."""
        ncl = C.c_int32(0)
        self._chk(self.L.ioc_left_adopt(self.h, C.byref(ncl)))
        return int(ncl.value)

    def index_build(self):
        self._chk(self.L.ioc_index_build(self.h))

    def score(self):
        self._chk(self.L.ioc_score(self.h))

    def resolve(self):
        it = C.c_int32(0)
        self._chk(self.L.ioc_resolve(self.h, C.byref(it)))
        return it.value

    def decisions(self):
        n = self.n
        t, s, f = np.zeros(n, np.int32), np.zeros(n, np.int8), np.zeros(n, np.uint8)
        self._chk(self.L.ioc_get_decisions(self.h, _p(t, C.c_int32), _p(s, C.c_int8), _p(f, C.c_uint8)))
        return t, s, f

    def cuts(self):
        """ioc_get_cuts: per query int(top * MinFraction) of the last resolve, CUT_NONE where the query has no walk."""
        cut = np.zeros(self.n, np.int32)
        self._chk(self.L.ioc_get_cuts(self.h, _p(cut, C.c_int32)))
        return cut

    def force_decision(self, q, target, strand=1):
        self._chk(self.L.ioc_force_decision(self.h, q, target, strand))

    def clear_forced(self):
        self._chk(self.L.ioc_clear_forced(self.h))

    def set_aln_verdicts(self, target, strand=None):
        """ioc_set_aln_verdicts: per query the alignment fallback's verdict — NO_VERDICT, -1 (open a cluster) or an earlier
        target with its strand (+1 / -1) —, taken where the mapping walk finds nothing although top >= MinShared.  While
        verdicts are set the resolve also collects the tie sets (ties()).  target None switches both off."""
        if target is None:
            self._chk(self.L.ioc_set_aln_verdicts(self.h, None, None))
            return
        target = np.ascontiguousarray(target, np.int32)
        strand = np.ascontiguousarray(strand, np.int8)
        if target.shape != (self.n,) or strand.shape != (self.n,):
            raise ValueError("one verdict and one strand per query")
        self._chk(self.L.ioc_set_aln_verdicts(self.h, _p(target, C.c_int32), _p(strand, C.c_int8)))

    def ties(self):
        """ioc_get_ties: (count uint32[n], keys uint32[n, TIE_SLOTS]) — per query the candidates tied at the top Size among the
        clusters that exist, key = target << 1 | (strand == -1); of a longer tie set the count and TIE_SLOTS of its keys."""
        count, keys = np.zeros(self.n, np.uint32), np.zeros((self.n, TIE_SLOTS), np.uint32)
        self._chk(self.L.ioc_get_ties(self.h, _p(count, C.c_uint32), _p(keys, C.c_uint32)))
        return count, keys

    def query_candidates(self, q, cap):
        t, s = np.zeros(cap, np.int32), np.zeros(cap, np.int8)
        sz, fi, tm = (np.zeros(cap, np.uint32) for _ in range(3))
        n = self._chk(self.L.ioc_query_candidates(self.h, q, cap, _p(t, C.c_int32), _p(s, C.c_int8),
                                                  _p(sz, C.c_uint32), _p(fi, C.c_uint32), _p(tm, C.c_uint32)))
        return t[:n], s[:n], sz[:n], fi[:n], tm[:n]

    def set_shard(self, world, rank, fn):
        """ioc_set_shard: fast-mode score + resolve of the queries j with j % world == rank only; fn(d_ptr, count, kind,
        stream) is the in-place all-reduce over device memory (kind: _lib.XCHG_*) and returns 0.  world <= 1 or fn None
        switches it off."""
        if fn is None or world <= 1:
            self._shard_cb = None
            self._chk(self.L.ioc_set_shard(self.h, 1, 0, _lib.EXCHANGE_FN(), None))
            return

        def tramp(user, buf, count, kind, stream):
            try:
                return int(fn(buf, count, kind, stream) or 0)
            except Exception:      # an exception must not unwind through the C frames
                import traceback
                traceback.print_exc()
                return 1
        self._shard_cb = _lib.EXCHANGE_FN(tramp)      # kept alive for as long as the context may call it
        self._chk(self.L.ioc_set_shard(self.h, world, rank, self._shard_cb, None))

    @property
    def shard_exchanges(self):
        return int(self.L.ioc_shard_exchanges(self.h))

    @property
    def shard_aligned_pairs(self):
        """pairs THIS rank aligned in the sharded alignment rounds since set_shard (sahlin / furious)"""
        return int(self.L.ioc_shard_aligned_pairs(self.h))

    def scored_candidates(self, q, cap=1 << 16):
        """(key, size) the scoring kernels wrote for query q: key = target << 1 | strand."""
        key, size = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        m = self._chk(self.L.ioc_scored_candidates(self.h, q, cap, _p(key, C.c_uint32), _p(size, C.c_uint32)))
        assert m <= cap
        return key[:m], size[:m]

    def index_export(self):
        nk, npost = C.c_int64(0), C.c_int64(0)
        self._chk(self.L.ioc_index_export(self.h, C.byref(nk), C.byref(npost), None, None, None))
        keys = np.zeros(max(nk.value, 1), np.uint32)
        offs = np.zeros(nk.value + 1, np.int64)
        post = np.zeros(max(npost.value, 1), np.uint32)
        self._chk(self.L.ioc_index_export(self.h, C.byref(nk), C.byref(npost), _p(keys, C.c_uint32),
                                          _p(offs, C.c_int64), _p(post, C.c_uint32)))
        return keys[:nk.value], offs, post[:npost.value]

    def resident_set_sequences(self, raw_seq, raw_off, raw_err):
        """Raw sequences of the resident queries: lets cluster_resident run sahlin mode."""
        raw_seq = raw_seq if isinstance(raw_seq, bytes) else np.asarray(raw_seq, np.uint8).tobytes()
        raw_off = np.ascontiguousarray(raw_off, np.int64)
        raw_err = np.ascontiguousarray(raw_err, np.float64)
        self._chk(self.L.ioc_resident_set_sequences(self.h, raw_seq, _p(raw_off, C.c_int64), _p(raw_err, C.c_double)))

    # ---- alignment fallback on the GPU ---------------------------------------------------------
    def align_set_pool(self, seqs):
        """Upload the raw sequences (list of bytes) the pairs of align_pairs index into."""
        offs = np.zeros(len(seqs) + 1, np.int64)
        np.cumsum([len(x) for x in seqs], out=offs[1:])
        blob = b"".join(seqs)
        self._chk(self.L.ioc_align_set_pool(self.h, len(seqs), blob, _p(offs, C.c_int64)))
        self._aln_pool_offs = offs

    def align_set_pool_qual(self, quals):
        """ioc_align_set_pool_qual: the quality lines (list of bytes, laid out like align_set_pool's sequences) of the current
        pool, for align_pairs_polish_weighted; None drops them, as every align_set_pool does."""
        if quals is None:
            self._chk(self.L.ioc_align_set_pool_qual(self.h, None, 0))
            return
        blob = b"".join(bytes(x) for x in quals)
        self._chk(self.L.ioc_align_set_pool_qual(self.h, blob, len(blob)))

    def align_pool_offsets(self):
        """Where the sequences of the last align_set_pool start (n + 1 offsets; empty pool: [0])."""
        return getattr(self, "_aln_pool_offs", np.zeros(1, np.int64))

    def _pool_len(self, q):
        """the length of sequence q of the pool that is set (0 for one outside it: the library refuses the call)"""
        offs = self.align_pool_offsets()
        return int(offs[q + 1] - offs[q]) if 0 <= int(q) < len(offs) - 1 else 0

    def align_set_verdict_threshold(self, thr):
        """ioc_align_set_verdict_threshold: > 0 lets tracebacks stop once ratio >= thr is decided (windows / ratio become bounds)."""
        self._chk(self.L.ioc_align_set_verdict_threshold(self.h, float(thr)))

    @staticmethod
    def _aln_pairs(pairs):
        arr = (_lib.AlnPair * max(len(pairs), 1))()
        for i, pr in enumerate(pairs):        # (a fifth element: the similarity hint, ioc_aln_pair::reserved)
            qi, ri, rc, e = pr[:4]
            arr[i].query, arr[i].ref, arr[i].ref_revcomp, arr[i].e = int(qi), int(ri), int(bool(rc)), float(e)
            arr[i].reserved = int(pr[4]) if len(pr) > 4 else 0
        return arr

    @staticmethod
    def _aln_out(n):
        """the (score, windows, ratio) arrays of n pairs, and the three pointers an aligning call takes"""
        out = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.float64)
        return out, (_p(out[0], C.c_int32), _p(out[1], C.c_int64), _p(out[2], C.c_double))

    def align_pairs(self, pairs, k, match=2, mismatch=-2, gap_extend=1):
        """ParasailAlign + getAlnRatio (src/cluster.cpp:408-459) for (query, ref, ref_revcomp, e[, hint]) tuples:
        returns (score, qualifying windows, ratio) arrays."""
        n = len(pairs)
        out, ptrs = self._aln_out(n)
        self._chk(self.L.ioc_align_pairs(self.h, n, self._aln_pairs(pairs), k, match, mismatch, gap_extend, *ptrs))
        return out

    def align_pairs_ops(self, pairs, k, match=2, mismatch=-2, gap_extend=1):
        """ioc_align_pairs_ops: align_pairs plus the alignments themselves — returns (score, windows, ratio, [bytes per pair]),
        the bytes as host_align_ops gives them.  Always exact counts (the verdict threshold is not applied)."""
        n = len(pairs)
        arr = self._aln_pairs(pairs)
        bound = self._chk(self.L.ioc_align_ops_bound(self.h, n, arr))
        out, ptrs = self._aln_out(n)
        ops, off = np.zeros(max(bound, 1), np.uint8), np.zeros(n + 1, np.int64)
        self._chk(self.L.ioc_align_pairs_ops(self.h, n, arr, k, match, mismatch, gap_extend, *ptrs, ops.ctypes.data, bound, _p(off, C.c_int64)))
        return (*out, [ops[off[i]:off[i + 1]].tobytes() for i in range(n)])

    def align_pairs_stats(self, pairs, k, match=2, mismatch=-2, gap_extend=1):
        """ioc_align_pairs_stats: align_pairs plus the statistics of the alignments (ops_stats of what align_pairs_ops returns),
        counted on the device — returns (score, windows, ratio, stats), stats a structured array (ALN_STATS_DTYPE).  Always exact
        counts (the verdict threshold is not applied)."""
        n = len(pairs)
        out, ptrs = self._aln_out(n)
        stats = np.zeros(n, ALN_STATS_DTYPE)
        self._chk(self.L.ioc_align_pairs_stats(self.h, n, self._aln_pairs(pairs), k, match, mismatch, gap_extend, *ptrs,
                                               stats.ctypes.data if n else None))
        return (*out, stats)

    def align_pairs_pileup(self, pairs, k, row_base, n_rows, stats=False, match=2, mismatch=-2, gap_extend=1):
        """ioc_align_pairs_pileup: align_pairs plus the pileup of the alignments on their references, added up on the device —
        pair i adds ops_pileup of its alignment into rows row_base[i] .. row_base[i] + len(reference) of a table of n_rows rows
        (PILEUP_DTYPE); pairs with one row_base are piled together.  Returns (score, windows, ratio, cols), with stats=True
        (score, windows, ratio, cols, stats) — the records of align_pairs_stats from the same alignments.  Always exact counts."""
        n = len(pairs)
        arr = self._aln_pairs(pairs)
        row_base = np.ascontiguousarray(row_base, np.int64)
        if row_base.shape != (n,):
            raise ValueError("row_base must hold one entry per pair")
        out, ptrs = self._aln_out(n)
        cols = np.zeros(max(int(n_rows), 0), PILEUP_DTYPE)
        st = np.zeros(n, ALN_STATS_DTYPE) if stats else None
        self._chk(self.L.ioc_align_pairs_pileup(self.h, n, arr, k, match, mismatch, gap_extend, *ptrs, st.ctypes.data if stats and n else None,
                                                _p(row_base, C.c_int64), int(n_rows), cols.ctypes.data))
        return (*out, cols, st) if stats else (*out, cols)

    def _pileup_call(self, weighted, frames, cols, wcols, ins, min_depth, cap):
        """pileup_call (ins: what the reads insert) and pileup_call_weighted (wcols; ins: wins)"""
        n = len(frames)
        rlen = np.array([len(f) for f in frames], np.int32)
        n_rows = int(rlen.sum()) + n
        cols, ins = _tables(cols, ins, n_rows)
        if weighted:
            wcols = np.ascontiguousarray(wcols, PILEUP_DTYPE)
            if wcols.shape != (n_rows,):
                raise ValueError(f"wcols must hold {n_rows} rows")
        f_off = np.zeros(n + 1, np.int64)
        np.cumsum(rlen, out=f_off[1:])
        bound = sum(pileup_call_bound(r) for r in rlen)
        cap = bound if cap is None else int(cap)
        seq, qual = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint8)
        off, st = np.zeros(n + 1, np.int64), np.zeros(n, POLISH_STATS_DTYPE)
        fn = self.L.ioc_pileup_call_weighted if weighted else self.L.ioc_pileup_call
        tables = (cols.ctypes.data, wcols.ctypes.data, ins.ctypes.data) if weighted else (cols.ctypes.data, ins.ctypes.data)
        self._chk(fn(self.h, n, _p(rlen, C.c_int32), b"".join(bytes(f) for f in frames), _p(f_off, C.c_int64), *tables, int(min_depth),
                     seq.ctypes.data, qual.ctypes.data, cap, _p(off, C.c_int64), st.ctypes.data if n else None))
        return ([seq[off[g]:off[g + 1]].tobytes() for g in range(n)], [qual[off[g]:off[g + 1]].tobytes() for g in range(n)], st)

    def pileup_call(self, frames, cols, ins, min_depth=3, cap=None):
        """ioc_pileup_call: the consensus call of many references at once on the device, from host tables — `frames` a list of
        bytes, segment g's len(frames[g]) + 1 rows of cols / ins following those of the earlier segments.  Returns
        ([sequence per segment], [qualities per segment], stats), stats an array of POLISH_STATS_DTYPE; each segment as
        pileup_call defines it."""
        return self._pileup_call(False, frames, cols, None, ins, min_depth, cap)

    def pileup_call_weighted(self, frames, cols, wcols, wins, min_depth=3, cap=None):
        """ioc_pileup_call_weighted: pileup_call by weight, from host tables — `cols` gates, `wcols` / `wins` decide; each segment as
        pileup_call_weighted (the function) defines it.  Returns what pileup_call returns."""
        return self._pileup_call(True, frames, cols, wcols, wins, min_depth, cap)

    def _seg_args(self, n, segs, seg_of_pair):
        """The segment arguments of a call over the pool: (PolishSeg array, seg_of_pair as int32, the segments' lengths, the rows
        of a table of theirs) — the lengths all 0 where a segment lies outside the pool (the library refuses the call then)."""
        ns = len(segs)
        sarr = (_lib.PolishSeg * max(ns, 1))()
        for g, (ref, rc) in enumerate(segs):
            sarr[g].ref, sarr[g].ref_revcomp = int(ref), int(bool(rc))
        sop = np.ascontiguousarray(seg_of_pair, np.int32)
        if sop.shape != (n,):
            raise ValueError("seg_of_pair must hold one entry per pair")
        offs = self.align_pool_offsets()
        ok = all(0 <= int(ref) < len(offs) - 1 for ref, _ in segs)
        rlen = [int(offs[int(ref) + 1] - offs[int(ref)]) if ok else 0 for ref, _ in segs]
        return sarr, sop, rlen, sum(rlen) + ns

    @staticmethod
    def _site_outs(n, rlen, sop, max_sites, alleles=True):
        """The outputs of a site search over segments of lengths rlen and the alleles of n pairs, with their caps:
        (sites, s_cap, s_off, found, alleles or None, a_cap, a_off)."""
        ns = len(rlen)
        per_seg = [pileup_sites_bound(r, max(int(max_sites), 1)) for r in rlen]
        s_cap = sum(per_seg)
        a_cap = sum(per_seg[g] for g in sop if 0 <= g < ns)
        return (np.zeros(max(s_cap, 1), PILE_SITE_DTYPE), s_cap, np.zeros(ns + 1, np.int64), np.zeros(max(ns, 1), np.int64),
                np.zeros(max(a_cap, 1), np.uint8) if alleles else None, a_cap, np.zeros(n + 1, np.int64))

    @staticmethod
    def _row0(rlen):
        """the first row of every segment of a table"""
        return np.concatenate([[0], np.cumsum(np.array(rlen, np.int64) + 1)])[:len(rlen)]

    def _align_pairs_polish(self, weighted, pairs, k, segs, seg_of_pair, min_depth, stats, tables, cap, match, mismatch, gap_extend):
        """align_pairs_polish, and align_pairs_polish_weighted with its third table"""
        n, ns = len(pairs), len(segs)
        arr = self._aln_pairs(pairs)
        sarr, sop, rlen, n_rows = self._seg_args(n, segs, seg_of_pair)
        bound = sum(pileup_call_bound(r) for r in rlen)
        cap = bound if cap is None else int(cap)
        (score, win, ratio), ptrs = self._aln_out(n)
        seq, qual = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint8)
        off, pol = np.zeros(ns + 1, np.int64), np.zeros(ns, POLISH_STATS_DTYPE)
        st = np.zeros(n, ALN_STATS_DTYPE) if stats else None
        # the tables in the order both the C function and the dict name them: cols, (wcols,) ins / wins
        names = ("cols", "wcols", "wins") if weighted else ("cols", "ins")
        tabs = [np.zeros(n_rows, PILEUP_INS_DTYPE if name in ("ins", "wins") else PILEUP_DTYPE) if tables else None for name in names]
        fn = self.L.ioc_align_pairs_polish_weighted if weighted else self.L.ioc_align_pairs_polish
        self._chk(fn(self.h, n, arr, k, match, mismatch, gap_extend, *ptrs, st.ctypes.data if stats and n else None, ns, sarr,
                     _p(sop, C.c_int32), int(min_depth), seq.ctypes.data, qual.ctypes.data, cap, _p(off, C.c_int64),
                     pol.ctypes.data if ns else None, *(t.ctypes.data if tables and n_rows else None for t in tabs)))
        out = {"score": score, "windows": win, "ratio": ratio, "polish": pol,
               "seq": [seq[off[g]:off[g + 1]].tobytes() for g in range(ns)], "qual": [qual[off[g]:off[g + 1]].tobytes() for g in range(ns)]}
        if stats:
            out["stats"] = st
        if tables:
            out.update(zip(names, tabs))
            out["row0"] = self._row0(rlen)
        return out

    def align_pairs_polish(self, pairs, k, segs, seg_of_pair, min_depth=3, stats=False, tables=False, cap=None, match=2, mismatch=-2,
                           gap_extend=1):
        """ioc_align_pairs_polish: align_pairs, both pileup tables and the consensus call of every segment, all on the device —
        segs: (pool sequence, revcomp) per segment, the frame the segment's pairs were aligned against; seg_of_pair: the segment
        pair i is piled into.  Returns a dict: score, windows, ratio, seq and qual (lists of bytes per segment), polish
        (POLISH_STATS_DTYPE per segment), with stats=True `stats` (ALN_STATS_DTYPE per pair), with tables=True `cols` and `ins`
        (the rows of segment g from sum(len(frame) + 1) of the earlier ones on) and `row0` (the first row per segment)."""
        return self._align_pairs_polish(False, pairs, k, segs, seg_of_pair, min_depth, stats, tables, cap, match, mismatch, gap_extend)

    def align_pairs_polish_weighted(self, pairs, k, segs, seg_of_pair, min_depth=3, stats=False, tables=False, cap=None, match=2,
                                    mismatch=-2, gap_extend=1):
        """ioc_align_pairs_polish_weighted: align_pairs_polish with every vote weighted by the base quality of the read that casts
        it (align_set_pool_qual first).  Returns the same dict; with tables=True `cols` (the counts, as align_pairs_polish has
        them), `wcols` and `wins` (the sums of weights) and `row0`."""
        return self._align_pairs_polish(True, pairs, k, segs, seg_of_pair, min_depth, stats, tables, cap, match, mismatch, gap_extend)

    def pileup_sites(self, rlen, cols, min_depth=3, min_alt=3, min_pct=25, max_sites=4096, cap=None):
        """ioc_pileup_sites: the variable sites of many references at once on the device, from a host table — segment g's
        rlen[g] + 1 rows of `cols` following those of the earlier segments.  Returns ([sites per segment], n_found): arrays of
        PILE_SITE_DTYPE, each segment as pileup_sites (the function) defines it, and how many sites each has in all."""
        rlen = np.ascontiguousarray(rlen, np.int32)
        n = len(rlen)
        n_rows = int(rlen.astype(np.int64).sum()) + n
        cols = np.ascontiguousarray(cols, PILEUP_DTYPE)
        if cols.shape != (n_rows,):
            raise ValueError(f"cols must hold {n_rows} rows")
        bound = sum(pileup_sites_bound(r, max(int(max_sites), 1)) for r in rlen)
        cap = bound if cap is None else int(cap)
        sites, off, found = np.zeros(max(cap, 1), PILE_SITE_DTYPE), np.zeros(n + 1, np.int64), np.zeros(max(n, 1), np.int64)
        self._chk(self.L.ioc_pileup_sites(self.h, n, _p(rlen, C.c_int32) if n else None, cols.ctypes.data if n else None, int(min_depth),
                                          int(min_alt), int(min_pct), int(max_sites), sites.ctypes.data, cap, _p(off, C.c_int64),
                                          _p(found, C.c_int64)))
        return [sites[off[g]:off[g + 1]].copy() for g in range(n)], found[:n]

    def align_pairs_alleles(self, pairs, k, segs, seg_of_pair, min_depth=3, min_alt=3, min_pct=25, max_sites=4096, stats=False, tables=False,
                            match=2, mismatch=-2, gap_extend=1):
        """ioc_align_pairs_alleles: align_pairs, the pileup of every segment, its variable sites and every pair's alleles at them,
        all on the device — segs and seg_of_pair as for align_pairs_polish.  Returns a dict: score, windows, ratio, `sites` (a list
        of PILE_SITE_DTYPE arrays per segment, at most max_sites each), `n_found` (sites per segment in all), `alleles` (a list of
        uint8 arrays per pair: one byte per kept site of its segment — the channel 0 .. 4, ALLELE_DEL or ALLELE_NONE at a base site,
        0 / 1 or ALLELE_NONE at an insertion site), with stats=True `stats` (ALN_STATS_DTYPE per pair), with tables=True `cols`
        (the table of counts) and `row0` (the first row per segment)."""
        return self._align_pairs_split(None, pairs, k, segs, seg_of_pair, min_depth, min_alt, min_pct, max_sites, None, None, None, stats, tables, True,
                                       match, mismatch, gap_extend, split=False)

    @staticmethod
    def _split_out(s_off, a_off_unused, sop, ns, n, link, phase, group, vote, seg):
        """The split's flat outputs as a dict of per-segment lists: link / phase by the sites' offsets, group / vote by the pairs of
        every segment in ascending pair order."""
        members = [np.flatnonzero(sop == g) for g in range(ns)]
        return {"link": [link[s_off[g]:s_off[g + 1]].copy() for g in range(ns)], "phase": [phase[s_off[g]:s_off[g + 1]].copy() for g in range(ns)],
                "group": group[:n], "vote": vote[:n], "seg": seg[:ns], "members": members}

    def alleles_split(self, sites, alleles, seg_of_pair, min_link=3, min_margin=1, rounds=2):
        """ioc_alleles_split: the split of many segments at once on the device, from host tables — sites: a list of PILE_SITE_DTYPE
        arrays per segment; alleles: a list of uint8 arrays per pair, one byte per site of segment seg_of_pair[i] (what
        align_pairs_alleles returns).  A segment's reads are its pairs in ascending order.  Returns a dict: `link` and `phase`
        (lists of arrays per segment), `group` (uint8 per pair), `vote` (int32 per pair), `seg` (SPLIT_SEG_DTYPE per segment) and
        `members` (the pairs of every segment), each segment as alleles_split (the function) defines it."""
        ns, n = len(sites), len(alleles)
        sop = np.ascontiguousarray(seg_of_pair, np.int32)
        if sop.shape != (n,):
            raise ValueError("seg_of_pair must hold one entry per pair")
        s_off = np.concatenate([[0], np.cumsum([len(x) for x in sites])]).astype(np.int64)
        a_off = np.concatenate([[0], np.cumsum([len(x) for x in alleles])]).astype(np.int64)
        flat_s = np.ascontiguousarray(np.concatenate([np.zeros(0, PILE_SITE_DTYPE)] + [np.asarray(x, PILE_SITE_DTYPE) for x in sites]))
        flat_a = np.ascontiguousarray(np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(x, np.uint8) for x in alleles]))
        S = int(s_off[-1])
        link, phase = np.zeros(max(S, 1), np.int64), np.zeros(max(S, 1), np.int8)
        group, vote, seg = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int32), np.zeros(max(ns, 1), SPLIT_SEG_DTYPE)
        self._chk(self.L.ioc_alleles_split(self.h, ns, n, _p(sop, C.c_int32) if n else None, flat_s.ctypes.data if S else None, _p(s_off, C.c_int64),
                                           flat_a.ctypes.data if len(flat_a) else None, _p(a_off, C.c_int64), int(min_link), int(min_margin),
                                           int(rounds), link.ctypes.data, phase.ctypes.data, group.ctypes.data, vote.ctypes.data, seg.ctypes.data))
        return self._split_out(s_off, a_off, sop, ns, n, link, phase, group, vote, seg)

    def planes_polish(self, frames, seg_of_pair, group, base, slots, min_depth=3, tables=False, cap=None):
        """ioc_planes_polish: the consensus of both groups of every segment on the device, from host planes — `frames` a list of
        bytes per segment; seg_of_pair / group (0, 1 or SPLIT_NONE) per pair; base / slots lists per pair of what ops_project and
        ops_project_ins give for that pair (len(frame) + 1 bytes, PILE_INS_SLOTS x (len(frame) + 1)).  Returns a dict: `gseq` and
        `gqual` (lists of [group 0, group 1] per segment), `gpolish` (POLISH_STATS_DTYPE, shape (segments, 2)), with tables=True
        `gcols` and `gins` (2 * (len(frame) + 1) rows per segment, group 0's before group 1's) and `grow0` (shape (segments, 2)) —
        each group-segment as pileup_call defines it on the tables planes_pile adds up from the group's reads."""
        ns, n = len(frames), len(base)
        rlen = np.array([len(f) for f in frames], np.int32)
        sop, grp = np.ascontiguousarray(seg_of_pair, np.int32), np.ascontiguousarray(group, np.uint8)
        if sop.shape != (n,) or grp.shape != (n,) or len(slots) != n:
            raise ValueError("seg_of_pair, group, base and slots must hold one entry per pair")
        rows = [int(rlen[g]) + 1 if 0 <= g < ns else 0 for g in sop]
        for i in range(n):
            if np.shape(base[i]) != (rows[i],) or np.shape(slots[i]) != (_lib.PILE_INS_SLOTS, rows[i]):
                raise ValueError(f"the planes of pair {i} are not those of its segment")
        P = sum(rows)
        fb = np.ascontiguousarray(np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(b, np.uint8) for b in base]))
        fs = np.ascontiguousarray(np.concatenate([np.zeros((_lib.PILE_INS_SLOTS, 0), np.uint8)] + [np.asarray(x, np.uint8) for x in slots], axis=1))
        f_off = np.zeros(ns + 1, np.int64)
        np.cumsum(rlen, out=f_off[1:])
        bound = 2 * sum(pileup_call_bound(r) for r in rlen)
        cap = bound if cap is None else int(cap)
        n_rows = 2 * (int(rlen.sum()) + ns)
        seq, qual = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint8)
        off, pol = np.zeros(2 * ns + 1, np.int64), np.zeros(2 * ns, POLISH_STATS_DTYPE)
        gcols, gins = (np.zeros(n_rows, PILEUP_DTYPE), np.zeros(n_rows, PILEUP_INS_DTYPE)) if tables else (None, None)
        self._chk(self.L.ioc_planes_polish(self.h, ns, _p(rlen, C.c_int32) if ns else None, b"".join(bytes(f) for f in frames), _p(f_off, C.c_int64), n,
                                           _p(sop, C.c_int32) if n else None, grp.ctypes.data if n else None, fb.ctypes.data if P else None,
                                           fs.ctypes.data if P else None, int(min_depth), seq.ctypes.data, qual.ctypes.data, cap, _p(off, C.c_int64),
                                           pol.ctypes.data if ns else None, gcols.ctypes.data if tables and n_rows else None,
                                           gins.ctypes.data if tables and n_rows else None))
        return self._gpolish_out(ns, rlen, seq, qual, off, pol, gcols, gins, tables)

    def planes_correct(self, frames, cols, ins, seg_of_pair, base, slots, min_depth=3, min_alt=3, min_pct=25, max_run=10, cap=None):
        """ioc_planes_correct: every read of many segments corrected on the device, from host planes and host tables — `frames` a
        list of bytes per segment, `cols` / `ins` the segments' tables one behind the other (as for pileup_call), seg_of_pair per pair,
        base / slots lists per pair of what ops_project and ops_project_ins give for that pair.  Returns ([sequence per pair],
        [qualities per pair], stats), stats an array of CORRECT_STATS_DTYPE; each pair as read_correct defines it."""
        ns, n = len(frames), len(base)
        rlen = np.array([len(f) for f in frames], np.int32)
        n_rows = int(rlen.sum()) + ns
        cols, ins = _tables(cols, ins, n_rows)
        sop = np.ascontiguousarray(seg_of_pair, np.int32)
        if sop.shape != (n,) or len(slots) != n:
            raise ValueError("seg_of_pair, base and slots must hold one entry per pair")
        rows = [int(rlen[g]) + 1 if 0 <= g < ns else 0 for g in sop]
        for i in range(n):
            if np.shape(base[i]) != (rows[i],) or np.shape(slots[i]) != (_lib.PILE_INS_SLOTS, rows[i]):
                raise ValueError(f"the planes of pair {i} are not those of its segment")
        P = sum(rows)
        fb = np.ascontiguousarray(np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(b, np.uint8) for b in base]))
        fs = np.ascontiguousarray(np.concatenate([np.zeros((_lib.PILE_INS_SLOTS, 0), np.uint8)] + [np.asarray(x, np.uint8) for x in slots], axis=1))
        f_off = np.zeros(ns + 1, np.int64)
        np.cumsum(rlen, out=f_off[1:])
        bound = sum(pileup_call_bound(rlen[g]) for g in sop if 0 <= g < ns)
        cap = bound if cap is None else int(cap)
        seq, qual = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint8)
        off, st = np.zeros(n + 1, np.int64), np.zeros(n, CORRECT_STATS_DTYPE)
        self._chk(self.L.ioc_planes_correct(self.h, ns, _p(rlen, C.c_int32) if ns else None, b"".join(bytes(f) for f in frames), _p(f_off, C.c_int64),
                                            cols.ctypes.data if n_rows else None, ins.ctypes.data if n_rows else None, n, _p(sop, C.c_int32) if n else None,
                                            fb.ctypes.data if P else None, fs.ctypes.data if P else None, int(min_depth), int(min_alt), int(min_pct),
                                            int(max_run), seq.ctypes.data, qual.ctypes.data, cap, _p(off, C.c_int64), st.ctypes.data if n else None))
        return ([seq[off[i]:off[i + 1]].tobytes() for i in range(n)], [qual[off[i]:off[i + 1]].tobytes() for i in range(n)], st)

    def planes_correct_groups(self, frames, seg_of_pair, group, n_groups, query, base, slots, ilen, qpos, min_depth=3, min_alt=3, min_pct=25, max_run=10,
                              cap=None):
        """ioc_planes_correct_groups: every read of many segments corrected against the tables of its own isoform on the device,
        from host planes, over the pool that is set — frames, seg_of_pair, group and n_groups as for planes_polish_groups, `query`
        (the pool sequence that is its read) per pair, base / slots / ilen / qpos lists per pair of what ops_project,
        ops_project_ins, ops_project_ilen and ops_project_qpos give for that pair.  A pair in a group of at least min_depth
        members is held against that group's tables, any other against those of all pairs of its segment.  Returns ([sequence per
        pair], [qualities per pair], stats), stats an array of ISO_CORRECT_STATS_DTYPE; each pair as read_correct_long defines it."""
        ns, n = len(frames), len(base)
        rlen = np.array([len(f) for f in frames], np.int32)
        sop, grp, ng, qy = (np.ascontiguousarray(x, np.int32) for x in (seg_of_pair, group, n_groups, query))
        if sop.shape != (n,) or grp.shape != (n,) or qy.shape != (n,) or len(slots) != n or len(ilen) != n or len(qpos) != n or ng.shape != (ns,):
            raise ValueError("seg_of_pair, group, query and the planes must hold one entry per pair and n_groups one per segment")
        rows = [int(rlen[g]) + 1 if 0 <= g < ns else 0 for g in sop]
        for i in range(n):
            if np.shape(base[i]) != (rows[i],) or np.shape(slots[i]) != (_lib.PILE_INS_SLOTS, rows[i]) or np.shape(ilen[i]) != (rows[i],) or \
                    np.shape(qpos[i]) != (rows[i],):
                raise ValueError(f"the planes of pair {i} are not those of its segment")
        P = sum(rows)
        flat = lambda planes, t: np.ascontiguousarray(np.concatenate([np.zeros(0, t)] + [np.asarray(b, t) for b in planes]))
        fb, fl, fq = flat(base, np.uint8), flat(ilen, np.uint8), flat(qpos, np.uint32)
        fs = np.ascontiguousarray(np.concatenate([np.zeros((_lib.PILE_INS_SLOTS, 0), np.uint8)] + [np.asarray(x, np.uint8) for x in slots], axis=1))
        f_off = np.zeros(ns + 1, np.int64)
        np.cumsum(rlen, out=f_off[1:])
        bound = sum(pileup_call_bound(rlen[g]) for g in sop if 0 <= g < ns) + sum(self._pool_len(q) for q in qy)
        cap = bound if cap is None else int(cap)
        seq, qual = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint8)
        off, st = np.zeros(n + 1, np.int64), np.zeros(n, ISO_CORRECT_STATS_DTYPE)
        self._chk(self.L.ioc_planes_correct_groups(self.h, ns, _p(rlen, C.c_int32) if ns else None, b"".join(bytes(f) for f in frames), _p(f_off, C.c_int64),
                                                   _p(ng, C.c_int32) if ns else None, n, _p(sop, C.c_int32) if n else None, _p(grp, C.c_int32) if n else None,
                                                   _p(qy, C.c_int32) if n else None, fb.ctypes.data if P else None, fs.ctypes.data if P else None,
                                                   fl.ctypes.data if P else None, fq.ctypes.data if P else None, int(min_depth), int(min_alt), int(min_pct),
                                                   int(max_run), seq.ctypes.data, qual.ctypes.data, cap, _p(off, C.c_int64), st.ctypes.data if n else None))
        return ([seq[off[i]:off[i + 1]].tobytes() for i in range(n)], [qual[off[i]:off[i + 1]].tobytes() for i in range(n)], st)

    def align_pairs_correct(self, pairs, k, segs, seg_of_pair, min_depth=3, min_alt=3, min_pct=25, max_run=10, stats=False, tables=False, cap=None,
                            match=2, mismatch=-2, gap_extend=1):
        """ioc_align_pairs_correct: align_pairs, both pileup tables, every pair's planes and the correction of every pair's read
        against its segment's pileup, all on the device, every pair aligned once — segs / seg_of_pair as for align_pairs_polish.
        Returns a dict: score, windows, ratio, `seq` and `qual` (lists of bytes per PAIR: the corrected aligned part of the query),
        `correct` (CORRECT_STATS_DTYPE per pair), with stats=True `stats` (ALN_STATS_DTYPE per pair), with tables=True `cols`, `ins`
        and `row0` as align_pairs_polish returns them.  Each pair as read_correct defines it on the pair's projections."""
        n, ns = len(pairs), len(segs)
        arr = self._aln_pairs(pairs)
        sarr, sop, rlen, n_rows = self._seg_args(n, segs, seg_of_pair)
        bound = sum(pileup_call_bound(rlen[g]) for g in sop if 0 <= g < ns)
        cap = bound if cap is None else int(cap)
        (score, win, ratio), ptrs = self._aln_out(n)
        seq, qual = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint8)
        off, cor = np.zeros(n + 1, np.int64), np.zeros(n, CORRECT_STATS_DTYPE)
        st = np.zeros(n, ALN_STATS_DTYPE) if stats else None
        cols, ins = (np.zeros(n_rows, PILEUP_DTYPE), np.zeros(n_rows, PILEUP_INS_DTYPE)) if tables else (None, None)
        self._chk(self.L.ioc_align_pairs_correct(self.h, n, arr, k, match, mismatch, gap_extend, *ptrs, st.ctypes.data if stats and n else None, ns, sarr,
                                                 _p(sop, C.c_int32), int(min_depth), int(min_alt), int(min_pct), int(max_run), seq.ctypes.data,
                                                 qual.ctypes.data, cap, _p(off, C.c_int64), cor.ctypes.data if n else None,
                                                 cols.ctypes.data if tables and n_rows else None, ins.ctypes.data if tables and n_rows else None))
        out = {"score": score, "windows": win, "ratio": ratio, "correct": cor,
               "seq": [seq[off[i]:off[i + 1]].tobytes() for i in range(n)], "qual": [qual[off[i]:off[i + 1]].tobytes() for i in range(n)]}
        if stats:
            out["stats"] = st
        if tables:
            out.update(cols=cols, ins=ins, row0=self._row0(rlen))
        return out

    @staticmethod
    def _blocks_out(ns, rlen, rule, rows, cap):
        """the output arrays of a block search over segments of these lengths, and the pointers the library takes behind the rule"""
        bound = sum(planes_blocks_bound(m, rule[5]) for m in rlen)
        cap = bound if cap is None else int(cap)
        n_rows = int(sum(rlen)) + ns
        tab = np.zeros(n_rows, BLOCK_ROW_DTYPE) if rows else None
        blocks, boff, seg = np.zeros(max(cap, 1), PILE_BLOCK_DTYPE), np.zeros(ns + 1, np.int64), np.zeros(ns, BLOCKS_SEG_DTYPE)
        return (tab, blocks, boff, seg), cap

    def _blocks_dict(self, ns, rlen, n, tab, blocks, boff, reads, seg):
        out = {"blocks": [blocks[boff[g]:boff[g + 1]] for g in range(ns)], "block_off": boff, "reads": reads, "seg": seg}
        if tab is not None:
            r0 = np.concatenate([self._row0(rlen), [len(tab)]]).astype(np.int64) if ns else np.zeros(1, np.int64)
            out.update(rows=[tab[r0[g]:r0[g + 1]] for g in range(ns)])
        return out

    def _blocks_family(self, pairs, k, segs, seg_of_pair, rule, stats, tables, rows, cap, match, mismatch, gap_extend):
        """What every call of the block family (align_pairs_blocks and the calls that go on from its block search) begins with: the
        pairs', the segments' and the block search's arrays.  Returns them as one record; `lead` is the arguments all of the entry
        points take first, the context's handle to out_cols."""
        f = types.SimpleNamespace(n=len(pairs), ns=len(segs), stats=stats, tables=tables, rows=rows)
        n, ns = f.n, f.ns
        arr = self._aln_pairs(pairs)
        sarr, f.sop, f.rlen, n_rows = self._seg_args(n, segs, seg_of_pair)
        f.r = _blocks_rule(rule)
        (f.tab, f.blocks, f.boff, f.seg), cap = self._blocks_out(ns, f.rlen, f.r, rows, cap)
        (f.score, f.win, f.ratio), ptrs = self._aln_out(n)
        f.reads = np.zeros(n, READ_BLOCKS_DTYPE)
        f.st = np.zeros(n, ALN_STATS_DTYPE) if stats else None
        f.cols = np.zeros(n_rows, PILEUP_DTYPE) if tables else None
        f.lead = (self.h, n, arr, k, match, mismatch, gap_extend, *ptrs, f.st.ctypes.data if stats and n else None, ns, sarr, _p(f.sop, C.c_int32), *f.r,
                  f.tab.ctypes.data if rows and len(f.tab) else None, f.blocks.ctypes.data, cap, _p(f.boff, C.c_int64), f.reads.ctypes.data if n else None,
                  f.seg.ctypes.data if ns else None, f.cols.ctypes.data if tables and n_rows else None)
        return f

    def _blocks_family_out(self, f, **more):
        """... and what every one of them ends with: align_pairs_blocks' dict, what the later stages made (`more`), `stats`, `cols` and `row0`"""
        out = {"score": f.score, "windows": f.win, "ratio": f.ratio, **self._blocks_dict(f.ns, f.rlen, f.n, f.tab, f.blocks, f.boff, f.reads, f.seg), **more}
        if f.stats:
            out["stats"] = f.st
        if f.tables:
            out.update(cols=f.cols, row0=self._row0(f.rlen))
        return out

    def planes_blocks(self, rlen, seg_of_pair, base, rows=True, cap=None, **rule):
        """ioc_planes_blocks: the exon blocks of many segments and every read's isoform on the device, from host base planes — `rlen`
        the segments' lengths, seg_of_pair per pair, `base` a list per pair of what ops_project gives for that pair (a segment's
        reads are its pairs in ascending order); the rule as keywords.  Returns a dict: `blocks` (a PILE_BLOCK_DTYPE array per
        segment), `block_off`, `reads` (READ_BLOCKS_DTYPE per pair), `seg` (BLOCKS_SEG_DTYPE per segment) and, with rows=True, `rows`
        (a BLOCK_ROW_DTYPE array per segment); each segment as api.planes_blocks defines it."""
        ns, n = len(rlen), len(base)
        rl = np.ascontiguousarray(rlen, np.int32)
        sop = np.ascontiguousarray(seg_of_pair, np.int32)
        if sop.shape != (n,):
            raise ValueError("seg_of_pair and base must hold one entry per pair")
        want = [int(rl[g]) + 1 if 0 <= g < ns else 0 for g in sop]
        for i in range(n):
            if np.shape(base[i]) != (want[i],):
                raise ValueError(f"the plane of pair {i} is not that of its segment")
        fb = np.ascontiguousarray(np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(b, np.uint8) for b in base]))
        r = _blocks_rule(rule)
        (tab, blocks, boff, seg), cap = self._blocks_out(ns, [max(int(m), 0) for m in rl], r, rows, cap)
        reads = np.zeros(n, READ_BLOCKS_DTYPE)
        self._chk(self.L.ioc_planes_blocks(self.h, ns, _p(rl, C.c_int32) if ns else None, n, _p(sop, C.c_int32) if n else None, fb.ctypes.data if len(fb) else None,
                                           *r, tab.ctypes.data if rows and len(tab) else None, blocks.ctypes.data, cap, _p(boff, C.c_int64),
                                           reads.ctypes.data if n else None, seg.ctypes.data if ns else None))
        return self._blocks_dict(ns, [int(m) for m in rl], n, tab, blocks, boff, reads, seg)

    @staticmethod
    def _inserts_out(ns, rlen, rule, rows, cap):
        """the output arrays of a search for insertion sites over segments of these lengths"""
        bound = sum(planes_inserts_bound(m, rule[5]) for m in rlen)
        cap = bound if cap is None else int(cap)
        tab = np.zeros(int(sum(rlen)) + ns, INSERT_ROW_DTYPE) if rows else None
        sites, soff, seg = np.zeros(max(cap, 1), PILE_INSERT_DTYPE), np.zeros(ns + 1, np.int64), np.zeros(ns, INSERTS_SEG_DTYPE)
        return (tab, sites, soff, seg), cap

    def _inserts_dict(self, ns, rlen, tab, sites, soff, reads, seg):
        out = {"sites": [sites[soff[g]:soff[g + 1]] for g in range(ns)], "site_off": soff, "reads": reads, "seg": seg}
        if tab is not None:
            r0 = np.concatenate([self._row0(rlen), [len(tab)]]).astype(np.int64) if ns else np.zeros(1, np.int64)
            out.update(rows=[tab[r0[g]:r0[g + 1]] for g in range(ns)])
        return out

    def planes_inserts(self, rlen, seg_of_pair, base, ilen, pre_key=None, pre_mask=None, pre_full=None, rows=True, cap=None, **rule):
        """ioc_planes_inserts: the insertion sites of many segments and every read's combined isoform on the device, from host
        planes — `rlen` the segments' lengths, seg_of_pair per pair, `base` / `ilen` a list per pair of what ops_project /
        ops_project_ilen give for that pair; pre_key / pre_mask per pair and pre_full per segment, all three or none; the rule as
        keywords.  Returns a dict: `sites` (a PILE_INSERT_DTYPE array per segment), `site_off`, `reads` (READ_INSERTS_DTYPE per pair),
        `seg` (INSERTS_SEG_DTYPE per segment) and, with rows=True, `rows` (an INSERT_ROW_DTYPE array per segment); each segment as
        api.planes_inserts defines it."""
        ns, n = len(rlen), len(base)
        rl = np.ascontiguousarray(rlen, np.int32)
        sop = np.ascontiguousarray(seg_of_pair, np.int32)
        if sop.shape != (n,) or len(ilen) != n:
            raise ValueError("seg_of_pair, base and ilen must hold one entry per pair")
        want = [int(rl[g]) + 1 if 0 <= g < ns else 0 for g in sop]
        for i in range(n):
            if np.shape(base[i]) != (want[i],) or np.shape(ilen[i]) != (want[i],):
                raise ValueError(f"the planes of pair {i} are not those of its segment")
        fb = np.ascontiguousarray(np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(b, np.uint8) for b in base]))
        fl = np.ascontiguousarray(np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(b, np.uint8) for b in ilen]))
        given = [x is not None for x in (pre_key, pre_mask, pre_full)]
        if any(given) and not all(given):
            raise ValueError("pre_key, pre_mask and pre_full: all three or none")
        pk = pm = pf = None
        if all(given):
            pk, pm, pf = (np.ascontiguousarray(x, np.uint64) for x in (pre_key, pre_mask, pre_full))
            if pk.shape != (n,) or pm.shape != (n,) or pf.shape != (ns,):
                raise ValueError("pre_key and pre_mask must hold one word per pair, pre_full one per segment")
            pk, pm, pf = (np.concatenate([x, np.zeros(1, np.uint64)]) for x in (pk, pm, pf))  # (never an empty array's pointer)
        r = _inserts_rule(rule)
        (tab, sites, soff, seg), cap = self._inserts_out(ns, [max(int(m), 0) for m in rl], r, rows, cap)
        reads = np.zeros(n, READ_INSERTS_DTYPE)
        self._chk(self.L.ioc_planes_inserts(self.h, ns, _p(rl, C.c_int32) if ns else None, n, _p(sop, C.c_int32) if n else None, fb.ctypes.data if len(fb) else None,
                                            fl.ctypes.data if len(fl) else None, *r, *(x.ctypes.data if x is not None else None for x in (pk, pm, pf)),
                                            tab.ctypes.data if rows and len(tab) else None, sites.ctypes.data, cap, _p(soff, C.c_int64),
                                            reads.ctypes.data if n else None, seg.ctypes.data if ns else None))
        return self._inserts_dict(ns, [int(m) for m in rl], tab, sites, soff, reads, seg)

    def align_pairs_blocks_inserts(self, pairs, k, segs, seg_of_pair, stats=False, tables=False, rows=True, cap=None, sites_cap=None, match=2, mismatch=-2,
                                   gap_extend=1, min_ins=INSERTS_RULE["min_ins"], slack=INSERTS_RULE["slack"], max_sites=INSERTS_RULE["max_sites"], **rule):
        """ioc_align_pairs_blocks_inserts: align_pairs_blocks with every pair's length plane projected beside its base plane and the
        search for insertion sites behind the block search, on the device, every pair aligned once — the block rule as keywords,
        min_ins / slack / max_sites for the sites (min_depth, min_alt and min_pct are shared).  Returns align_pairs_blocks' dict,
        byte for byte, and under `inserts` what Context.planes_inserts returns, group / how of its reads being the isoform over blocks
        and sites together."""
        f = self._blocks_family(pairs, k, segs, seg_of_pair, rule, stats, tables, rows, cap, match, mismatch, gap_extend)
        n, ns, rlen = f.n, f.ns, f.rlen
        ir = [int(min_ins), int(slack), f.r[1], f.r[2], f.r[3], int(max_sites)]
        (itab, sites, soff, iseg), sites_cap = self._inserts_out(ns, rlen, ir, rows, sites_cap)
        ireads = np.zeros(n, READ_INSERTS_DTYPE)
        self._chk(self.L.ioc_align_pairs_blocks_inserts(*f.lead, ir[0], ir[1], ir[5], itab.ctypes.data if rows and len(itab) else None, sites.ctypes.data, sites_cap,
                                                        _p(soff, C.c_int64), ireads.ctypes.data if n else None, iseg.ctypes.data if ns else None))
        return self._blocks_family_out(f, inserts=self._inserts_dict(ns, rlen, itab, sites, soff, ireads, iseg))

    @staticmethod
    def _windows_dict(win, seq, qual, off, pol):
        S = len(win)
        return {"win": win, "seq": [seq[off[x]:off[x + 1]].tobytes() for x in range(S)], "qual": [qual[off[x]:off[x + 1]].tobytes() for x in range(S)],
                "off": off, "polish": pol}

    def planes_insert_windows(self, rlen, seg_of_pair, query, base, qpos, sites, keys, min_depth=3, tables=False, cap=None, site_off=None, **rule):
        """ioc_planes_insert_windows: the consensus of the carriers' windows at every kept insertion site, on the device, over the pool
        that is set — `rlen` the segments' lengths, seg_of_pair and `query` (the pool sequence that is its read) per pair, `base` /
        `qpos` a list per pair of what ops_project / ops_project_qpos give, `sites` a PILE_INSERT_DTYPE array per segment and `keys`
        per pair as planes_inserts returned them (site_off: in place of the offsets the arrays give, with `sites` packed); slack,
        max_win, match, mismatch and gap as keywords (WINDOWS_RULE has the defaults).  Returns a dict, a site each in site order: `win`
        (INSERT_WINDOW_DTYPE; template_pair is the pair), `seq` and `qual` (bytes; empty where a site has no voter), `off`, `polish`
        (POLISH_STATS_DTYPE) and, with tables=True, `cols`, `ins` and `row0` (site x's tlen + 1 rows begin at row0[x]) — each site as
        pileup_call defines it on the tables planes_pile adds up from its voters' alignments to the template."""
        unknown = set(rule) - set(WINDOWS_RULE)
        if unknown:
            raise TypeError(f"unknown rule parameters: {sorted(unknown)}")
        r = [int({**WINDOWS_RULE, **rule}[n]) for n in WINDOWS_RULE]
        ns, n = len(rlen), len(base)
        rl, sop, qy, ky = (np.ascontiguousarray(x, t) for x, t in ((rlen, np.int32), (seg_of_pair, np.int32), (query, np.int32), (keys, np.uint64)))
        if sop.shape != (n,) or qy.shape != (n,) or ky.shape != (n,) or len(qpos) != n:
            raise ValueError("seg_of_pair, query, keys, base and qpos must hold one entry per pair")
        want = [int(rl[g]) + 1 if 0 <= g < ns else 0 for g in sop]
        for i in range(n):
            if np.shape(base[i]) != (want[i],) or np.shape(qpos[i]) != (want[i],):
                raise ValueError(f"the planes of pair {i} are not those of its segment")
        fb = np.ascontiguousarray(np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(b, np.uint8) for b in base]))
        fq = np.ascontiguousarray(np.concatenate([np.zeros(0, np.uint32)] + [np.asarray(b, np.uint32) for b in qpos]))
        if site_off is None:
            soff = np.concatenate([[0], np.cumsum([len(s) for s in sites])]).astype(np.int64)
            st = np.ascontiguousarray(np.concatenate([np.zeros(0, PILE_INSERT_DTYPE)] + [np.asarray(s, PILE_INSERT_DTYPE) for s in sites]))
        else:
            soff, st = np.ascontiguousarray(site_off, np.int64), np.ascontiguousarray(sites, PILE_INSERT_DTYPE)
        if soff.shape != (ns + 1,):
            raise ValueError("the sites must hold one array per segment")
        S = max(int(soff[-1]), 0)
        cap = insert_windows_bound(S, r[1]) if cap is None else int(cap)
        win, off, pol = np.zeros(max(S, 1), INSERT_WINDOW_DTYPE), np.zeros(S + 1, np.int64), np.zeros(max(S, 1), POLISH_STATS_DTYPE)
        seq, qual = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint8)
        n_rows = S * (max(r[1], 0) + 1)
        cols, ins = (np.zeros(max(n_rows, 1), PILEUP_DTYPE), np.zeros(max(n_rows, 1), PILEUP_INS_DTYPE)) if tables else (None, None)
        pad = lambda a: np.concatenate([a, np.zeros(1, a.dtype)])  # (never an empty array's pointer)
        st, ky, qy, sop, fb, fq = (pad(x) for x in (st, ky, qy, sop, fb, fq))
        self._chk(self.L.ioc_planes_insert_windows(self.h, ns, _p(rl, C.c_int32) if ns else None, n, _p(sop, C.c_int32), _p(qy, C.c_int32), fb.ctypes.data,
                                                   fq.ctypes.data, st.ctypes.data, _p(soff, C.c_int64), ky.ctypes.data, r[0], r[1], r[2], r[3], r[4],
                                                   int(min_depth), win.ctypes.data, seq.ctypes.data, qual.ctypes.data, cap, _p(off, C.c_int64),
                                                   pol.ctypes.data, cols.ctypes.data if tables else None, ins.ctypes.data if tables else None))
        out = self._windows_dict(win[:S], seq, qual, off, pol[:S])
        if tables:
            per = win[:S]["tlen"].astype(np.int64) + (win[:S]["tlen"] > 0)
            row0 = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
            out.update(cols=cols[:row0[-1]], ins=ins[:row0[-1]], row0=row0)
        return out

    def planes_insert_window_variants(self, rlen, seg_of_pair, query, base, qpos, sites, keys, min_depth=3, pre_key=None, pre_mask=None, pre_full=None, agree=True,
                                      cap=None, site_off=None, **rule):
        """ioc_planes_insert_window_variants: planes_insert_windows with the voters of every kept site split in two where they are two
        exons, on the device — its arguments, pre_key / pre_mask per pair and pre_full per segment (the block stage's: all three or
        none), and min_agree, min_alt and min_pct beside the window rule as keywords (VARIANTS_RULE has the defaults).  Returns a dict:
        `win` (INSERT_WINDOW_DTYPE) and `var` (WINDOW_VARIANT_DTYPE; template_pair_b is the pair) per site; `seq`, `qual` and `polish`
        per slot (2 x: site x's variant A, 2 x + 1: its B, empty where the site does not split) with `off`; `variant` (n_pairs x 32
        bytes, WINVAR_*: byte k the pair's variant at site k of its segment) and, with agree=True, `agree` (n_pairs x 32 x 2,
        NO_AGREEMENT where a round did not align the pair); `reads` (READ_VARIANTS_DTYPE: key2 and the isoform counted again) and `seg`
        (VARIANTS_SEG_DTYPE)."""
        w, v = _variants_rule(rule)
        ns, n = len(rlen), len(base)
        rl, sop, qy, ky = (np.ascontiguousarray(x, t) for x, t in ((rlen, np.int32), (seg_of_pair, np.int32), (query, np.int32), (keys, np.uint64)))
        if sop.shape != (n,) or qy.shape != (n,) or ky.shape != (n,) or len(qpos) != n:
            raise ValueError("seg_of_pair, query, keys, base and qpos must hold one entry per pair")
        want = [int(rl[g]) + 1 if 0 <= g < ns else 0 for g in sop]
        for i in range(n):
            if np.shape(base[i]) != (want[i],) or np.shape(qpos[i]) != (want[i],):
                raise ValueError(f"the planes of pair {i} are not those of its segment")
        fb = np.ascontiguousarray(np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(b, np.uint8) for b in base]))
        fq = np.ascontiguousarray(np.concatenate([np.zeros(0, np.uint32)] + [np.asarray(b, np.uint32) for b in qpos]))
        if site_off is None:
            soff = np.concatenate([[0], np.cumsum([len(s) for s in sites])]).astype(np.int64)
            st = np.ascontiguousarray(np.concatenate([np.zeros(0, PILE_INSERT_DTYPE)] + [np.asarray(s, PILE_INSERT_DTYPE) for s in sites]))
        else:
            soff, st = np.ascontiguousarray(site_off, np.int64), np.ascontiguousarray(sites, PILE_INSERT_DTYPE)
        if soff.shape != (ns + 1,):
            raise ValueError("the sites must hold one array per segment")
        pre = [None if x is None else np.ascontiguousarray(x, np.uint64) for x in (pre_key, pre_mask, pre_full)]
        if any(x is not None for x in pre) and (any(x is None for x in pre) or pre[0].shape != (n,) or pre[1].shape != (n,) or pre[2].shape != (ns,)):
            raise ValueError("pre_key and pre_mask per pair and pre_full per segment: all three or none")
        S = max(int(soff[-1]), 0)
        cap = insert_window_variants_bound(S, w[1]) if cap is None else int(cap)
        win, var = np.zeros(max(S, 1), INSERT_WINDOW_DTYPE), np.zeros(max(S, 1), WINDOW_VARIANT_DTYPE)
        off, pol = np.zeros(2 * S + 1, np.int64), np.zeros(max(2 * S, 1), POLISH_STATS_DTYPE)
        seq, qual = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint8)
        variant, agr = np.zeros((max(n, 1), _lib.INSERTS_MAX), np.uint8), np.zeros((max(n, 1), _lib.INSERTS_MAX, 2), np.int32)
        reads, seg = np.zeros(max(n, 1), READ_VARIANTS_DTYPE), np.zeros(max(ns, 1), VARIANTS_SEG_DTYPE)
        pad = lambda a: np.concatenate([a, np.zeros(1, a.dtype)])  # (never an empty array's pointer)
        st, ky, qy, sop, fb, fq = (pad(x) for x in (st, ky, qy, sop, fb, fq))
        pre = [None if x is None else pad(x) for x in pre]
        self._chk(self.L.ioc_planes_insert_window_variants(self.h, ns, _p(rl, C.c_int32) if ns else None, n, _p(sop, C.c_int32), _p(qy, C.c_int32), fb.ctypes.data,
                                                           fq.ctypes.data, st.ctypes.data, _p(soff, C.c_int64), ky.ctypes.data, *w, int(min_depth), *v,
                                                           *(None if x is None else x.ctypes.data for x in pre), win.ctypes.data, var.ctypes.data,
                                                           seq.ctypes.data, qual.ctypes.data, cap, _p(off, C.c_int64), pol.ctypes.data, variant.ctypes.data,
                                                           agr.ctypes.data if agree else None, reads.ctypes.data, seg.ctypes.data))
        out = {"win": win[:S], "var": var[:S], "seq": [seq[off[x]:off[x + 1]].tobytes() for x in range(2 * S)],
               "qual": [qual[off[x]:off[x + 1]].tobytes() for x in range(2 * S)], "off": off, "polish": pol[:2 * S], "variant": variant[:n], "reads": reads[:n],
               "seg": seg[:ns]}
        if agree:
            out["agree"] = agr[:n]
        return out

    def align_pairs_blocks_inserts_seq(self, pairs, k, segs, seg_of_pair, stats=False, tables=False, rows=True, cap=None, sites_cap=None, win_cap=None, match=2,
                                       mismatch=-2, gap_extend=1, min_ins=INSERTS_RULE["min_ins"], slack=INSERTS_RULE["slack"],
                                       max_sites=INSERTS_RULE["max_sites"], max_win=WIN_MAX, win_match=WINDOWS_RULE["match"],
                                       win_mismatch=WINDOWS_RULE["mismatch"], win_gap=WINDOWS_RULE["gap"], polish_min_depth=3, _full=None, _variants=None, **rule):
        """ioc_align_pairs_blocks_inserts_seq: align_pairs_blocks_inserts with every pair's position plane projected as well and the
        window kernels behind the insert kernels, on the device, every pair aligned once.  Returns align_pairs_blocks_inserts' dict,
        byte for byte, and under `insert_windows` what Context.planes_insert_windows returns (without tables) for the sites kept."""
        f = self._blocks_family(pairs, k, segs, seg_of_pair, rule, stats, tables, rows, cap, match, mismatch, gap_extend)
        n, ns, rlen, sop = f.n, f.ns, f.rlen, f.sop
        ir = [int(min_ins), int(slack), f.r[1], f.r[2], f.r[3], int(max_sites)]
        (itab, sites, soff, iseg), sites_cap = self._inserts_out(ns, rlen, ir, rows, sites_cap)
        ireads = np.zeros(n, READ_INSERTS_DTYPE)
        S = sum(planes_inserts_bound(m, ir[5]) for m in rlen)
        win_cap = insert_windows_bound(S, max_win) if win_cap is None else int(win_cap)
        wrec, woff, wpol = np.zeros(max(S, 1), INSERT_WINDOW_DTYPE), np.zeros(S + 1, np.int64), np.zeros(max(S, 1), POLISH_STATS_DTYPE)
        wseq, wqual = np.zeros(max(win_cap, 1), np.uint8), np.zeros(max(win_cap, 1), np.uint8)
        entry, more = self.L.ioc_align_pairs_blocks_inserts_seq, ()
        if _full is not None:   # (align_pairs_isoforms_full: the same call with the isoforms' outputs behind it)
            n_reads = np.bincount(sop[(sop >= 0) & (sop < ns)], minlength=ns) if n else np.zeros(ns, np.int64)
            fb = isoforms_full_bound(rlen, n_reads, _full["max_iso"], ir[5], max_win)
            f_cap, f_iso, f_rec = (fb[x] if _full[c] is None else int(_full[c]) for x, c in enumerate(("cap", "iso_cap", "splice_cap")))
            f_seq, f_qual = np.zeros(max(f_cap, 1), np.uint8), np.zeros(max(f_cap, 1), np.uint8)
            f_off, f_spoff, f_ioff = np.zeros(max(f_iso, 0) + 1, np.int64), np.zeros(max(f_iso, 0) + 1, np.int64), np.zeros(ns + 1, np.int64)
            f_pol, f_sst = np.zeros(max(f_iso, 1), POLISH_STATS_DTYPE), np.zeros(max(f_iso, 1), SPLICE_STATS_DTYPE)
            f_splice = np.zeros(max(f_rec, 1), SPLICE_SITE_DTYPE)
            entry = self.L.ioc_align_pairs_isoforms_full
            more_full = more = (int(_full["max_iso"]), f_seq.ctypes.data, f_qual.ctypes.data, f_cap, _p(f_off, C.c_int64), f_pol.ctypes.data, f_sst.ctypes.data,
                                f_splice.ctypes.data, f_rec, _p(f_spoff, C.c_int64), f_iso, _p(f_ioff, C.c_int64))
        if _variants is not None:   # (align_pairs_blocks_inserts_variants: the same call with the variants' outputs behind it)
            v_cap = insert_window_variants_bound(S, max_win) if _variants["cap"] is None else int(_variants["cap"])
            v_var, v_off, v_pol = np.zeros(max(S, 1), WINDOW_VARIANT_DTYPE), np.zeros(2 * S + 1, np.int64), np.zeros(max(2 * S, 1), POLISH_STATS_DTYPE)
            v_seq, v_qual = np.zeros(max(v_cap, 1), np.uint8), np.zeros(max(v_cap, 1), np.uint8)
            v_variant, v_agree = np.zeros((max(n, 1), _lib.INSERTS_MAX), np.uint8), np.zeros((max(n, 1), _lib.INSERTS_MAX, 2), np.int32)
            v_reads, v_seg = np.zeros(max(n, 1), READ_VARIANTS_DTYPE), np.zeros(max(ns, 1), VARIANTS_SEG_DTYPE)
            entry = self.L.ioc_align_pairs_blocks_inserts_variants
            more = (int(_variants["min_agree"]), v_var.ctypes.data, v_seq.ctypes.data, v_qual.ctypes.data, v_cap, _p(v_off, C.c_int64), v_pol.ctypes.data,
                    v_variant.ctypes.data, v_agree.ctypes.data, v_reads.ctypes.data, v_seg.ctypes.data)
            if _full is not None:   # (align_pairs_isoforms_full_variants: both, the variants' outputs first)
                entry, more = self.L.ioc_align_pairs_isoforms_full_variants, more + more_full
        self._chk(entry(*f.lead, ir[0], ir[1], ir[5], itab.ctypes.data if rows and len(itab) else None, sites.ctypes.data, sites_cap, _p(soff, C.c_int64),
                        ireads.ctypes.data if n else None, iseg.ctypes.data if ns else None, int(max_win), int(win_match), int(win_mismatch), int(win_gap),
                        int(polish_min_depth), wrec.ctypes.data, wseq.ctypes.data, wqual.ctypes.data, win_cap, _p(woff, C.c_int64), wpol.ctypes.data, *more))
        kept = int(soff[ns]) if ns else 0
        made = {"inserts": self._inserts_dict(ns, rlen, itab, sites, soff, ireads, iseg),
                "insert_windows": self._windows_dict(wrec[:kept], wseq, wqual, woff[:kept + 1], wpol[:kept])}
        if _variants is not None:
            made["insert_variants"] = {"win": wrec[:kept], "var": v_var[:kept], "seq": [v_seq[v_off[x]:v_off[x + 1]].tobytes() for x in range(2 * kept)],
                                       "qual": [v_qual[v_off[x]:v_off[x + 1]].tobytes() for x in range(2 * kept)], "off": v_off[:2 * kept + 1], "polish": v_pol[:2 * kept],
                                       "variant": v_variant[:n], "agree": v_agree[:n], "reads": v_reads[:n], "seg": v_seg[:ns]}
        if _full is not None:
            G = int(f_ioff[ns])
            made["isoforms_full"] = {**self._groups_out(f_ioff, f_seq, f_qual, f_off, f_pol[:G]), "off": f_off[:G + 1], "sstats": f_sst[:G],
                                     "splice": [f_splice[int(f_spoff[x]):int(f_spoff[x + 1])] for x in range(G)], "splice_off": f_spoff[:G + 1]}
        return self._blocks_family_out(f, **made)

    def align_pairs_blocks_inserts_variants(self, pairs, k, segs, seg_of_pair, min_agree=VARIANTS_RULE["min_agree"], var_cap=None, **kw):
        """ioc_align_pairs_blocks_inserts_variants: align_pairs_blocks_inserts_seq with the variant kernels behind the window kernels —
        two exons at one junction told apart, every read re-keyed and the isoforms counted again, every pair aligned once.  Returns
        align_pairs_blocks_inserts_seq's dict, byte for byte, and under `insert_variants` what Context.planes_insert_window_variants
        returns for the sites kept, the block stage's keys serving as pre_*; min_alt and min_pct are the searches'."""
        return self.align_pairs_blocks_inserts_seq(pairs, k, segs, seg_of_pair, _variants=dict(min_agree=min_agree, cap=var_cap), **kw)

    def align_pairs_isoforms_full(self, pairs, k, segs, seg_of_pair, max_iso=16, full_cap=None, iso_cap=None, splice_cap=None, **kw):
        """ioc_align_pairs_isoforms_full: align_pairs_blocks_inserts_seq with the six slot planes projected as well and, behind the
        window kernels, the consensus of the first min(n_groups, max_iso) COMBINED isoforms of every segment with the windows of the
        sites each carries spliced in — every isoform's full-length sequence from one alignment of every read.  Returns
        align_pairs_blocks_inserts_seq's dict, byte for byte, and under `isoforms_full` what Context.planes_isoforms_full returns
        (without tables; `gseg_off` is iso_off).  polish_min_depth serves the windows and the isoforms; full_cap, iso_cap and
        splice_cap default to isoforms_full_bound of the segments."""
        return self.align_pairs_blocks_inserts_seq(pairs, k, segs, seg_of_pair, _full=dict(max_iso=max_iso, cap=full_cap, iso_cap=iso_cap, splice_cap=splice_cap), **kw)

    def align_pairs_isoforms_full_variants(self, pairs, k, segs, seg_of_pair, max_iso=16, min_agree=VARIANTS_RULE["min_agree"], var_cap=None, full_cap=None,
                                           iso_cap=None, splice_cap=None, **kw):
        """ioc_align_pairs_isoforms_full_variants: align_pairs_blocks_inserts_variants and align_pairs_isoforms_full in one fused call —
        the isoforms are those the variant stage counted again, each keyed by key2 of its lowest-numbered direct read, and every
        carried site's window is the slot of the variant the isoform holds there.  Returns align_pairs_blocks_inserts_variants' dict,
        byte for byte, and `isoforms_full` as align_pairs_isoforms_full shapes it; full_cap, iso_cap and splice_cap default to
        isoforms_full_bound of the segments."""
        return self.align_pairs_blocks_inserts_seq(pairs, k, segs, seg_of_pair, _variants=dict(min_agree=min_agree, cap=var_cap),
                                                   _full=dict(max_iso=max_iso, cap=full_cap, iso_cap=iso_cap, splice_cap=splice_cap), **kw)

    def align_pairs_blocks(self, pairs, k, segs, seg_of_pair, stats=False, tables=False, rows=True, cap=None, match=2, mismatch=-2, gap_extend=1, **rule):
        """ioc_align_pairs_blocks: align_pairs, the table of counts, every pair's base plane and the block search over the planes, all
        on the device, every pair aligned once — segs / seg_of_pair as for align_pairs_alleles; the rule as keywords.  Returns a dict:
        score, windows, ratio, and `blocks`, `block_off`, `reads`, `seg`, `rows` as Context.planes_blocks returns them; with stats=True
        `stats` (ALN_STATS_DTYPE per pair), with tables=True `cols` and `row0`."""
        f = self._blocks_family(pairs, k, segs, seg_of_pair, rule, stats, tables, rows, cap, match, mismatch, gap_extend)
        self._chk(self.L.ioc_align_pairs_blocks(*f.lead))
        return self._blocks_family_out(f)

    @staticmethod
    def _ends_out(ns, rlen, n_reads, rule, rows, sites_cap, variants_cap):
        """the output arrays of a search for ends over segments of these lengths and read counts"""
        bounds = [reads_ends_bound(m, k, rule[5], rule[6]) for m, k in zip(rlen, n_reads)]
        sites_cap = sum(b[0] for b in bounds) if sites_cap is None else int(sites_cap)
        variants_cap = sum(b[1] for b in bounds) if variants_cap is None else int(variants_cap)
        tab = np.zeros(int(sum(rlen)) + ns, END_ROW_DTYPE) if rows else None
        sites, soff = np.zeros(max(sites_cap, 1), END_SITE_DTYPE), np.zeros(2 * ns + 1, np.int64)
        variants, voff, seg = np.zeros(max(variants_cap, 1), END_VARIANT_DTYPE), np.zeros(ns + 1, np.int64), np.zeros(ns, ENDS_SEG_DTYPE)
        return (tab, sites, soff, variants, voff, seg), sites_cap, variants_cap

    def _ends_dict(self, ns, rlen, tab, sites, soff, variants, voff, reads, seg):
        out = {"starts": [sites[soff[2 * g]:soff[2 * g + 1]] for g in range(ns)], "stops": [sites[soff[2 * g + 1]:soff[2 * g + 2]] for g in range(ns)],
               "site_off": soff, "variants": [variants[voff[g]:voff[g + 1]] for g in range(ns)], "var_off": voff, "reads": reads, "seg": seg}
        if tab is not None:
            r0 = np.concatenate([self._row0(rlen), [len(tab)]]).astype(np.int64) if ns else np.zeros(1, np.int64)
            out.update(rows=[tab[r0[g]:r0[g + 1]] for g in range(ns)])
        return out

    def reads_ends(self, rlen, seg_of_pair, extents, pre_group=None, rows=True, sites_cap=None, variants_cap=None, **rule):
        """ioc_reads_ends: the alternative ends of many segments on the device, from host arrays — `rlen` the segments' lengths,
        seg_of_pair and `extents` (READ_EXTENT_DTYPE) per pair, pre_group per pair or None; the rule as keywords.  Returns a dict:
        `starts`, `stops` (an END_SITE_DTYPE array per segment each), `site_off`, `variants` (an END_VARIANT_DTYPE array per segment),
        `var_off`, `reads` (READ_ENDS_DTYPE per pair), `seg` (ENDS_SEG_DTYPE per segment) and, with rows=True, `rows` (an
        END_ROW_DTYPE array per segment); each segment as api.host_reads_ends defines it."""
        ext = _extents(extents)
        ns, n = len(rlen), len(ext)
        rl = np.ascontiguousarray(rlen, np.int32)
        sop = np.ascontiguousarray(seg_of_pair, np.int32)
        if sop.shape != (n,):
            raise ValueError("seg_of_pair and extents must hold one entry per pair")
        pg = None
        if pre_group is not None:
            pg = np.ascontiguousarray(pre_group, np.int32)
            if pg.shape != (n,):
                raise ValueError("pre_group must hold one entry per pair")
            pg = np.concatenate([pg, np.zeros(1, np.int32)])  # (never an empty array's pointer)
        r = _ends_rule(rule)
        counts = np.bincount(sop[(sop >= 0) & (sop < ns)], minlength=ns) if ns else []
        (tab, sites, soff, variants, voff, seg), sites_cap, variants_cap = self._ends_out(ns, [max(int(m), 0) for m in rl], counts, r, rows, sites_cap, variants_cap)
        reads = np.zeros(n, READ_ENDS_DTYPE)
        self._chk(self.L.ioc_reads_ends(self.h, ns, _p(rl, C.c_int32) if ns else None, n, _p(sop, C.c_int32) if n else None, ext.ctypes.data if n else None,
                                        pg.ctypes.data if pg is not None else None, *r, tab.ctypes.data if rows and len(tab) else None, sites.ctypes.data,
                                        sites_cap, _p(soff, C.c_int64), variants.ctypes.data, variants_cap, _p(voff, C.c_int64),
                                        reads.ctypes.data if n else None, seg.ctypes.data if ns else None))
        return self._ends_dict(ns, [int(m) for m in rl], tab, sites, soff, variants, voff, reads, seg)

    def align_pairs_blocks_ends(self, pairs, k, segs, seg_of_pair, stats=False, tables=False, rows=True, cap=None, sites_cap=None, variants_cap=None, match=2,
                                mismatch=-2, gap_extend=1, slack=ENDS_RULE["slack"], min_over=ENDS_RULE["min_over"], ends_min_pct=ENDS_RULE["min_pct"],
                                max_sites=ENDS_RULE["max_sites"], max_variants=ENDS_RULE["max_variants"], **rule):
        """ioc_align_pairs_blocks_ends: align_pairs_blocks with the search for ends behind the block search, on the device, every
        pair aligned once — the block rule as keywords, slack / min_over / ends_min_pct / max_sites / max_variants for the ends
        (min_depth and min_alt are shared), pre_group being the block stage's isoform.  Returns align_pairs_blocks' dict, byte for
        byte, `extents` (READ_EXTENT_DTYPE per pair) and under `ends` what Context.reads_ends returns."""
        f = self._blocks_family(pairs, k, segs, seg_of_pair, rule, stats, tables, rows, cap, match, mismatch, gap_extend)
        n, ns, rlen = f.n, f.ns, f.rlen
        er = [int(slack), int(min_over), f.r[1], f.r[2], int(ends_min_pct), int(max_sites), int(max_variants)]
        sopa = np.asarray(f.sop, np.int64)
        counts = np.bincount(sopa[(sopa >= 0) & (sopa < ns)], minlength=ns) if ns else []
        (etab, sites, soff, variants, voff, eseg), sites_cap, variants_cap = self._ends_out(ns, rlen, counts, er, rows, sites_cap, variants_cap)
        ereads, ext = np.zeros(n, READ_ENDS_DTYPE), np.zeros(n, READ_EXTENT_DTYPE)
        self._chk(self.L.ioc_align_pairs_blocks_ends(*f.lead, er[0], er[1], er[4], er[5], er[6], ext.ctypes.data if n else None,
                                                     etab.ctypes.data if rows and len(etab) else None, sites.ctypes.data, sites_cap, _p(soff, C.c_int64),
                                                     variants.ctypes.data, variants_cap, _p(voff, C.c_int64), ereads.ctypes.data if n else None,
                                                     eseg.ctypes.data if ns else None))
        return self._blocks_family_out(f, extents=ext, ends=self._ends_dict(ns, rlen, etab, sites, soff, variants, voff, ereads, eseg))

    @staticmethod
    def _groups_out(goff, seq, qual, off, pol):
        """The flat outputs of a call over goff[g] .. goff[g + 1] group-segments of segment g as per-segment lists: `gseq` and
        `gqual` (a list of bytes per group), `gpolish` (a POLISH_STATS_DTYPE array per segment), `gseg_off`."""
        ns = len(goff) - 1
        cut = lambda a, g: [a[off[x]:off[x + 1]].tobytes() for x in range(int(goff[g]), int(goff[g + 1]))]
        return {"gseq": [cut(seq, g) for g in range(ns)], "gqual": [cut(qual, g) for g in range(ns)],
                "gpolish": [pol[int(goff[g]):int(goff[g + 1])] for g in range(ns)], "gseg_off": goff}

    def planes_polish_groups(self, frames, seg_of_pair, group, n_groups, base, slots, min_depth=3, tables=False, cap=None):
        """ioc_planes_polish_groups: the consensus of every group of every segment on the device, from host planes — as
        planes_polish, with n_groups[g] groups of segment g and group[i] in -1 .. n_groups[seg_of_pair[i]] - 1 (-1: in no table).
        Returns a dict: `gseq` and `gqual` (per segment a list of bytes per group), `gpolish` (per segment a POLISH_STATS_DTYPE array,
        a record per group), `gseg_off` (segment g's group-segments are gseg_off[g] .. gseg_off[g + 1]) and, with tables=True,
        `gcols` and `gins` (rlen + 1 rows per group-segment, in group-segment order) and `grow0` (the first row of every
        group-segment) — each group-segment as pileup_call defines it on the tables planes_pile adds up from the group's reads."""
        ns, n = len(frames), len(base)
        rlen = np.array([len(f) for f in frames], np.int32)
        sop, grp, ng = np.ascontiguousarray(seg_of_pair, np.int32), np.ascontiguousarray(group, np.int32), np.ascontiguousarray(n_groups, np.int32)
        if sop.shape != (n,) or grp.shape != (n,) or len(slots) != n or ng.shape != (ns,):
            raise ValueError("seg_of_pair, group, base and slots must hold one entry per pair and n_groups one per segment")
        rows = [int(rlen[g]) + 1 if 0 <= g < ns else 0 for g in sop]
        for i in range(n):
            if np.shape(base[i]) != (rows[i],) or np.shape(slots[i]) != (_lib.PILE_INS_SLOTS, rows[i]):
                raise ValueError(f"the planes of pair {i} are not those of its segment")
        P = sum(rows)
        fb = np.ascontiguousarray(np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(b, np.uint8) for b in base]))
        fs = np.ascontiguousarray(np.concatenate([np.zeros((_lib.PILE_INS_SLOTS, 0), np.uint8)] + [np.asarray(x, np.uint8) for x in slots], axis=1))
        f_off = np.zeros(ns + 1, np.int64)
        np.cumsum(rlen, out=f_off[1:])
        groups = np.maximum(ng.astype(np.int64), 0)   # (a negative count: the library refuses the call)
        goff = np.concatenate([[0], np.cumsum(groups)]).astype(np.int64)
        G = int(goff[-1])
        bound = sum(int(groups[g]) * pileup_call_bound(rlen[g]) for g in range(ns))
        cap = bound if cap is None else int(cap)
        per = np.repeat(rlen.astype(np.int64) + 1, groups)
        n_rows = int(per.sum())
        seq, qual = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint8)
        off, pol = np.zeros(G + 1, np.int64), np.zeros(G, POLISH_STATS_DTYPE)
        gcols, gins = (np.zeros(n_rows, PILEUP_DTYPE), np.zeros(n_rows, PILEUP_INS_DTYPE)) if tables else (None, None)
        self._chk(self.L.ioc_planes_polish_groups(self.h, ns, _p(rlen, C.c_int32) if ns else None, b"".join(bytes(f) for f in frames), _p(f_off, C.c_int64),
                                                  _p(ng, C.c_int32) if ns else None, n, _p(sop, C.c_int32) if n else None, _p(grp, C.c_int32) if n else None,
                                                  fb.ctypes.data if P else None, fs.ctypes.data if P else None, int(min_depth), seq.ctypes.data,
                                                  qual.ctypes.data, cap, _p(off, C.c_int64), pol.ctypes.data if G else None,
                                                  gcols.ctypes.data if tables and n_rows else None, gins.ctypes.data if tables and n_rows else None))
        out = self._groups_out(goff, seq, qual, off, pol)
        if tables:
            out.update(gcols=gcols, gins=gins, grow0=np.concatenate([[0], np.cumsum(per)])[:G].astype(np.int64))
        return out

    def planes_isoforms_full(self, frames, seg_of_pair, group, n_groups, base, slots, iso_key, win, win_seq, win_qual, min_depth=3, tables=False, cap=None,
                             splice_cap=None, _var=None):
        """ioc_planes_isoforms_full: the full-length sequence of every group of every segment on the device, from host planes —
        planes_polish_groups with, per group-segment, `iso_key` (the insert key of its direct reads, group-segment order) and, per
        segment, `win` (an INSERT_WINDOW_DTYPE array, a record per kept site) and `win_seq` / `win_qual` (a list of bytes per site) as
        planes_insert_windows returned them.  Returns planes_polish_groups' dict and `off`, `sstats` (SPLICE_STATS_DTYPE per
        group-segment), `splice` (per group-segment a SPLICE_SITE_DTYPE array, a record per site of its segment) and `splice_off` —
        each group-segment as isoform_splice defines it on the tables planes_pile adds up from the group's reads."""
        ns, n = len(frames), len(base)
        per_site = 1 if _var is None else 2   # (planes_isoforms_full_variants: win_seq / win_qual hold two slots a site)
        rlen = np.array([len(f) for f in frames], np.int32)
        sop, grp, ng = np.ascontiguousarray(seg_of_pair, np.int32), np.ascontiguousarray(group, np.int32), np.ascontiguousarray(n_groups, np.int32)
        if sop.shape != (n,) or grp.shape != (n,) or len(slots) != n or ng.shape != (ns,) or len(win) != ns or len(win_seq) != ns or len(win_qual) != ns:
            raise ValueError("seg_of_pair, group, base and slots must hold one entry per pair and n_groups, win, win_seq and win_qual one per segment")
        rows = [int(rlen[g]) + 1 if 0 <= g < ns else 0 for g in sop]
        for i in range(n):
            if np.shape(base[i]) != (rows[i],) or np.shape(slots[i]) != (_lib.PILE_INS_SLOTS, rows[i]):
                raise ValueError(f"the planes of pair {i} are not those of its segment")
        P = sum(rows)
        fb = np.ascontiguousarray(np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(b, np.uint8) for b in base]))
        fs = np.ascontiguousarray(np.concatenate([np.zeros((_lib.PILE_INS_SLOTS, 0), np.uint8)] + [np.asarray(x, np.uint8) for x in slots], axis=1))
        f_off = np.zeros(ns + 1, np.int64)
        np.cumsum(rlen, out=f_off[1:])
        groups = np.maximum(ng.astype(np.int64), 0)   # (a negative count: the library refuses the call)
        goff = np.concatenate([[0], np.cumsum(groups)]).astype(np.int64)
        G = int(goff[-1])
        keys = np.ascontiguousarray(iso_key, np.uint64)
        if keys.shape != (G,):
            raise ValueError("iso_key must hold one key per group-segment")
        for g in range(ns):
            if len(win_seq[g]) != per_site * len(win[g]) or len(win_qual[g]) != per_site * len(win[g]) or any(len(s) != len(q) for s, q in zip(win_seq[g], win_qual[g])):
                raise ValueError(f"the windows of segment {g} are not one sequence and one string of qualities per site")
        n_sites = np.array([len(w) for w in win], np.int64)
        soff = np.concatenate([[0], np.cumsum(n_sites)]).astype(np.int64)
        S = int(soff[-1])
        wrec = np.ascontiguousarray(np.concatenate([np.zeros(0, INSERT_WINDOW_DTYPE)] + [np.asarray(w, INSERT_WINDOW_DTYPE) for w in win]))
        flat = [bytes(s) for g in range(ns) for s in win_seq[g]]
        woff = np.concatenate([[0], np.cumsum([len(s) for s in flat])]).astype(np.int64)
        wseq, wqual = b"".join(flat), b"".join(bytes(q) for g in range(ns) for q in win_qual[g])
        wbytes = [int(woff[per_site * soff[g + 1]] - woff[per_site * soff[g]]) for g in range(ns)]
        bound = sum(int(groups[g]) * isoform_splice_bound(rlen[g], wbytes[g]) for g in range(ns))
        cap = bound if cap is None else int(cap)
        R = int((groups * n_sites).sum())
        splice_cap = R if splice_cap is None else int(splice_cap)
        per = np.repeat(rlen.astype(np.int64) + 1, groups)
        n_rows = int(per.sum())
        seq, qual = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint8)
        off, pol, sst = np.zeros(G + 1, np.int64), np.zeros(max(G, 1), POLISH_STATS_DTYPE), np.zeros(max(G, 1), SPLICE_STATS_DTYPE)
        rec, spoff = np.zeros(max(splice_cap, 1), SPLICE_SITE_DTYPE), np.zeros(G + 1, np.int64)
        gcols, gins = (np.zeros(n_rows, PILEUP_DTYPE), np.zeros(n_rows, PILEUP_INS_DTYPE)) if tables else (None, None)
        pad = lambda a: np.concatenate([a, np.zeros(1, a.dtype)])  # (never an empty array's pointer)
        keys, wrec = pad(keys), pad(wrec)
        entry, var_arg = self.L.ioc_planes_isoforms_full, ()
        if _var is not None:
            if len(_var) != ns or any(len(_var[g]) != len(win[g]) for g in range(ns)):
                raise ValueError("var must hold a record per site of every segment")
            vrec = pad(np.ascontiguousarray(np.concatenate([np.zeros(0, WINDOW_VARIANT_DTYPE)] + [np.asarray(v, WINDOW_VARIANT_DTYPE) for v in _var])))
            entry, var_arg = self.L.ioc_planes_isoforms_full_variants, (vrec.ctypes.data,)
        self._chk(entry(self.h, ns, _p(rlen, C.c_int32) if ns else None, b"".join(bytes(f) for f in frames), _p(f_off, C.c_int64),
                                                  _p(ng, C.c_int32) if ns else None, n, _p(sop, C.c_int32) if n else None, _p(grp, C.c_int32) if n else None,
                                                  fb.ctypes.data if P else None, fs.ctypes.data if P else None, keys.ctypes.data, wrec.ctypes.data, *var_arg,
                                                  _p(soff, C.c_int64), wseq, wqual, _p(woff, C.c_int64), int(min_depth), seq.ctypes.data, qual.ctypes.data, cap,
                                                  _p(off, C.c_int64), pol.ctypes.data, sst.ctypes.data, rec.ctypes.data, splice_cap, _p(spoff, C.c_int64),
                                                  gcols.ctypes.data if tables and n_rows else None, gins.ctypes.data if tables and n_rows else None))
        out = self._groups_out(goff, seq, qual, off, pol[:G])
        out.update(off=off, sstats=sst[:G], splice=[rec[int(spoff[x]):int(spoff[x + 1])] for x in range(G)], splice_off=spoff)
        if tables:
            out.update(gcols=gcols, gins=gins, grow0=np.concatenate([[0], np.cumsum(per)])[:G].astype(np.int64))
        return out

    def planes_isoforms_full_variants(self, frames, seg_of_pair, group, n_groups, base, slots, iso_key, win, var, slot_seq, slot_qual, min_depth=3, tables=False,
                                      cap=None, splice_cap=None):
        """ioc_planes_isoforms_full_variants: planes_isoforms_full by variant — `iso_key` holds a key2 per group-segment, `var` per
        segment a WINDOW_VARIANT_DTYPE array beside `win`, and slot_seq / slot_qual per segment a list of bytes per SLOT (2 b: site b's
        variant A, 2 b + 1: its B) as planes_insert_window_variants returned them.  Returns planes_isoforms_full's dict, each
        group-segment as isoform_splice_variants defines it."""
        return self.planes_isoforms_full(frames, seg_of_pair, group, n_groups, base, slots, iso_key, win, slot_seq, slot_qual, min_depth=min_depth, tables=tables,
                                         cap=cap, splice_cap=splice_cap, _var=var)

    def align_pairs_blocks_polish(self, pairs, k, segs, seg_of_pair, max_iso=16, polish_min_depth=3, stats=False, tables=False, rows=True, cap=None,
                                  polish_cap=None, iso_cap=None, match=2, mismatch=-2, gap_extend=1, _entry="ioc_align_pairs_blocks_polish", **rule):
        """ioc_align_pairs_blocks_polish: align_pairs_blocks with the consensus of the first min(n_groups, max_iso) isoforms of every
        segment called from the reads' planes where they lie — no read is aligned a second time.  Returns align_pairs_blocks' dict
        plus `gseq`, `gqual`, `gpolish` and `gseg_off` as planes_polish_groups returns them: isoform h of segment g from its direct
        and assigned reads, against the segment's frame.  polish_cap / iso_cap default to the bounds (blocks_polish_bound)."""
        f = self._blocks_family(pairs, k, segs, seg_of_pair, rule, stats, tables, rows, cap, match, mismatch, gap_extend)
        ns, rlen, sop = f.ns, f.rlen, f.sop
        count = np.bincount(sop[(sop >= 0) & (sop < ns)], minlength=ns) if ns else np.zeros(0, np.int64)
        bounds = [blocks_polish_bound(rlen[g], count[g], max(int(max_iso), 0)) for g in range(ns)]
        i_cap = sum(b[0] for b in bounds) if iso_cap is None else int(iso_cap)
        p_cap = sum(b[1] for b in bounds) if polish_cap is None else int(polish_cap)
        seq, qual = np.zeros(max(p_cap, 1), np.uint8), np.zeros(max(p_cap, 1), np.uint8)
        off, pol, goff = np.zeros(max(i_cap, 0) + 1, np.int64), np.zeros(max(i_cap, 1), POLISH_STATS_DTYPE), np.zeros(ns + 1, np.int64)
        self._chk(getattr(self.L, _entry)(*f.lead, int(max_iso), int(polish_min_depth), seq.ctypes.data, qual.ctypes.data, p_cap, _p(off, C.c_int64), pol.ctypes.data,
                                          i_cap, _p(goff, C.c_int64)))
        return self._blocks_family_out(f, **self._groups_out(goff, seq, qual, off, pol))

    def align_pairs_blocks_correct(self, pairs, k, segs, seg_of_pair, correct_min_depth=3, correct_min_alt=3, correct_min_pct=25, correct_max_run=10, stats=False,
                                   tables=False, rows=True, cap=None, correct_cap=None, match=2, mismatch=-2, gap_extend=1, **rule):
        """ioc_align_pairs_blocks_correct: align_pairs_blocks with every read corrected against the tables of its own isoform — the
        block search's group — from the planes where they lie; no read is aligned a second time.  Returns align_pairs_blocks' dict
        plus `seq` and `qual` (lists of bytes per PAIR) and `correct` (ISO_CORRECT_STATS_DTYPE per pair) as planes_correct_groups
        returns them.  correct_cap defaults to the bound: every pair's segment bound and its query's length."""
        f = self._blocks_family(pairs, k, segs, seg_of_pair, rule, stats, tables, rows, cap, match, mismatch, gap_extend)
        n, ns = f.n, f.ns
        bound = sum(pileup_call_bound(f.rlen[g]) for g in f.sop if 0 <= g < ns) + sum(self._pool_len(p[0]) for p in pairs)
        c_cap = bound if correct_cap is None else int(correct_cap)
        seq, qual = np.zeros(max(c_cap, 1), np.uint8), np.zeros(max(c_cap, 1), np.uint8)
        off, cor = np.zeros(n + 1, np.int64), np.zeros(n, ISO_CORRECT_STATS_DTYPE)
        self._chk(self.L.ioc_align_pairs_blocks_correct(*f.lead, int(correct_min_depth), int(correct_min_alt), int(correct_min_pct), int(correct_max_run),
                                                        seq.ctypes.data, qual.ctypes.data, c_cap, _p(off, C.c_int64), cor.ctypes.data if n else None))
        return self._blocks_family_out(f, correct=cor, seq=[seq[off[i]:off[i + 1]].tobytes() for i in range(n)],
                                       qual=[qual[off[i]:off[i + 1]].tobytes() for i in range(n)])

    def planes_polish_groups_weighted(self, frames, seg_of_pair, group, n_groups, base, slots, wbase, wslots, min_depth=3, tables=False, cap=None):
        """ioc_planes_polish_groups_weighted: planes_polish_groups with every read's vote counted by its weight — wbase / wslots the
        weight planes of every pair (ops_project_weights), laid out like base / slots.  Returns planes_polish_groups' dict; with
        tables=True `gcols` (the counts, as planes_polish_groups returns them), `gwcols` and `gwins` (the sums of weights,
        planes_pile_weighted over the group's reads) and `grow0` — each group-segment as pileup_call_weighted defines it on them."""
        ns, n = len(frames), len(base)
        rlen = np.array([len(f) for f in frames], np.int32)
        sop, grp, ng = np.ascontiguousarray(seg_of_pair, np.int32), np.ascontiguousarray(group, np.int32), np.ascontiguousarray(n_groups, np.int32)
        if sop.shape != (n,) or grp.shape != (n,) or len(slots) != n or len(wbase) != n or len(wslots) != n or ng.shape != (ns,):
            raise ValueError("seg_of_pair, group and the planes must hold one entry per pair and n_groups one per segment")
        rows = [int(rlen[g]) + 1 if 0 <= g < ns else 0 for g in sop]
        for i in range(n):
            if np.shape(base[i]) != (rows[i],) or np.shape(slots[i]) != (_lib.PILE_INS_SLOTS, rows[i]) or np.shape(wbase[i]) != (rows[i],) or \
                    np.shape(wslots[i]) != (_lib.PILE_INS_SLOTS, rows[i]):
                raise ValueError(f"the planes of pair {i} are not those of its segment")
        P = sum(rows)
        flat = lambda planes: np.ascontiguousarray(np.concatenate([np.zeros(0, np.uint8)] + [np.asarray(b, np.uint8) for b in planes]))
        flat6 = lambda planes: np.ascontiguousarray(np.concatenate([np.zeros((_lib.PILE_INS_SLOTS, 0), np.uint8)] + [np.asarray(x, np.uint8) for x in planes], axis=1))
        fb, fs, fwb, fws = flat(base), flat6(slots), flat(wbase), flat6(wslots)
        f_off = np.zeros(ns + 1, np.int64)
        np.cumsum(rlen, out=f_off[1:])
        groups = np.maximum(ng.astype(np.int64), 0)   # (a negative count: the library refuses the call)
        goff = np.concatenate([[0], np.cumsum(groups)]).astype(np.int64)
        G = int(goff[-1])
        bound = sum(int(groups[g]) * pileup_call_bound(rlen[g]) for g in range(ns))
        cap = bound if cap is None else int(cap)
        per = np.repeat(rlen.astype(np.int64) + 1, groups)
        n_rows = int(per.sum())
        seq, qual = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint8)
        off, pol = np.zeros(G + 1, np.int64), np.zeros(G, POLISH_STATS_DTYPE)
        gcols, gwcols, gwins = (np.zeros(n_rows, PILEUP_DTYPE), np.zeros(n_rows, PILEUP_DTYPE), np.zeros(n_rows, PILEUP_INS_DTYPE)) if tables else (None, None, None)
        tab = lambda a: a.ctypes.data if tables and n_rows else None
        self._chk(self.L.ioc_planes_polish_groups_weighted(self.h, ns, _p(rlen, C.c_int32) if ns else None, b"".join(bytes(f) for f in frames), _p(f_off, C.c_int64),
                                                           _p(ng, C.c_int32) if ns else None, n, _p(sop, C.c_int32) if n else None, _p(grp, C.c_int32) if n else None,
                                                           fb.ctypes.data if P else None, fs.ctypes.data if P else None, fwb.ctypes.data if P else None,
                                                           fws.ctypes.data if P else None, int(min_depth), seq.ctypes.data, qual.ctypes.data, cap, _p(off, C.c_int64),
                                                           pol.ctypes.data if G else None, tab(gcols), tab(gwcols), tab(gwins)))
        out = self._groups_out(goff, seq, qual, off, pol)
        if tables:
            out.update(gcols=gcols, gwcols=gwcols, gwins=gwins, grow0=np.concatenate([[0], np.cumsum(per)])[:G].astype(np.int64))
        return out

    def align_pairs_blocks_polish_weighted(self, pairs, k, segs, seg_of_pair, **kw):
        """ioc_align_pairs_blocks_polish_weighted: align_pairs_blocks_polish with every isoform called by weight, under the quality
        lines of align_set_pool_qual (IocError without them).  The arguments and the dict of align_pairs_blocks_polish; everything
        but `gseq`, `gqual` and `gpolish` is what that call returns."""
        return self.align_pairs_blocks_polish(pairs, k, segs, seg_of_pair, _entry="ioc_align_pairs_blocks_polish_weighted", **kw)

    @staticmethod
    def _gpolish_out(ns, rlen, seq, qual, off, pol, gcols, gins, tables):
        """The group polish's flat outputs as a dict: group-segment 2 g + h becomes entry [g][h]."""
        out = {"gseq": [[seq[off[2 * g + h]:off[2 * g + h + 1]].tobytes() for h in (0, 1)] for g in range(ns)],
               "gqual": [[qual[off[2 * g + h]:off[2 * g + h + 1]].tobytes() for h in (0, 1)] for g in range(ns)], "gpolish": pol.reshape(ns, 2)}
        if tables:
            rows = np.asarray(rlen, np.int64) + 1
            first = 2 * np.concatenate([[0], np.cumsum(rows)])[:ns]
            out.update(gcols=gcols, gins=gins, grow0=np.stack([first, first + rows], axis=1).reshape(ns, 2))
        return out

    def align_pairs_split(self, pairs, k, segs, seg_of_pair, min_depth=3, min_alt=3, min_pct=25, max_sites=4096, min_link=3, min_margin=1, rounds=2,
                          stats=False, tables=False, alleles=False, match=2, mismatch=-2, gap_extend=1):
        """ioc_align_pairs_split: align_pairs_alleles with the split of every segment's reads run where the alleles lie.  Returns
        align_pairs_alleles' dict — `alleles` only with alleles=True, `cols` and `row0` only with tables=True — and the split's:
        `link`, `phase` (lists per segment), `group`, `vote` (per pair), `seg` (SPLIT_SEG_DTYPE per segment), `members`."""
        return self._align_pairs_split(None, pairs, k, segs, seg_of_pair, min_depth, min_alt, min_pct, max_sites, min_link, min_margin, rounds, stats,
                                       tables, alleles, match, mismatch, gap_extend)

    def align_pairs_split_polish(self, pairs, k, segs, seg_of_pair, min_depth=3, min_alt=3, min_pct=25, max_sites=4096, min_link=3, min_margin=1,
                                 rounds=2, polish_min_depth=3, stats=False, tables=False, alleles=False, cap=None, match=2, mismatch=-2, gap_extend=1):
        """ioc_align_pairs_split_polish: align_pairs_split with the consensus of both groups of every segment called from the reads'
        planes where they lie — no read is aligned a second time.  Returns align_pairs_split's dict plus `gseq` and `gqual` (lists of
        [group 0, group 1] per segment), `gpolish` (POLISH_STATS_DTYPE, shape (segments, 2)) and, with tables=True, `gcols`, `gins`
        and `grow0` as planes_polish returns them.  A group without reads returns the segment's frame at quality '!'."""
        return self._align_pairs_split((int(polish_min_depth), cap), pairs, k, segs, seg_of_pair, min_depth, min_alt, min_pct, max_sites, min_link,
                                       min_margin, rounds, stats, tables, alleles, match, mismatch, gap_extend)

    def _align_pairs_split(self, polish, pairs, k, segs, seg_of_pair, min_depth, min_alt, min_pct, max_sites, min_link, min_margin, rounds, stats,
                           tables, alleles, match, mismatch, gap_extend, split=True):
        """align_pairs_split, align_pairs_split_polish with polish = (polish_min_depth, cap), and align_pairs_alleles with split=False"""
        n, ns = len(pairs), len(segs)
        arr = self._aln_pairs(pairs)
        sarr, sop, rlen, n_rows = self._seg_args(n, segs, seg_of_pair)
        sites, s_cap, s_off, found, alle, a_cap, a_off = self._site_outs(n, rlen, sop, max_sites, alleles)
        (score, win, ratio), ptrs = self._aln_out(n)
        st = np.zeros(n, ALN_STATS_DTYPE) if stats else None
        cols = np.zeros(n_rows, PILEUP_DTYPE) if tables else None
        args = (self.h, n, arr, k, match, mismatch, gap_extend, *ptrs, st.ctypes.data if stats and n else None, ns, sarr, _p(sop, C.c_int32),
                int(min_depth), int(min_alt), int(min_pct), int(max_sites), sites.ctypes.data, s_cap, _p(s_off, C.c_int64), _p(found, C.c_int64),
                alle.ctypes.data if alleles else None, a_cap if alleles else 0, _p(a_off, C.c_int64), cols.ctypes.data if tables and n_rows else None)
        out = {"score": score, "windows": win, "ratio": ratio}
        if not split:
            self._chk(self.L.ioc_align_pairs_alleles(*args))
        else:
            link, phase = np.zeros(max(s_cap, 1), np.int64), np.zeros(max(s_cap, 1), np.int8)
            group, vote, seg = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int32), np.zeros(max(ns, 1), SPLIT_SEG_DTYPE)
            args += (int(min_link), int(min_margin), int(rounds), link.ctypes.data, phase.ctypes.data, group.ctypes.data, vote.ctypes.data, seg.ctypes.data)
        if split and polish is None:
            self._chk(self.L.ioc_align_pairs_split(*args))
        elif split:
            bound = 2 * sum(pileup_call_bound(r) for r in rlen)
            g_cap = bound if polish[1] is None else int(polish[1])
            g_seq, g_qual = np.zeros(max(g_cap, 1), np.uint8), np.zeros(max(g_cap, 1), np.uint8)
            g_off, g_pol = np.zeros(2 * ns + 1, np.int64), np.zeros(2 * ns, POLISH_STATS_DTYPE)
            gcols, gins = (np.zeros(2 * n_rows, PILEUP_DTYPE), np.zeros(2 * n_rows, PILEUP_INS_DTYPE)) if tables else (None, None)
            self._chk(self.L.ioc_align_pairs_split_polish(*args, polish[0], g_seq.ctypes.data, g_qual.ctypes.data, g_cap, _p(g_off, C.c_int64),
                                                          g_pol.ctypes.data if ns else None, gcols.ctypes.data if tables and n_rows else None,
                                                          gins.ctypes.data if tables and n_rows else None))
        out.update(sites=[sites[s_off[g]:s_off[g + 1]].copy() for g in range(ns)], n_found=found[:ns])
        if split:
            out.update(self._split_out(s_off, a_off, sop, ns, n, link, phase, group, vote, seg))
        if polish is not None:
            out.update(self._gpolish_out(ns, rlen, g_seq, g_qual, g_off, g_pol, gcols, gins, tables))
        if alleles:
            out["alleles"] = [alle[a_off[i]:a_off[i + 1]].copy() for i in range(n)]
        if stats:
            out["stats"] = st
        if tables:
            out["cols"] = cols
            out["row0"] = self._row0(rlen)
        return out

    # ---- sort-stage feeders --------------------------------------------------------------------
    def qual_scores(self, offs, qual, k):
        """CalcQualScore / CalcErrorRate per read (src/qualscore.cpp:14-37, 107-154)."""
        offs = np.ascontiguousarray(offs, np.int64)
        qual = np.ascontiguousarray(qual, np.uint8)
        n = len(offs) - 1
        score, err = np.zeros(n, np.float64), np.zeros(n, np.float64)
        self._chk(self.L.ioc_qual_scores(self.h, n, _p(offs, C.c_int64), _p(qual, C.c_uint8), k,
                                         _p(score, C.c_double), _p(err, C.c_double)))
        return score, err

    def extract_minimizers(self, offs, seq, qual, k, w):
        """HomopolymerCompress + KmerEncodeSeq + GetKmerMinimizers on both strands
        (src/qualscore.cpp:39-105); the minimizers stay on the device."""
        offs = np.ascontiguousarray(offs, np.int64)
        seq = np.ascontiguousarray(seq, np.uint8)
        qual = np.ascontiguousarray(qual, np.uint8)
        n = len(offs) - 1
        hpc_len, hpc_err = np.zeros(n, np.uint32), np.zeros(n, np.float64)
        off_fwd, off_rev = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        status = np.zeros(n, np.int32)
        self._chk(self.L.ioc_extract_minimizers(self.h, n, _p(offs, C.c_int64), _p(seq, C.c_uint8),
                                                _p(qual, C.c_uint8), k, w, _p(hpc_len, C.c_uint32),
                                                _p(hpc_err, C.c_double), _p(off_fwd, C.c_int64),
                                                _p(off_rev, C.c_int64), _p(status, C.c_int32)))
        return dict(hpc_len=hpc_len, hpc_err=hpc_err, off_fwd=off_fwd, off_rev=off_rev, status=status)

    def extracted_download(self, total):
        mn, ps = np.zeros(max(total, 1), np.uint32), np.zeros(max(total, 1), np.uint32)
        self._chk(self.L.ioc_extracted_download(self.h, _p(mn, C.c_uint32), _p(ps, C.c_uint32), len(mn)))
        return mn[:total], ps[:total]

    def queries_from_extracted(self, keep, err_cell, min_total):
        keep = np.ascontiguousarray(keep, np.uint8)
        err_cell = np.ascontiguousarray(err_cell, np.uint8)
        min_total = np.ascontiguousarray(min_total, np.uint32)
        self._chk(self.L.ioc_queries_from_extracted(self.h, _p(keep, C.c_uint8), _p(err_cell, C.c_uint8),
                                                    _p(min_total, C.c_uint32)))
        self.n = len(keep)

    def gather_records_device(self, entries, d_min_ptr, d_pos_ptr, cap):
        """ioc_gather_records_device: the minimizer lists of `entries` of the current queries, gathered on the device
        into the caller's device buffers (addresses as ints, capacity in words).  Returns (words, off_fwd, off_rev)."""
        entries = np.ascontiguousarray(entries, np.int32)
        n = len(entries)
        of, orv = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        w = self.L.ioc_gather_records_device(self.h, n, _p(entries, C.c_int32), C.c_void_p(int(d_min_ptr)), C.c_void_p(int(d_pos_ptr)),
                                             int(cap), _p(of, C.c_int64), _p(orv, C.c_int64))
        self._chk(w)
        return int(w), of, orv

    def timings(self):
        t = Timings()
        self._chk(self.L.ioc_get_timings(self.h, C.byref(t)))
        return t.as_dict()

    def count_reference_postings(self):
        h = C.c_int64(0)
        self._chk(self.L.ioc_count_reference_postings(self.h, C.byref(h)))
        return h.value

    def synchronize(self):
        self._chk(self.L.ioc_synchronize(self.h))

    # ---- ClusterSortedReads on one sorted batch (src/cluster.cpp:67-322) -------------------------
    def cluster_batch(self, params: Params, batch: dict, table=_lib.TABLE_PATH):
        """batch: dict with off_fwd, off_rev, min_val, min_pos, raw_len, hpc_len, score, raw_err,
        hpc_err, state, min_qual (the fields of ioc_batch_view).  Returns (cls, strand, stats)."""
        return self.cluster_merge(params, None, batch, table)

    def _make_view(self, batch: dict):
        """ioc_batch_view over the arrays of `batch` (see _merge_call); returns (view, n, objects that must outlive the call)."""
        on_dev = bool(batch.get("minimizers_on_device"))   # min_val / min_pos: device addresses (ints), total = words
        arrs = {
            "off_fwd": np.ascontiguousarray(batch["off_fwd"], np.int64),
            "off_rev": np.ascontiguousarray(batch["off_rev"], np.int64),
            "min_val": None if on_dev else np.ascontiguousarray(batch["min_val"], np.uint32),
            "min_pos": None if on_dev else np.ascontiguousarray(batch["min_pos"], np.uint32),
            "raw_len": np.ascontiguousarray(batch["raw_len"], np.uint32),
            "hpc_len": np.ascontiguousarray(batch["hpc_len"], np.uint32),
            "score": np.ascontiguousarray(batch["score"], np.float64),
            "raw_err": np.ascontiguousarray(batch["raw_err"], np.float64),
            "hpc_err": np.ascontiguousarray(batch["hpc_err"], np.float64),
            "state": np.ascontiguousarray(batch["state"], np.uint8),
        }
        n = len(arrs["off_fwd"]) - 1
        nm = None
        if batch.get("n_members") is not None:
            nm = np.ascontiguousarray(batch["n_members"], np.int32)
        rseq = roff = None
        if batch.get("raw_seq") is not None:   # sahlin / furious: sequences for the host aligner
            rseq = batch["raw_seq"] if isinstance(batch["raw_seq"], bytes) else np.asarray(batch["raw_seq"], np.uint8).tobytes()
            roff = np.ascontiguousarray(batch["raw_off"], np.int64)
        isc = None
        if batch.get("is_cluster") is not None:
            isc = np.ascontiguousarray(batch["is_cluster"], np.uint8)
        if on_dev:
            mvp = C.cast(C.c_void_p(int(batch["min_val"])), C.POINTER(C.c_uint32))
            mpp = C.cast(C.c_void_p(int(batch["min_pos"])), C.POINTER(C.c_uint32))
            total = int(batch["total"])
        else:
            mvp, mpp, total = _p(arrs["min_val"], C.c_uint32), _p(arrs["min_pos"], C.c_uint32), len(arrs["min_val"])
        v = BatchView(n=n, off_fwd=_p(arrs["off_fwd"], C.c_int64), off_rev=_p(arrs["off_rev"], C.c_int64),
                      min_val=mvp, min_pos=mpp,
                      total=total, raw_len=_p(arrs["raw_len"], C.c_uint32),
                      hpc_len=_p(arrs["hpc_len"], C.c_uint32), score=_p(arrs["score"], C.c_double),
                      raw_err=_p(arrs["raw_err"], C.c_double), hpc_err=_p(arrs["hpc_err"], C.c_double),
                      state=_p(arrs["state"], C.c_uint8), min_qual=float(batch.get("min_qual", 7.0)),
                      raw_seq=rseq, raw_off=_p(roff, C.c_int64) if roff is not None else None,
                      n_members=_p(nm, C.c_int32) if nm is not None else None,
                      depth=int(batch.get("depth", -1)), min_cls_size=int(batch.get("min_cls_size", 3)),
                      is_cluster=_p(isc, C.c_uint8) if isc is not None else None, minimizers_on_device=1 if on_dev else 0)
        return v, n, (arrs, nm, rseq, roff, isc)

    def _merge_call(self, params: Params, left, batch: dict, table, cons=None):
        """ClusterSortedReads(left, right).  left: None (initial clustering) or dict with cls_hpc_err,
        keys, offs, postings (the left clusters' representative error rates + MinDB as CSR).
        batch: the right batch (ioc_batch_view fields; for a clustered right batch one record per
        right cluster = its representative, plus n_members / depth / min_cls_size)."""
        v, n, _alive = self._make_view(batch)
        lv = None
        if left is not None and left.get("resident"):
            # the left state already on the device (left_load / left_adopt + index_update) is used as it is; the
            # representatives' sequences (sahlin / furious) are host data all the same
            le = np.ascontiguousarray(left["cls_hpc_err"], np.float64)
            lseq = loff = lerr = None
            if left.get("rep_seq") is not None:
                lseq = left["rep_seq"] if isinstance(left["rep_seq"], bytes) else np.asarray(left["rep_seq"], np.uint8).tobytes()
                loff = np.ascontiguousarray(left["rep_off"], np.int64)
                lerr = np.ascontiguousarray(left["cls_raw_err"], np.float64)
            lv = LeftView(n_clusters=len(le), cls_hpc_err=_p(le, C.c_double), n_keys=-1, keys=None, offs=None,
                          postings=None, rep_seq=lseq, rep_off=_p(loff, C.c_int64) if loff is not None else None,
                          cls_raw_err=_p(lerr, C.c_double) if lerr is not None else None)
        elif left is not None:
            le = np.ascontiguousarray(left["cls_hpc_err"], np.float64)
            lk = np.ascontiguousarray(left["keys"], np.uint32)
            lo = np.ascontiguousarray(left["offs"], np.int64)
            lp = np.ascontiguousarray(left["postings"], np.uint32)
            lseq = loff = lerr = None
            if left.get("rep_seq") is not None:
                lseq = left["rep_seq"] if isinstance(left["rep_seq"], bytes) else np.asarray(left["rep_seq"], np.uint8).tobytes()
                loff = np.ascontiguousarray(left["rep_off"], np.int64)
                lerr = np.ascontiguousarray(left["cls_raw_err"], np.float64)
            lv = LeftView(n_clusters=len(le), cls_hpc_err=_p(le, C.c_double), n_keys=len(lk),
                          keys=_p(lk, C.c_uint32), offs=_p(lo, C.c_int64), postings=_p(lp, C.c_uint32),
                          rep_seq=lseq, rep_off=_p(loff, C.c_int64) if loff is not None else None,
                          cls_raw_err=_p(lerr, C.c_double) if lerr is not None else None)
        cls, strand = np.zeros(n, np.int32), np.zeros(n, np.int8)
        st = ClusterStats()
        if cons is None:
            self._chk(self.L.ioc_cluster_merge(self.h, C.byref(params), table.encode(),
                                               C.byref(lv) if lv is not None else None, C.byref(v),
                                               _p(cls, C.c_int32), _p(strand, C.c_int8), C.byref(st)))
        else:
            cargs, ops = cons
            self._chk(self.L.ioc_cluster_consensus(self.h, C.byref(params), table.encode(),
                                                   C.byref(lv) if lv is not None else None, C.byref(v), C.byref(cargs),
                                                   C.byref(ops), _p(cls, C.c_int32), _p(strand, C.c_int8), C.byref(st)))
        self.n = n
        self.params = params
        self._keep = [batch.get("_keepalive")]   # device tensors borrowed by the context (minimizers_on_device)
        return cls, strand, st.as_dict()

    def cluster_merge(self, params: Params, left, batch: dict, table=_lib.TABLE_PATH):
        """ClusterSortedReads(left, right), consensus off (see _merge_call for the views)."""
        return self._merge_call(params, left, batch, table)

    def cluster_consensus(self, params: Params, left, batch: dict, cons_args, ops, table=_lib.TABLE_PATH):
        """ClusterSortedReads with the consensus branch (ioc_cluster_consensus): cons_args = _lib.ConsensusArgs,
        ops = _lib.ConsensusOps (the caller's graph store); batch needs raw_seq / raw_off."""
        return self._merge_call(params, left, batch, table, cons=(cons_args, ops))

    def cluster_resident(self):
        n = self.n
        cls, strand = np.zeros(n, np.int32), np.zeros(n, np.int8)
        st = ClusterStats()
        self._chk(self.L.ioc_cluster_resident(self.h, _p(cls, C.c_int32), _p(strand, C.c_int8), C.byref(st)))
        return cls, strand, st.as_dict()
