"""ctypes bindings of the CPU oracle (oracle/liboracle.so) and of oracle/_ref.

TEST INFRASTRUCTURE: importable only from tests/, bench.py's cpu_baseline leg and
__graft_entry__.smoke().  Nothing under isonclust2_amd/ imports this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PMIN_BIN = os.path.join(os.path.dirname(HERE), "isonclust2_amd", "data", "pmin_shared.bin")


class Params(C.Structure):
    _fields_ = [("k", C.c_int32), ("w", C.c_int32), ("min_shared", C.c_int32),
                ("min_cls_size", C.c_int32), ("mode", C.c_int32), ("cons_max_size", C.c_int32),
                ("min_qual", C.c_double), ("mapped_threshold", C.c_double),
                ("aligned_threshold", C.c_double), ("min_fraction", C.c_double),
                ("min_prob_no_hits", C.c_double)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("probes", "postings", "mapped_calls", "queries",
                                          "new_clusters", "joins", "index_appends", "aln_invoked",
                                          "tie_reads", "cons_invoked")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


MODE = {"sahlin": 0, "fast": 1, "furious": 2, "none": 3}


def default_params(k=11, w=15, mode="fast"):
    """Defaults of CmdArgs (src/args.h:9-37)."""
    return Params(k=k, w=w, min_shared=5, min_cls_size=3, mode=MODE[mode], cons_max_size=-150,
                  min_qual=7.0, mapped_threshold=0.65, aligned_threshold=0.2, min_fraction=0.8,
                  min_prob_no_hits=0.1)


def build(force=False):
    so = os.path.join(HERE, "liboracle.so")
    srcs = [os.path.join(HERE, "oracle.cpp"), os.path.join(HERE, "poa_oracle.cpp"), os.path.join(HERE, "sg_striped.cpp")]
    if force or not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(x) for x in srcs if os.path.exists(x)):
        subprocess.check_call(["make", "-s", "-C", HERE, "all"])
    return so


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    # ORACLE_LIB: a sanitizer build of the oracle (tools/run_sanitizers.sh)
    L = C.CDLL(os.environ.get("ORACLE_LIB") or build())
    vp, i32, i64p = C.c_void_p, C.c_int, C.POINTER(C.c_int64)
    u32p, i32p, dp, cp = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_char_p
    L.orc_hpc.argtypes = [cp, cp, i32, cp, cp]
    L.orc_revcomp.argtypes = [cp, i32, cp]
    L.orc_kmer_encode.argtypes = [cp, i32, i32, u32p]
    L.orc_minimizers.argtypes = [u32p, i32, i32, i32, u32p, u32p, u32p]
    L.orc_qual_tab.argtypes = [i32, dp]
    L.orc_qual_score.argtypes = [cp, i32, i32]
    L.orc_qual_score.restype = C.c_double
    L.orc_error_rate.argtypes = [cp, i32, i32]
    L.orc_error_rate.restype = C.c_double
    L.orc_round.argtypes = [C.c_double, i32]
    L.orc_round.restype = C.c_double
    L.orc_pmin_table.argtypes = [cp, i32, i32, dp]
    L.orc_pmin_lookup.argtypes = [dp, C.c_double, C.c_double, i32p]
    L.orc_pmin_lookup.restype = C.c_double
    L.orc_gap_limit.argtypes = [C.c_double, C.c_double]
    L.orc_kmer_to_index.argtypes = [cp, i32]
    L.orc_kmer_to_index.restype = C.c_uint32
    L.orc_index_to_kmer.argtypes = [C.c_uint32, i32, cp]
    L.orc_minmatch.argtypes = [cp, cp, i32, cp, cp, i32, i32, i32, cp, C.c_double, u32p, dp, dp]
    L.orc_reads_new.argtypes = [cp, cp, i64p, i32]
    L.orc_reads_new.restype = vp
    L.orc_reads_free.argtypes = [vp]
    L.orc_reads_score_sort.argtypes = [vp, i32, i32]
    L.orc_reads_n.argtypes = [vp]
    L.orc_reads_shift_orig.argtypes = [vp, i32]
    L.orc_reads_shift_orig.restype = None
    L.orc_reads_order.argtypes = [vp, i32p, dp, dp]
    L.orc_batch_prepare.argtypes = [vp, i32, i32, C.POINTER(Params), i32]
    L.orc_batch_prepare.restype = vp
    L.orc_batch_free.argtypes = [vp]
    L.orc_batch_n_entries.argtypes = [vp]
    L.orc_batch_entry_info.argtypes = [vp, i32p, i32p, i32p, i32p, dp, dp, dp, i32p, i32p]
    L.orc_batch_entry_mins.argtypes = [vp, i32, i32, u32p, u32p, u32p]
    L.orc_batch_entry_hpc.argtypes = [vp, i32, cp, cp]
    L.orc_cluster.argtypes = [vp, vp, C.POINTER(Params), cp, C.POINTER(Stats)]
    L.orc_batch_n_clusters.argtypes = [vp]
    L.orc_batch_n_members.argtypes = [vp]
    L.orc_batch_members.argtypes = [vp, i32p, i32p, i32p, i32p]
    L.orc_batch_index.argtypes = [vp, u32p, i64p, u32p, i64p]
    L.orc_batch_index.restype = C.c_int64
    L.orc_set_aligner.argtypes = [vp]
    L.orc_use_builtin_aligner.argtypes = [i32]
    L.orc_align.argtypes = [cp, i32, cp, i32, i32, i32, i32, i32, cp, i32, i32p]
    L.orc_gap_open.argtypes = [C.c_double]
    L.orc_aln_ratio.argtypes = [cp, i32, C.c_double, C.c_uint, C.c_uint]
    L.orc_aln_ratio.restype = C.c_double
    u8p = C.POINTER(C.c_uint8)
    L.orc_trace_set.argtypes = [i32p, i32, i32]
    L.orc_trace_set.restype = None
    L.orc_trace_rows.argtypes = [i32p, i32p, i32p, u32p, u32p, u32p, i32p, u8p]
    L.orc_trace_rows.restype = C.c_int64
    L.orc_trace_mapped_calls.argtypes = [i32p, i32p, i32p, u32p, u32p, dp, dp]
    L.orc_trace_mapped_calls.restype = C.c_int64
    L.orc_batch_update_mindb.argtypes = [vp, C.c_int, u32p, C.c_int64, u32p, C.c_int64, C.c_int]
    L.orc_set_consensus.argtypes = [vp, C.c_int, C.c_int]
    L.orc_set_consensus.restype = None
    # the scalar partial-order alignment (poa_oracle.cpp)
    L.orp_create.argtypes = [i32] * 6
    L.orp_create.restype = vp
    L.orp_create_mode.argtypes = [i32] * 7
    L.orp_create_mode.restype = vp
    L.orp_destroy.argtypes = [vp]
    L.orp_destroy.restype = None
    L.orp_bind.argtypes = [vp, vp]
    L.orp_bind.restype = None
    L.orp_graph_export.argtypes = [vp, i32, i32, i32p, i32p, i32p, cp, i32p, i32p, i32p, i64p, i32p, i32p]
    L.orp_last_alignment.argtypes = [vp, i32, i32p, i32p, i32p]
    L.orp_graph_copy.argtypes = [vp, i32, i32, vp, i32, i32]
    L.orc_sg_striped16.argtypes = [cp, i32, cp, i32, i32, i32, i32, i32, i32p]
    L.orc_sg_striped16.restype = C.c_int32
    _lib = L
    return L


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


# ---- thin numpy-level helpers -------------------------------------------------------------
def hpc(seq: bytes, qual: bytes):
    o1, o2 = C.create_string_buffer(len(seq) + 1), C.create_string_buffer(len(seq) + 1)
    n = lib().orc_hpc(seq, qual, len(seq), o1, o2)
    return o1.raw[:n], o2.raw[:n]


def revcomp(seq: bytes):
    o = C.create_string_buffer(len(seq) + 1)
    if lib().orc_revcomp(seq, len(seq), o) != 0:
        raise ValueError("invalid base")
    return o.raw[:len(seq)]


def kmer_encode(seq: bytes, k: int):
    out = np.zeros(max(len(seq), 1), np.uint32)
    n = lib().orc_kmer_encode(seq, len(seq), k, _p(out, C.c_uint32))
    return out[:n].copy()


def minimizers(kmers: np.ndarray, k: int, w: int):
    kmers = np.ascontiguousarray(kmers, np.uint32)
    n = len(kmers)
    a, b, c = (np.zeros(max(n, 1), np.uint32) for _ in range(3))
    m = lib().orc_minimizers(_p(kmers, C.c_uint32), n, k, w, _p(a, C.c_uint32), _p(b, C.c_uint32),
                             _p(c, C.c_uint32))
    return a[:m].copy(), b[:m].copy(), c[:m].copy()


def qual_score(qual: bytes, k: int):
    return lib().orc_qual_score(qual, len(qual), k)


def error_rate(qual: bytes, nomin=True):
    return lib().orc_error_rate(qual, len(qual), 1 if nomin else 0)


def pmin_table(k, w, path=PMIN_BIN):
    t = np.zeros(225, np.float64)
    n = lib().orc_pmin_table(path.encode(), k, w, _p(t, C.c_double))
    if n < 0:
        raise IOError(path)
    return t.reshape(15, 15), n


def pmin_lookup(tab, e1, e2):
    tab = np.ascontiguousarray(tab, np.float64).reshape(-1)
    err = C.c_int32(0)
    r = lib().orc_pmin_lookup(_p(tab, C.c_double), e1, e2, C.byref(err))
    if err.value:
        raise KeyError((e1, e2))
    return r


def align(read: bytes, rep: bytes, e: float, k: int, match=2, mismatch=-2, gap_extend=1):
    """The oracle's own semi-global aligner + getAlnRatio (src/cluster.cpp:408-459): (score, comp, ratio)."""
    cap = len(read) + len(rep) + 2
    comp = C.create_string_buffer(cap)
    sc = C.c_int32()
    n = lib().orc_align(read, len(read), rep, len(rep), match, mismatch, lib().orc_gap_open(e), gap_extend, comp, cap, C.byref(sc))
    if n < 0:
        raise RuntimeError("orc_align failed")
    return sc.value, comp.raw[:n], lib().orc_aln_ratio(comp, n, e, len(read), k)


def trace_set(entries=(), mapped_calls=False):
    """Candidate tables of these right-batch entries (+ optionally every getMappedRatio call) are recorded by the
    next Batch.cluster; trace_rows() / trace_mapped_calls() read them."""
    a = np.ascontiguousarray(list(entries), np.int32)
    lib().orc_trace_set(_p(a, C.c_int32) if len(a) else None, len(a), 1 if mapped_calls else 0)


def trace_rows():
    n = lib().orc_trace_rows(None, None, None, None, None, None, None, None)
    d = dict(entry=np.zeros(n, np.int32), cls=np.zeros(n, np.int32), strand=np.zeros(n, np.int32),
             size=np.zeros(n, np.uint32), first_index=np.zeros(n, np.uint32), total_mapped=np.zeros(n, np.uint32),
             order_pos=np.zeros(n, np.int32), walked=np.zeros(n, np.uint8))
    if n:
        lib().orc_trace_rows(_p(d["entry"], C.c_int32), _p(d["cls"], C.c_int32), _p(d["strand"], C.c_int32),
                             _p(d["size"], C.c_uint32), _p(d["first_index"], C.c_uint32), _p(d["total_mapped"], C.c_uint32),
                             _p(d["order_pos"], C.c_int32), _p(d["walked"], C.c_uint8))
    return d


def trace_mapped_calls():
    n = lib().orc_trace_mapped_calls(None, None, None, None, None, None, None)
    d = dict(entry=np.zeros(n, np.int32), cls=np.zeros(n, np.int32), strand=np.zeros(n, np.int32),
             total=np.zeros(n, np.uint32), hpc_len=np.zeros(n, np.uint32), ratio=np.zeros(n, np.float64),
             p_error=np.zeros(n, np.float64))
    if n:
        lib().orc_trace_mapped_calls(_p(d["entry"], C.c_int32), _p(d["cls"], C.c_int32), _p(d["strand"], C.c_int32),
                                     _p(d["total"], C.c_uint32), _p(d["hpc_len"], C.c_uint32), _p(d["ratio"], C.c_double),
                                     _p(d["p_error"], C.c_double))
    return d


class ReadSet:
    """FillQualScores + SortByQualScores over a list of (seq, qual) byte strings."""

    def __init__(self, seqs, quals):
        offs = np.zeros(len(seqs) + 1, np.int64)
        offs[1:] = np.cumsum([len(s) for s in seqs])
        self._s, self._q = b"".join(seqs), b"".join(quals)
        self._offs = offs
        self.h = lib().orc_reads_new(self._s, self._q, _p(offs, C.c_int64), len(seqs))

    @classmethod
    def from_flat(cls, seq_flat: np.ndarray, qual_flat: np.ndarray, offs: np.ndarray):
        self = cls.__new__(cls)
        self._s, self._q = seq_flat.tobytes(), qual_flat.tobytes()
        self._offs = np.ascontiguousarray(offs, np.int64)
        self.h = lib().orc_reads_new(self._s, self._q, _p(self._offs, C.c_int64), len(offs) - 1)
        return self

    def score_sort(self, k, w):
        lib().orc_reads_score_sort(self.h, k, w)

    def shift_orig(self, base):
        lib().orc_reads_shift_orig(self.h, int(base))

    def order(self):
        n = lib().orc_reads_n(self.h)
        o, s, e = np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(n, np.float64)
        lib().orc_reads_order(self.h, _p(o, C.c_int32), _p(s, C.c_double), _p(e, C.c_double))
        return o, s, e

    def __len__(self):
        return lib().orc_reads_n(self.h)

    def __del__(self):
        if getattr(self, "h", None):
            lib().orc_reads_free(self.h)
            self.h = None


class Batch:
    def __init__(self, reads: ReadSet, start, end, params: Params, batch_nr=0):
        self.params = params
        self.h = lib().orc_batch_prepare(reads.h, start, end, C.byref(params), batch_nr)
        if not self.h:
            raise ValueError("PrepareSortedBatch failed (non-ACGT base)")

    def n_entries(self):
        return lib().orc_batch_n_entries(self.h)

    def entry_info(self):
        n = self.n_entries()
        i32 = lambda: np.zeros(n, np.int32)
        f64 = lambda: np.zeros(n, np.float64)
        d = dict(state=i32(), orig=i32(), raw_len=i32(), hpc_len=i32(), score=f64(), raw_err=f64(),
                 hpc_err=f64(), n_fwd=i32(), n_rev=i32())
        lib().orc_batch_entry_info(self.h, _p(d["state"], C.c_int32), _p(d["orig"], C.c_int32),
                                   _p(d["raw_len"], C.c_int32), _p(d["hpc_len"], C.c_int32),
                                   _p(d["score"], C.c_double), _p(d["raw_err"], C.c_double),
                                   _p(d["hpc_err"], C.c_double), _p(d["n_fwd"], C.c_int32),
                                   _p(d["n_rev"], C.c_int32))
        return d

    def entry_mins(self, i, strand, n):
        a, b, c = (np.zeros(max(n, 1), np.uint32) for _ in range(3))
        m = lib().orc_batch_entry_mins(self.h, i, strand, _p(a, C.c_uint32), _p(b, C.c_uint32),
                                       _p(c, C.c_uint32))
        return a[:m], b[:m], c[:m]

    def entry_hpc(self, i, n):
        a, b = C.create_string_buffer(n + 1), C.create_string_buffer(n + 1)
        m = lib().orc_batch_entry_hpc(self.h, i, a, b)
        return a.raw[:m], b.raw[:m]

    def minimizer_soa(self):
        """Flat SoA of all entries' minimizers: (info, off_fwd, off_rev, min, pos); fwd lists first."""
        info = self.entry_info()
        n = self.n_entries()
        nf, nr = info["n_fwd"].astype(np.int64), info["n_rev"].astype(np.int64)
        off_f = np.zeros(n + 1, np.int64)
        off_f[1:] = np.cumsum(nf)
        off_r = np.zeros(n + 1, np.int64)
        off_r[1:] = np.cumsum(nr)
        off_r += off_f[-1]
        tot = int(off_r[-1])
        mn, ps = np.zeros(tot, np.uint32), np.zeros(tot, np.uint32)
        for i in range(n):
            for s, off, cnt in ((0, off_f, nf), (1, off_r, nr)):
                if cnt[i]:
                    a, b, c = self.entry_mins(i, s, int(cnt[i]))
                    assert np.array_equal(c, np.arange(len(c), dtype=np.uint32))
                    mn[off[i]:off[i] + cnt[i]] = a
                    ps[off[i]:off[i] + cnt[i]] = b
        return info, off_f, off_r, mn, ps

    def cluster(self, right=None, mode="fast", min_cls_size=-1, stats=True, path=PMIN_BIN):
        p = Params.from_buffer_copy(self.params)
        p.mode = MODE[mode]
        p.min_cls_size = min_cls_size
        st = Stats()
        rc = lib().orc_cluster(self.h, right.h if right is not None else None, C.byref(p),
                               path.encode(), C.byref(st) if stats else None)
        if rc != 0:
            raise RuntimeError(f"orc_cluster failed: {rc}")
        return st.as_dict()

    def members(self):
        n = lib().orc_batch_n_members(self.h)
        a, b, c, d = (np.zeros(max(n, 1), np.int32) for _ in range(4))
        m = lib().orc_batch_members(self.h, _p(a, C.c_int32), _p(b, C.c_int32), _p(c, C.c_int32),
                                    _p(d, C.c_int32))
        return a[:m], b[:m], c[:m], d[:m]

    def n_clusters(self):
        return lib().orc_batch_n_clusters(self.h)

    def assignments(self, n_reads):
        """(cls, strand) per original read index; -1/0 for reads in no cluster."""
        cls, orig, strand, is_rep = self.members()
        acl = np.full(n_reads, -1, np.int32)
        ast = np.zeros(n_reads, np.int32)
        keep = is_rep == 0
        acl[orig[keep]] = cls[keep]
        ast[orig[keep]] = strand[keep]
        return acl, ast

    def index(self):
        np_ = C.c_int64(0)
        nk = lib().orc_batch_index(self.h, None, None, None, C.byref(np_))
        keys = np.zeros(max(nk, 1), np.uint32)
        offs = np.zeros(nk + 1, np.int64)
        post = np.zeros(max(np_.value, 1), np.uint32)
        lib().orc_batch_index(self.h, _p(keys, C.c_uint32), _p(offs, C.c_int64), _p(post, C.c_uint32),
                              C.byref(np_))
        return keys[:nk], offs, post[:np_.value]

    def update_mindb(self, cls, old_min, new_min, mins_too=True):
        """UpdateMinDB (src/minimizer.cpp:124-160) for cluster `cls` of this (clustered) batch."""
        old_min = np.ascontiguousarray(old_min, np.uint32)
        new_min = np.ascontiguousarray(new_min, np.uint32)
        rc = lib().orc_batch_update_mindb(self.h, int(cls), _p(old_min, C.c_uint32), len(old_min),
                                          _p(new_min, C.c_uint32), len(new_min), 1 if mins_too else 0)
        if rc != 0:
            raise ValueError("orc_batch_update_mindb failed")

    def __del__(self):
        if getattr(self, "h", None):
            lib().orc_batch_free(self.h)
            self.h = None


# ---- oracle/_ref (reference TUs compiled where they lie; build container only) ------------------------
_ref = None


def ref():
    """Returns the ctypes handle of oracle/_ref/libisonref.so, or None if it was never built."""
    global _ref
    if _ref is not None:
        return _ref
    so = os.path.join(HERE, "_ref", "libisonref.so")
    if not os.path.exists(so):
        return None
    R = C.CDLL(so)
    R.ref_kmer_encode.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_uint32)]
    R.ref_kmer_to_index.argtypes = [C.c_char_p, C.c_int]
    R.ref_kmer_to_index.restype = C.c_uint32
    R.ref_index_to_kmer.argtypes = [C.c_uint32, C.c_int, C.c_char_p]
    R.ref_revcomp.argtypes = [C.c_char_p, C.c_int, C.c_char_p]
    R.ref_round.argtypes = [C.c_double, C.c_int]
    R.ref_round.restype = C.c_double
    R.ref_pmin_init.argtypes = [C.c_int, C.c_int]
    R.ref_pmin_init.restype = C.c_void_p
    R.ref_pmin_size.argtypes = [C.c_void_p]
    R.ref_pmin_free.argtypes = [C.c_void_p]
    R.ref_pmin_lookup.argtypes = [C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_int)]
    R.ref_pmin_lookup.restype = C.c_double
    _ref = R
    return R


# ---- the scalar POA behind the consensus' graph operations (poa_oracle.cpp) -----------------------------------------------
class PoaOps(C.Structure):
    """orc_cons_ops (oracle.h) = the first six members of ioc_consensus_ops."""
    _fields_ = [("user", C.c_void_p), ("create", C.c_void_p), ("size", C.c_void_p), ("add", C.c_void_p),
                ("consensus", C.c_void_p), ("purge", C.c_void_p)]


class OraclePoa:
    """One store of partial-order graphs {(side, idx)} with spoa 4.0's operations restated (poa_oracle.cpp): create / add /
    size / consensus / purge, plus inspection of a graph and of the last alignment.  mode: the alignment type, numbered like
    `cluster -A` (0 local, 1 global, 2 semi-global)."""
    SC = dict(m=4, n=-8, g=-8, e=-4, q=-20, c=-1)   # src/main.cpp:285-290

    def __init__(self, mode=0, **sc):
        sc = dict(self.SC, **sc)
        self.L = lib()
        self.mode = mode
        self.h = self.L.orp_create_mode(mode, sc["m"], sc["n"], sc["g"], sc["e"], sc["q"], sc["c"])
        assert self.h, f"unknown alignment type {mode}"
        self.ops = PoaOps()
        self.L.orp_bind(self.h, C.addressof(self.ops))
        proto = lambda *a: C.CFUNCTYPE(C.c_int, C.c_void_p, *a)
        self._create = proto(C.c_int, C.c_int, C.c_char_p, C.c_int)(self.ops.create)
        self._size = proto(C.c_int, C.c_int)(self.ops.size)
        self._add = proto(C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_uint)(self.ops.add)
        self._cons = proto(C.c_int, C.c_int, C.c_char_p, C.c_int)(self.ops.consensus)
        self._purge = proto(C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_uint)(self.ops.purge)

    def ops_pointer(self):
        """for orc_set_consensus / a struct that starts like ioc_consensus_ops"""
        return C.cast(C.pointer(self.ops), C.c_void_p)

    def create(self, idx, s, side=0):
        assert self._create(self.ops.user, side, idx, s, len(s)) == 0

    def add(self, idx, s, w=1, side=0):
        assert self._add(self.ops.user, side, idx, s, len(s), w) == 0

    def purge(self, idx, s, w=1, side=0):
        assert self._purge(self.ops.user, side, idx, s, len(s), w) == 0

    def size(self, idx, side=0):
        return self._size(self.ops.user, side, idx)

    def consensus(self, idx, side=0):
        buf = C.create_string_buffer(1 << 20)
        n = self._cons(self.ops.user, side, idx, buf, len(buf))
        assert n >= 0
        return buf.raw[:n]

    def graph(self, idx, side=0, aligned=False):
        nn, ne, na = C.c_int32(), C.c_int32(), C.c_int32()
        assert self.L.orp_graph_export(self.h, side, idx, C.byref(nn), C.byref(ne), C.byref(na), None, None, None, None, None, None, None) == 0
        bases = C.create_string_buffer(nn.value + 1)
        rank = np.zeros(max(1, nn.value), np.int32)
        ef, et = np.zeros(max(1, ne.value), np.int32), np.zeros(max(1, ne.value), np.int32)
        ew = np.zeros(max(1, ne.value), np.int64)
        ao, al = np.zeros(nn.value + 1, np.int32), np.zeros(max(1, na.value), np.int32)
        assert self.L.orp_graph_export(self.h, side, idx, C.byref(nn), C.byref(ne), C.byref(na), bases, _p(rank, C.c_int32), _p(ef, C.c_int32),
                                       _p(et, C.c_int32), _p(ew, C.c_int64), _p(ao, C.c_int32), _p(al, C.c_int32)) == 0
        out = (bases.raw[:nn.value], rank[:nn.value], ef[:ne.value], et[:ne.value], ew[:ne.value])
        if aligned:
            out += ([al[ao[v]:ao[v + 1]].tolist() for v in range(nn.value)],)
        return out

    def copy_graph_to(self, idx, other, to_side, to_idx, side=0):
        assert self.L.orp_graph_copy(self.h, side, idx, other.h, to_side, to_idx) == 0

    def last_alignment(self):
        sc = C.c_int32()
        n = self.L.orp_last_alignment(self.h, 0, None, None, C.byref(sc))
        nodes, pos = np.zeros(max(1, n), np.int32), np.zeros(max(1, n), np.int32)
        assert self.L.orp_last_alignment(self.h, n, _p(nodes, C.c_int32), _p(pos, C.c_int32), C.byref(sc)) == n
        return nodes[:n], pos[:n], sc.value

    def close(self):
        if self.h:
            self.L.orp_destroy(self.h)
            self.h = None
