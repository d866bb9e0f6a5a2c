"""ctypes loader of libisonclust2_hip.so (the C ABI of include/isonclust2_hip.h).

There is no CPU fallback: if the HIP library is missing, cannot be loaded, or no GPU is visible,
every compute entry point raises.  The library is built in-tree by `__graft_entry__.build()` /
`make -C isonclust2_amd/csrc`.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IOC_LIB", os.path.join(HERE, "libisonclust2_hip.so"))  # IOC_LIB: developer builds
TABLE_PATH = os.path.join(HERE, "data", "pmin_shared.bin")


class IocError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"isonclust2_hip error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    _fields_ = [("k", C.c_int32), ("w", C.c_int32), ("min_shared", C.c_int32), ("mode", C.c_int32),
                ("min_fraction", C.c_double), ("mapped_threshold", C.c_double),
                ("min_prob_no_hits", C.c_double), ("aligned_threshold", C.c_double)]


class BatchView(C.Structure):
    _fields_ = [("n", C.c_int32), ("off_fwd", C.POINTER(C.c_int64)), ("off_rev", C.POINTER(C.c_int64)),
                ("min_val", C.POINTER(C.c_uint32)), ("min_pos", C.POINTER(C.c_uint32)),
                ("total", C.c_int64), ("raw_len", C.POINTER(C.c_uint32)),
                ("hpc_len", C.POINTER(C.c_uint32)), ("score", C.POINTER(C.c_double)),
                ("raw_err", C.POINTER(C.c_double)), ("hpc_err", C.POINTER(C.c_double)),
                ("state", C.POINTER(C.c_uint8)), ("min_qual", C.c_double),
                ("raw_seq", C.c_char_p), ("raw_off", C.POINTER(C.c_int64)),
                ("n_members", C.POINTER(C.c_int32)), ("depth", C.c_int32), ("min_cls_size", C.c_int32),
                ("is_cluster", C.POINTER(C.c_uint8)), ("minimizers_on_device", C.c_int32)]


class LeftView(C.Structure):
    _fields_ = [("n_clusters", C.c_int32), ("cls_hpc_err", C.POINTER(C.c_double)), ("n_keys", C.c_int64),
                ("keys", C.POINTER(C.c_uint32)), ("offs", C.POINTER(C.c_int64)),
                ("postings", C.POINTER(C.c_uint32)), ("rep_seq", C.c_char_p),
                ("rep_off", C.POINTER(C.c_int64)), ("cls_raw_err", C.POINTER(C.c_double))]


class ClusterStats(C.Structure):
    _fields_ = [("n_clusters", C.c_int64), ("n_joined", C.c_int64), ("n_gated", C.c_int64),
                ("n_tie_replays", C.c_int64), ("n_aln_invoked", C.c_int64),
                ("resolve_iters", C.c_int32), ("aln_rounds", C.c_int32), ("n_aln_pairs", C.c_int64),
                ("n_aln_order_dep", C.c_int64), ("n_cons_invoked", C.c_int64), ("n_cons_restarts", C.c_int64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class RepRecord(C.Structure):  # ioc_rep_record
    _fields_ = [("raw_seq", C.POINTER(C.c_char)), ("raw_len", C.c_int32), ("raw_qual", C.c_char), ("raw_err", C.c_double),
                ("raw_score", C.c_double), ("hpc_seq", C.POINTER(C.c_char)), ("hpc_len", C.c_int32), ("hpc_err", C.c_double),
                ("fwd_min", C.POINTER(C.c_uint32)), ("fwd_pos", C.POINTER(C.c_uint32)), ("n_fwd", C.c_int32),
                ("rev_min", C.POINTER(C.c_uint32)), ("rev_pos", C.POINTER(C.c_uint32)), ("n_rev", C.c_int32),
                ("entry", C.c_int32)]


CONS_CREATE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_char), C.c_int)
CONS_SIZE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int)
CONS_ADD = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_char), C.c_int, C.c_uint)
CONS_CONSENSUS = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_char), C.c_int)
CONS_PURGE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_char), C.c_int, C.c_uint)
CONS_REP_CHANGED = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.POINTER(RepRecord))


class ConsensusOps(C.Structure):  # ioc_consensus_ops (the oracle's orc_cons_ops is its first six members)
    _fields_ = [("user", C.c_void_p), ("create", CONS_CREATE), ("size", CONS_SIZE), ("add", CONS_ADD),
                ("consensus", CONS_CONSENSUS), ("purge", CONS_PURGE), ("rep_changed", CONS_REP_CHANGED),
                ("spec", C.c_void_p)]   # ioc_consensus_spec_ops* (NULL: no deferred consensus; ioc_poa_bind sets it)


class ConsensusArgs(C.Structure):  # ioc_consensus_args
    _fields_ = [("cons_min_size", C.c_int32), ("cons_max_size", C.c_int32), ("cons_period", C.c_int32),
                ("left_depth", C.c_int32), ("left_sizes", C.POINTER(C.c_int32))]


class AlnPair(C.Structure):  # ioc_aln_pair
    _fields_ = [("query", C.c_int32), ("ref", C.c_int32), ("ref_revcomp", C.c_int32), ("reserved", C.c_int32),
                ("e", C.c_double)]


class AlnStats(C.Structure):  # ioc_aln_stats (64 bytes)
    _fields_ = [(n, C.c_int32) for n in ("length", "columns", "matches", "mismatches", "ins", "del", "ins_runs", "del_runs", "longest_ins",
                                         "longest_del", "lead_i", "lead_d", "trail_i", "trail_d")] + [("reserved", C.c_int32 * 2)]


class PileupCol(C.Structure):  # ioc_pileup_col (32 bytes)
    _fields_ = [(n, C.c_uint32) for n in ("a", "c", "g", "t", "other", "del", "ins_runs", "ins_bases")]


PILE_INS_SLOTS = 6  # IOC_PILE_INS_SLOTS


class PileupIns(C.Structure):  # ioc_pileup_ins (128 bytes)
    _fields_ = [("slot", (C.c_uint32 * 5) * PILE_INS_SLOTS), ("longer", C.c_uint32), ("reserved", C.c_uint32)]


class PolishStats(C.Structure):  # ioc_polish_stats (32 bytes)
    _fields_ = [(n, C.c_int32) for n in ("out_len", "n_sub", "n_del", "n_ins", "n_low")] + [("reserved", C.c_int32 * 3)]


class CorrectStats(C.Structure):  # ioc_correct_stats (32 bytes)
    _fields_ = [(n, C.c_int32) for n in ("out_len", "n_sub", "n_fill", "n_remove", "n_ins_add", "n_ins_drop", "n_low", "n_guarded")]


class IsoCorrectStats(C.Structure):  # ioc_iso_correct_stats (48 bytes)
    _fields_ = CorrectStats._fields_ + [(n, C.c_int32) for n in ("table", "n_long_runs", "n_long_bases", "flags")]


ISOC_UNRESOLVED = 1  # IOC_ISOC_UNRESOLVED


class PileSite(C.Structure):  # ioc_pile_site (32 bytes)
    _fields_ = [(n, C.c_int32) for n in ("row", "kind", "major", "minor")] + [(n, C.c_uint32) for n in ("depth", "n_major", "n_minor", "reserved")]


ALLELE_DEL, ALLELE_NONE = 5, 7  # IOC_ALLELE_DEL, IOC_ALLELE_NONE
SITE_BASE, SITE_INS = 0, 1      # IOC_SITE_BASE, IOC_SITE_INS
SPLIT_NONE = 255                # IOC_SPLIT_NONE
BLOCK_KEEP, BLOCK_SKIP, BLOCK_PART, BLOCK_NONE = 0, 1, 2, 3    # IOC_BLOCK_*
ISO_DIRECT, ISO_ASSIGNED, ISO_RARE, ISO_AMBIGUOUS = 0, 1, 2, 3  # IOC_ISO_*
BLOCKS_MAX = 32                 # IOC_BLOCKS_MAX
INS_LACK, INS_CARRY, INS_NONE = 0, 1, 3  # IOC_INS_*
INSERTS_MAX, INS_SLACK_MAX = 32, 32      # IOC_INSERTS_MAX, IOC_INS_SLACK_MAX
WIN_MAX = 512                            # IOC_WIN_MAX
INS_CARRY_B = 2                          # IOC_INS_CARRY_B
WINVAR_NONE, WINVAR_A, WINVAR_B, WINVAR_OTHER = 0, 1, 2, 3  # IOC_WINVAR_*
WINVAR_MIN_AGREE = 45                    # IOC_WINVAR_MIN_AGREE
WIN_NONE, WIN_VOTER, WIN_SHORT, WIN_LONG = 0, 1, 2, 3  # IOC_WIN_*
SPLICE_LACK, SPLICE_DONE, SPLICE_UNCALLED, SPLICE_OVERLAP = 0, 1, 2, 3  # IOC_SPLICE_*


class BlockRow(C.Structure):  # ioc_block_row (8 bytes)
    _fields_ = [("depth", C.c_uint32), ("in_gap", C.c_uint32)]


class PileBlock(C.Structure):  # ioc_pile_block (32 bytes)
    _fields_ = [("first", C.c_int32), ("end", C.c_int32)] + [(n, C.c_uint32) for n in ("n_keep", "n_skip", "n_part", "n_none")] + [("reserved", C.c_uint32 * 2)]


class ReadBlocks(C.Structure):  # ioc_read_blocks (32 bytes)
    _fields_ = [("key", C.c_uint64)] + [(n, C.c_int32) for n in ("group", "how", "first_row", "end_row", "n_gaps", "gap_rows")]


class BlocksSeg(C.Structure):  # ioc_blocks_seg (32 bytes)
    _fields_ = [(n, C.c_int32) for n in ("n_blocks", "n_found", "n_groups", "n_reads", "n_direct", "n_assigned", "n_rare", "n_ambiguous")]


class InsertRow(C.Structure):  # ioc_insert_row (8 bytes)
    _fields_ = [("span", C.c_uint32), ("in_ins", C.c_uint32)]


class PileInsert(C.Structure):  # ioc_pile_insert (32 bytes)
    _fields_ = [("first", C.c_int32), ("end", C.c_int32)] + [(n, C.c_uint32) for n in ("n_carry", "n_lack", "n_none", "len_min", "len_max", "reserved")]


class ReadInserts(C.Structure):  # ioc_read_inserts (32 bytes)
    _fields_ = [("key", C.c_uint64)] + [(n, C.c_int32) for n in ("group", "how", "n_near", "ins_bases")] + [("reserved", C.c_uint32 * 2)]


class InsertsSeg(C.Structure):  # ioc_inserts_seg (32 bytes)
    _fields_ = [(n, C.c_int32) for n in ("n_sites", "n_found", "n_groups", "n_reads", "n_direct", "n_assigned", "n_rare", "n_ambiguous")]


class InsertWindow(C.Structure):  # ioc_insert_window (32 bytes)
    _fields_ = [(n, C.c_int32) for n in ("lo", "hi", "template_pair", "tlen")] + [(n, C.c_uint32) for n in ("n_voters", "n_short", "n_long", "reserved")]


class SpliceSite(C.Structure):  # ioc_splice_site (16 bytes)
    _fields_ = [(n, C.c_int32) for n in ("state", "at", "len", "reserved")]


class SpliceStats(C.Structure):  # ioc_splice_stats (32 bytes)
    _fields_ = [(n, C.c_int32) for n in ("n_done", "n_uncalled", "n_overlap", "rows_replaced", "spliced_bytes")] + [("reserved", C.c_int32 * 3)]


ENDS_MAX, ENDS_SLACK_MAX = 32, 32  # IOC_ENDS_MAX, IOC_ENDS_SLACK_MAX
END_START, END_STOP = 0, 1         # IOC_END_*


class ReadExtent(C.Structure):  # ioc_read_extent (16 bytes)
    _fields_ = [(n, C.c_int32) for n in ("first_row", "end_row", "head", "tail")]


class EndSite(C.Structure):  # ioc_end_site (32 bytes)
    _fields_ = [("first", C.c_int32), ("end", C.c_int32), ("n_reads", C.c_uint32), ("n_over", C.c_uint32), ("peak_row", C.c_int32), ("peak_reads", C.c_uint32),
                ("kind", C.c_int32), ("reserved", C.c_uint32)]


class EndVariant(C.Structure):  # ioc_end_variant (16 bytes)
    _fields_ = [(n, C.c_int32) for n in ("pre_group", "start_site", "stop_site")] + [("n_reads", C.c_uint32)]


class ReadEnds(C.Structure):  # ioc_read_ends (16 bytes)
    _fields_ = [(n, C.c_int32) for n in ("start_site", "stop_site", "variant", "reserved")]


class EndsSeg(C.Structure):  # ioc_ends_seg (32 bytes)
    _fields_ = [(n, C.c_int32) for n in ("n_reads", "n_starts", "n_starts_found", "n_stops", "n_stops_found", "n_variants", "n_variants_found", "n_placed")]


class EndRow(C.Structure):  # ioc_end_row (16 bytes)
    _fields_ = [(n, C.c_uint32) for n in ("starts", "stops", "w_starts", "w_stops")]


class SplitSeg(C.Structure):  # ioc_split_seg (32 bytes)
    _fields_ = [(n, C.c_int32) for n in ("seed", "n_linked", "n_reads", "n_group0", "n_group1", "n_none")] + [("seed_link", C.c_int64)]


class PolishSeg(C.Structure):  # ioc_polish_seg
    _fields_ = [("ref", C.c_int32), ("ref_revcomp", C.c_int32)]


class DistMergeTimes(C.Structure):  # ioc_dist_merge_times
    _fields_ = [("ms_exchange_lists", C.c_float), ("ms_merge", C.c_double), ("bytes_lists", C.c_int64), ("bytes_records", C.c_int64),
                ("sharded", C.c_int32), ("exchanges", C.c_int32)]


# ioc_exchange_fn (ioc_set_shard): user, device buffer, element count, kind, hip stream
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p)
XCHG_MAX_U8, XCHG_MIN_U32, XCHG_SUM_I32 = 0, 1, 2


class Timings(C.Structure):
    _fields_ = [("ms_build", C.c_float), ("ms_score", C.c_float), ("ms_resolve", C.c_float),
                ("resolve_iters", C.c_int32), ("n_queries", C.c_int32), ("n_minimizers", C.c_int64),
                ("n_index_postings", C.c_int64), ("n_candidates", C.c_int64),
                ("n_mapped_evals", C.c_int64), ("postings_traversed", C.c_int64),
                ("ms_align_fwd", C.c_float), ("ms_align_trace", C.c_float), ("n_align_pairs", C.c_int64),
                ("n_align_cells", C.c_int64),
                ("n_align_refused", C.c_int64), ("score_oob", C.c_int32), ("score_oob_probe", C.c_int32),
                ("align_arena_bytes", C.c_int64), ("align_slices", C.c_int32), ("align_version", C.c_int32),
                ("n_align_cells_computed", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# every symbol include/isonclust2_hip.h declares (tests check the library exports all of them)
SYMBOLS = [
    "ioc_ctx_create", "ioc_ctx_destroy", "ioc_ctx_trim", "ioc_ctx_prewarm", "ioc_last_error", "ioc_set_stream", "ioc_synchronize",
    "ioc_set_params", "ioc_queries_upload", "ioc_queries_bind_device", "ioc_left_load",
    "ioc_index_build", "ioc_score", "ioc_resolve", "ioc_get_decisions", "ioc_get_cuts", "ioc_force_decision",
    "ioc_clear_forced", "ioc_query_candidates", "ioc_index_export", "ioc_qual_scores",
    "ioc_extract_minimizers", "ioc_extracted_download", "ioc_extracted_hpc_download", "ioc_queries_from_extracted",
    "ioc_get_timings", "ioc_count_reference_postings", "ioc_host_gap_limits", "ioc_host_err_cell", "ioc_host_min_total",
    "ioc_cluster_batch", "ioc_cluster_merge", "ioc_cluster_resident", "ioc_host_align", "ioc_host_gap_open", "ioc_host_align_route",
    "ioc_host_aln_ratio", "ioc_host_align_ops", "ioc_host_align_corridor","ioc_host_ops_to_cigar", "ioc_host_ops_stats", "ioc_host_ops_pileup", "ioc_host_ops_pileup_ins", "ioc_host_pileup_call", "ioc_host_qual_weight", "ioc_host_ops_pileup_weighted", "ioc_host_pileup_call_weighted", "ioc_host_ops_project", "ioc_host_pileup_sites", "ioc_host_site_alleles", "ioc_host_alleles_split", "ioc_host_ops_project_ins", "ioc_host_planes_pile", "ioc_align_set_pool", "ioc_align_pairs", "ioc_align_ops_bound",
    "ioc_align_pairs_ops", "ioc_align_pairs_stats", "ioc_align_pairs_pileup", "ioc_pileup_call", "ioc_align_pairs_polish", "ioc_align_set_pool_qual", "ioc_pileup_call_weighted", "ioc_align_pairs_polish_weighted", "ioc_pileup_sites", "ioc_align_pairs_alleles", "ioc_alleles_split", "ioc_align_pairs_split", "ioc_planes_polish", "ioc_align_pairs_split_polish", "ioc_set_aln_verdicts", "ioc_get_ties", "ioc_resident_set_sequences",
    "ioc_index_update", "ioc_left_export", "ioc_left_adopt", "ioc_cluster_consensus",
    "ioc_poa_create", "ioc_poa_create_mode", "ioc_poa_destroy", "ioc_poa_bind", "ioc_poa_graph_export", "ioc_poa_last_alignment",
    "ioc_poa_graph_save", "ioc_poa_graph_load", "ioc_poa_graph_load_many", "ioc_gather_records_device", "ioc_queries_generation", "ioc_scored_candidates",
    "ioc_dist_unique_id", "ioc_dist_init", "ioc_dist_shutdown", "ioc_dist_info", "ioc_dist_allgather_device",
    "ioc_dist_allgatherv_device", "ioc_dist_allgather_i64", "ioc_dist_allgatherv_host", "ioc_dist_allreduce_max",
    "ioc_dist_barrier", "ioc_dist_merge", "ioc_set_shard", "ioc_shard_exchanges", "ioc_shard_aligned_pairs", "ioc_dist_exchange", "ioc_dist_set_shard", "ioc_align_set_verdict_threshold",
    "ioc_host_read_correct", "ioc_planes_correct", "ioc_align_pairs_correct",
    "ioc_host_planes_blocks", "ioc_planes_blocks", "ioc_align_pairs_blocks",
    "ioc_planes_polish_groups", "ioc_align_pairs_blocks_polish",
    "ioc_host_ops_project_weights", "ioc_host_planes_pile_weighted", "ioc_planes_polish_groups_weighted", "ioc_align_pairs_blocks_polish_weighted",
    "ioc_host_ops_project_ilen", "ioc_host_planes_inserts", "ioc_planes_inserts", "ioc_align_pairs_blocks_inserts",
    "ioc_host_ops_project_qpos", "ioc_host_align_global_ops", "ioc_host_insert_windows", "ioc_planes_insert_windows", "ioc_align_pairs_blocks_inserts_seq",
    "ioc_host_ops_agreement", "ioc_host_key_isoforms", "ioc_host_insert_window_variants", "ioc_planes_insert_window_variants", "ioc_align_pairs_blocks_inserts_variants",
    "ioc_host_isoform_splice", "ioc_planes_isoforms_full", "ioc_align_pairs_isoforms_full",
    "ioc_host_isoform_splice_variants", "ioc_planes_isoforms_full_variants", "ioc_align_pairs_isoforms_full_variants",
    "ioc_host_ops_extent", "ioc_host_reads_ends", "ioc_reads_ends", "ioc_align_pairs_blocks_ends",
    "ioc_host_read_correct_long", "ioc_planes_correct_groups", "ioc_align_pairs_blocks_correct",
]

_lib = None


def load():
    """Load the HIP library or raise (never falls back)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IocError(-100, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    # torch wheels bundle their own libamdhip64; two HIP runtimes in one process cannot both own the
    # GPU.  Importing torch first makes the dynamic loader resolve our DT_NEEDED libamdhip64 to the copy
    # torch already mapped, so both sides share one runtime whatever the initialisation order.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    pi64, pu32, pu8 = C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    pi32, pi8, pd = C.POINTER(C.c_int32), C.POINTER(C.c_int8), C.POINTER(C.c_double)
    L.ioc_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.ioc_ctx_destroy.argtypes = [vp]
    L.ioc_ctx_destroy.restype = None
    L.ioc_last_error.argtypes = [vp]
    L.ioc_last_error.restype = C.c_char_p
    L.ioc_set_stream.argtypes = [vp, vp]
    L.ioc_synchronize.argtypes = [vp]
    L.ioc_set_params.argtypes = [vp, C.POINTER(Params), pi32]
    L.ioc_queries_upload.argtypes = [vp, i32, pi64, pi64, pu32, pu32, i64, pu32, pu8, pu32]
    L.ioc_queries_bind_device.argtypes = [vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, pi64, pi64]
    L.ioc_gather_records_device.argtypes = [vp, i32, pi32, vp, vp, i64, pi64, pi64]
    L.ioc_gather_records_device.restype = i64
    L.ioc_scored_candidates.argtypes = [vp, i32, i32, pu32, pu32]
    L.ioc_queries_generation.argtypes = [vp]
    L.ioc_queries_generation.restype = i64
    L.ioc_left_load.argtypes = [vp, i32, pu8, i64, pu32, pi64, pu32]
    L.ioc_index_update.argtypes = [vp, i32, pu32, i64, pu32, i64, C.c_uint8]
    L.ioc_left_export.argtypes = [vp, pi64, pi64, pu32, pi64, pu32]
    L.ioc_left_adopt.argtypes = [vp, pi32]
    L.ioc_index_build.argtypes = [vp]
    L.ioc_score.argtypes = [vp]
    L.ioc_resolve.argtypes = [vp, pi32]
    L.ioc_get_decisions.argtypes = [vp, pi32, pi8, pu8]
    L.ioc_get_cuts.argtypes = [vp, pi32]
    L.ioc_force_decision.argtypes = [vp, i32, i32, i32]
    L.ioc_clear_forced.argtypes = [vp]
    L.ioc_query_candidates.argtypes = [vp, i32, i32, pi32, pi8, pu32, pu32, pu32]
    L.ioc_index_export.argtypes = [vp, pi64, pi64, pu32, pi64, pu32]
    L.ioc_qual_scores.argtypes = [vp, i32, pi64, pu8, i32, pd, pd]
    L.ioc_extract_minimizers.argtypes = [vp, i32, pi64, pu8, pu8, i32, i32, pu32, pd, pi64, pi64, pi32]
    L.ioc_extracted_download.argtypes = [vp, pu32, pu32, i64]
    L.ioc_extracted_hpc_download.argtypes = [vp, C.c_char_p, C.c_char_p, i64]
    L.ioc_queries_from_extracted.argtypes = [vp, pu8, pu8, pu32]
    L.ioc_get_timings.argtypes = [vp, C.POINTER(Timings)]
    L.ioc_count_reference_postings.argtypes = [vp, pi64]
    L.ioc_host_gap_limits.argtypes = [C.c_char_p, i32, i32, C.c_double, pi32, pd]
    L.ioc_host_err_cell.argtypes = [C.c_double]
    L.ioc_host_err_cell.restype = C.c_uint8
    L.ioc_host_min_total.argtypes = [C.c_uint32, C.c_double]
    L.ioc_host_min_total.restype = C.c_uint32
    L.ioc_cluster_batch.argtypes = [vp, C.POINTER(Params), C.c_char_p, C.POINTER(BatchView), pi32, pi8,
                                    C.POINTER(ClusterStats)]
    L.ioc_cluster_merge.argtypes = [vp, C.POINTER(Params), C.c_char_p, C.POINTER(LeftView), C.POINTER(BatchView),
                                    pi32, pi8, C.POINTER(ClusterStats)]
    L.ioc_cluster_consensus.argtypes = [vp, C.POINTER(Params), C.c_char_p, C.POINTER(LeftView), C.POINTER(BatchView),
                                        C.POINTER(ConsensusArgs), C.POINTER(ConsensusOps), pi32, pi8, C.POINTER(ClusterStats)]
    L.ioc_poa_create.argtypes = [vp, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
    L.ioc_poa_create_mode.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
    L.ioc_poa_destroy.argtypes = [vp]
    L.ioc_poa_destroy.restype = None
    L.ioc_poa_bind.argtypes = [vp, C.POINTER(ConsensusOps)]
    L.ioc_poa_bind.restype = None
    L.ioc_poa_graph_export.argtypes = [vp, C.c_int, C.c_int, pi32, pi32, C.c_char_p, pi32, pi32, pi32, pi64]
    L.ioc_poa_last_alignment.argtypes = [vp, i32, pi32, pi32, pi32]
    L.ioc_poa_graph_save.argtypes = [vp, C.c_int, C.c_int, pu8, i64]
    L.ioc_poa_graph_save.restype = C.c_int64
    L.ioc_poa_graph_load.argtypes = [vp, C.c_int, C.c_int, pu8, i64]
    L.ioc_poa_graph_load_many.argtypes = [vp, C.c_int, C.c_int32, C.POINTER(C.c_int32), C.POINTER(pu8), C.POINTER(i64)]
    L.ioc_host_align.argtypes = [C.c_char_p, i32, C.c_char_p, i32, i32, i32, i32, i32, C.c_char_p, i32, pi32]
    L.ioc_host_align_ops.argtypes = [C.c_char_p, i32, C.c_char_p, i32, i32, i32, i32, i32, C.c_char_p, i32, pi32]
    L.ioc_host_align_corridor.argtypes = [C.c_char_p, i32, C.c_char_p, i32, i32, i32, i32, i32, pi32, i32, i32, pi32, pi32, C.c_char_p, i32, pi32]
    L.ioc_host_ops_to_cigar.argtypes = [C.c_char_p, i64, C.c_char_p, i64]
    L.ioc_host_ops_to_cigar.restype = C.c_int64
    L.ioc_host_ops_stats.argtypes = [C.c_char_p, i64, C.POINTER(AlnStats)]
    L.ioc_host_ops_pileup.argtypes = [C.c_char_p, i64, C.c_char_p, i32, i32, C.c_void_p]
    L.ioc_host_ops_pileup_ins.argtypes = [C.c_char_p, i64, C.c_char_p, i32, i32, C.c_void_p]
    L.ioc_host_pileup_call.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, i32, i32, C.c_void_p, C.c_void_p, i64, C.POINTER(PolishStats)]
    L.ioc_host_pileup_call.restype = C.c_int64
    L.ioc_host_qual_weight.argtypes = [C.c_uint8]
    L.ioc_host_qual_weight.restype = C.c_uint32
    L.ioc_host_ops_pileup_weighted.argtypes = [C.c_char_p, i64, C.c_char_p, C.c_char_p, i32, i32, C.c_void_p, C.c_void_p]
    L.ioc_host_pileup_call_weighted.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, i32, i32, C.c_void_p, C.c_void_p, i64,
                                                C.POINTER(PolishStats)]
    L.ioc_host_pileup_call_weighted.restype = C.c_int64
    L.ioc_host_ops_project.argtypes = [C.c_char_p, i64, C.c_char_p, i32, i32, C.c_void_p, C.c_void_p]
    L.ioc_host_pileup_sites.argtypes = [C.c_void_p, i32, i32, i32, i32, i32, C.c_void_p, pi64]
    L.ioc_host_pileup_sites.restype = C.c_int64
    L.ioc_host_site_alleles.argtypes = [C.c_void_p, C.c_void_p, i32, C.c_void_p, i32, C.c_void_p]
    L.ioc_host_alleles_split.argtypes = [C.c_void_p, i32, C.c_void_p, i32, i32, i32, i32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ioc_host_ops_project_ins.argtypes = [C.c_char_p, i64, C.c_char_p, i32, i32, C.c_void_p]
    L.ioc_host_planes_pile.argtypes = [C.c_void_p, C.c_void_p, i32, C.c_void_p, C.c_void_p]
    L.ioc_host_gap_open.argtypes = [C.c_double]
    L.ioc_host_align_route.argtypes = [i32, i32, i32, i32]
    L.ioc_host_aln_ratio.argtypes = [C.c_char_p, i32, C.c_double, C.c_uint32, C.c_uint32]
    L.ioc_host_aln_ratio.restype = C.c_double
    L.ioc_cluster_resident.argtypes = [vp, pi32, pi8, C.POINTER(ClusterStats)]
    L.ioc_resident_set_sequences.argtypes = [vp, C.c_char_p, pi64, pd]
    L.ioc_set_aln_verdicts.argtypes = [vp, pi32, pi8]
    L.ioc_get_ties.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.ioc_align_set_pool.argtypes = [vp, i32, C.c_char_p, C.POINTER(C.c_int64)]
    L.ioc_align_pairs.argtypes = [vp, i32, C.POINTER(AlnPair), i32, i32, i32, i32, pi32, C.POINTER(C.c_int64),
                                  C.POINTER(C.c_double)]
    L.ioc_align_ops_bound.argtypes = [vp, i32, C.POINTER(AlnPair)]
    L.ioc_align_ops_bound.restype = C.c_int64
    L.ioc_align_pairs_ops.argtypes = [vp, i32, C.POINTER(AlnPair), i32, i32, i32, i32, pi32, C.POINTER(C.c_int64),
                                      C.POINTER(C.c_double), C.c_void_p, i64, C.POINTER(C.c_int64)]
    L.ioc_align_pairs_stats.argtypes = [vp, i32, C.POINTER(AlnPair), i32, i32, i32, i32, pi32, C.POINTER(C.c_int64),
                                        C.POINTER(C.c_double), C.c_void_p]
    L.ioc_align_pairs_pileup.argtypes = [vp, i32, C.POINTER(AlnPair), i32, i32, i32, i32, pi32, C.POINTER(C.c_int64),
                                         C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int64), i64, C.c_void_p]
    L.ioc_pileup_call.argtypes = [vp, i32, pi32, C.c_char_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, i32, C.c_void_p, C.c_void_p, i64,
                                  C.POINTER(C.c_int64), C.c_void_p]
    L.ioc_align_pairs_polish.argtypes = [vp, i32, C.POINTER(AlnPair), i32, i32, i32, i32, pi32, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                                         C.c_void_p, i32, C.POINTER(PolishSeg), pi32, i32, C.c_void_p, C.c_void_p, i64,
                                         C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p]
    L.ioc_align_set_pool_qual.argtypes = [vp, C.c_char_p, i64]
    L.ioc_pileup_call_weighted.argtypes = [vp, i32, pi32, C.c_char_p, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, i32, C.c_void_p,
                                           C.c_void_p, i64, C.POINTER(C.c_int64), C.c_void_p]
    L.ioc_align_pairs_polish_weighted.argtypes = [vp, i32, C.POINTER(AlnPair), i32, i32, i32, i32, pi32, C.POINTER(C.c_int64),
                                                  C.POINTER(C.c_double), C.c_void_p, i32, C.POINTER(PolishSeg), pi32, i32, C.c_void_p, C.c_void_p,
                                                  i64, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ioc_pileup_sites.argtypes = [vp, i32, pi32, C.c_void_p, i32, i32, i32, i32, C.c_void_p, i64, pi64, pi64]
    L.ioc_align_pairs_alleles.argtypes = [vp, i32, C.POINTER(AlnPair), i32, i32, i32, i32, pi32, pi64, pd, C.c_void_p, i32, C.POINTER(PolishSeg),
                                          pi32, i32, i32, i32, i32, C.c_void_p, i64, pi64, pi64, C.c_void_p, i64, pi64, C.c_void_p]
    L.ioc_alleles_split.argtypes = [vp, i32, i32, pi32, C.c_void_p, pi64, C.c_void_p, pi64, i32, i32, i32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]
    L.ioc_align_pairs_split.argtypes = L.ioc_align_pairs_alleles.argtypes + [i32, i32, i32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ioc_planes_polish.argtypes = [vp, i32, pi32, C.c_char_p, pi64, i32, pi32, C.c_void_p, C.c_void_p, C.c_void_p, i32, C.c_void_p, C.c_void_p, i64, pi64,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
    L.ioc_align_pairs_split_polish.argtypes = L.ioc_align_pairs_split.argtypes + [i32, C.c_void_p, C.c_void_p, i64, pi64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ioc_host_read_correct.argtypes = [C.c_void_p, C.c_void_p, i32, C.c_void_p, C.c_void_p, C.c_char_p, i32, i32, i32, i32, C.c_void_p, C.c_void_p, i64,
                                        C.POINTER(CorrectStats)]
    L.ioc_host_read_correct.restype = C.c_int64
    L.ioc_planes_correct.argtypes = [vp, i32, pi32, C.c_char_p, pi64, C.c_void_p, C.c_void_p, i32, pi32, C.c_void_p, C.c_void_p, i32, i32, i32, i32,
                                     C.c_void_p, C.c_void_p, i64, pi64, C.c_void_p]
    L.ioc_align_pairs_correct.argtypes = [vp, i32, C.POINTER(AlnPair), i32, i32, i32, i32, pi32, pi64, pd, C.c_void_p, i32, C.POINTER(PolishSeg), pi32,
                                          i32, i32, i32, i32, C.c_void_p, C.c_void_p, i64, pi64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ioc_host_planes_blocks.argtypes = [C.c_void_p, i32, i32, i32, i32, i32, i32, i32, i32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ioc_planes_blocks.argtypes = [vp, i32, pi32, i32, pi32, C.c_void_p, i32, i32, i32, i32, i32, i32, C.c_void_p, C.c_void_p, i64, pi64, C.c_void_p, C.c_void_p]
    L.ioc_align_pairs_blocks.argtypes = [vp, i32, C.POINTER(AlnPair), i32, i32, i32, i32, pi32, pi64, pd, C.c_void_p, i32, C.POINTER(PolishSeg), pi32,
                                         i32, i32, i32, i32, i32, i32, C.c_void_p, C.c_void_p, i64, pi64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ioc_planes_polish_groups.argtypes = [vp, i32, pi32, C.c_char_p, pi64, pi32, i32, pi32, pi32, C.c_void_p, C.c_void_p, i32, C.c_void_p, C.c_void_p, i64,
                                           pi64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ioc_align_pairs_blocks_polish.argtypes = L.ioc_align_pairs_blocks.argtypes + [i32, i32, C.c_void_p, C.c_void_p, i64, pi64, C.c_void_p, i64, pi64]
    L.ioc_host_ops_project_weights.argtypes = [C.c_char_p, i64, C.c_char_p, C.c_char_p, i32, i32, C.c_void_p, C.c_void_p]
    L.ioc_host_planes_pile_weighted.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, i32, C.c_void_p, C.c_void_p]
    L.ioc_planes_polish_groups_weighted.argtypes = [vp, i32, pi32, C.c_char_p, pi64, pi32, i32, pi32, pi32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, i32, C.c_void_p,
                                                    C.c_void_p, i64, pi64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ioc_align_pairs_blocks_polish_weighted.argtypes = L.ioc_align_pairs_blocks_polish.argtypes
    L.ioc_host_ops_project_ilen.argtypes = [C.c_char_p, i64, i32, C.c_void_p]
    L.ioc_host_planes_inserts.argtypes = [C.c_void_p, C.c_void_p, i32, i32, i32, i32, i32, i32, i32, i32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]
    L.ioc_planes_inserts.argtypes = [vp, i32, pi32, i32, pi32, C.c_void_p, C.c_void_p, i32, i32, i32, i32, i32, i32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, i64, pi64, C.c_void_p, C.c_void_p]
    L.ioc_align_pairs_blocks_inserts.argtypes = L.ioc_align_pairs_blocks.argtypes + [i32, i32, i32, C.c_void_p, C.c_void_p, i64, pi64, C.c_void_p, C.c_void_p]
    L.ioc_host_ops_project_qpos.argtypes = [C.c_char_p, i64, i32, C.c_void_p]
    L.ioc_host_align_global_ops.argtypes = [C.c_char_p, i32, C.c_char_p, i32, i32, i32, i32, C.c_void_p, i64, pi32]
    L.ioc_host_align_global_ops.restype = C.c_int64
    L.ioc_host_insert_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, i32, i32, C.c_void_p, i32, C.c_void_p, i32, i32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
    L.ioc_planes_insert_windows.argtypes = [vp, i32, pi32, i32, pi32, pi32, C.c_void_p, C.c_void_p, C.c_void_p, pi64, C.c_void_p, i32, i32, i32, i32, i32, i32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, i64, pi64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ioc_align_pairs_blocks_inserts_seq.argtypes = L.ioc_align_pairs_blocks_inserts.argtypes + [i32, i32, i32, i32, i32, C.c_void_p, C.c_void_p, C.c_void_p, i64,
                                                                                                 pi64, C.c_void_p]
    L.ioc_host_ops_agreement.argtypes = [C.c_char_p, i64, pi32]
    L.ioc_host_key_isoforms.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, i32, i32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ioc_host_insert_window_variants.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, i32, i32, C.c_void_p, i32, C.c_void_p, C.c_char_p, C.c_void_p] + [i32] * 9 + [
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, i64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ioc_planes_insert_window_variants.argtypes = [vp, i32, pi32, i32, pi32, pi32, C.c_void_p, C.c_void_p, C.c_void_p, pi64, C.c_void_p] + [i32] * 9 + [
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, i64, pi64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ioc_align_pairs_blocks_inserts_variants.argtypes = L.ioc_align_pairs_blocks_inserts_seq.argtypes + [i32, C.c_void_p, C.c_void_p, C.c_void_p, i64, pi64, C.c_void_p,
                                                                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ioc_host_isoform_splice.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, i32, i32, C.c_uint64, C.c_void_p, i32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, i64, C.POINTER(PolishStats), C.c_void_p, C.POINTER(SpliceStats)]
    L.ioc_host_isoform_splice.restype = C.c_int64
    L.ioc_planes_isoforms_full.argtypes = [vp, i32, pi32, C.c_char_p, pi64, pi32, i32, pi32, pi32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, pi64, C.c_void_p,
                                           C.c_void_p, pi64, i32, C.c_void_p, C.c_void_p, i64, pi64, C.c_void_p, C.c_void_p, C.c_void_p, i64, pi64, C.c_void_p,
                                           C.c_void_p]
    L.ioc_align_pairs_isoforms_full.argtypes = L.ioc_align_pairs_blocks_inserts_seq.argtypes + [i32, C.c_void_p, C.c_void_p, i64, pi64, C.c_void_p, C.c_void_p,
                                                                                               C.c_void_p, i64, pi64, i64, pi64]
    a = L.ioc_host_isoform_splice.argtypes
    L.ioc_host_isoform_splice_variants.argtypes = a[:7] + [C.c_void_p] + a[7:]   # (var behind win)
    L.ioc_host_isoform_splice_variants.restype = C.c_int64
    a = L.ioc_planes_isoforms_full.argtypes
    L.ioc_planes_isoforms_full_variants.argtypes = a[:13] + [C.c_void_p] + a[13:]   # (var behind win)
    n_seq = len(L.ioc_align_pairs_blocks_inserts_seq.argtypes)
    L.ioc_align_pairs_isoforms_full_variants.argtypes = L.ioc_align_pairs_blocks_inserts_variants.argtypes + L.ioc_align_pairs_isoforms_full.argtypes[n_seq:]
    L.ioc_host_ops_extent.argtypes = [C.c_char_p, i64, i32, C.POINTER(ReadExtent)]
    L.ioc_host_reads_ends.argtypes = [C.c_void_p, C.c_void_p, i32, i32, i32, i32, i32, i32, i32, i32, i32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]
    ends_out = [i32, i32, i32, i32, i32, i32, i32]  # (the rule; the fused call has min_depth and min_alt from the block rule)
    L.ioc_reads_ends.argtypes = [vp, i32, pi32, i32, pi32, C.c_void_p, C.c_void_p] + ends_out + [C.c_void_p, C.c_void_p, i64, pi64, C.c_void_p, i64, pi64,
                                                                                                 C.c_void_p, C.c_void_p]
    L.ioc_align_pairs_blocks_ends.argtypes = L.ioc_align_pairs_blocks.argtypes + [i32, i32, i32, i32, i32, C.c_void_p, C.c_void_p, C.c_void_p, i64, pi64,
                                                                                  C.c_void_p, i64, pi64, C.c_void_p, C.c_void_p]
    L.ioc_host_read_correct_long.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, i32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, i32, i32, i32, i32, i32,
                                             C.c_void_p, C.c_void_p, i64, C.POINTER(IsoCorrectStats)]
    L.ioc_host_read_correct_long.restype = C.c_int64
    L.ioc_planes_correct_groups.argtypes = [vp, i32, pi32, C.c_char_p, pi64, pi32, i32, pi32, pi32, pi32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, i32, i32, i32, i32,
                                            C.c_void_p, C.c_void_p, i64, pi64, C.c_void_p]
    L.ioc_align_pairs_blocks_correct.argtypes = L.ioc_align_pairs_blocks.argtypes + [i32, i32, i32, i32, C.c_void_p, C.c_void_p, i64, pi64, C.c_void_p]
    L.ioc_dist_unique_id.argtypes = [pu8]
    L.ioc_dist_init.argtypes = [vp, pu8, i32, i32]
    L.ioc_dist_shutdown.argtypes = [vp]
    L.ioc_dist_info.argtypes = [vp, pi32, pi32]
    L.ioc_dist_allgather_device.argtypes = [vp, vp, vp, i64]
    L.ioc_dist_allgatherv_device.argtypes = [vp, vp, vp, pi64, pi64, i32]
    L.ioc_dist_allgather_i64.argtypes = [vp, i64, pi64]
    L.ioc_dist_allgatherv_host.argtypes = [vp, vp, i64, vp, pi64]
    L.ioc_dist_allreduce_max.argtypes = [vp, pd]
    L.ioc_dist_barrier.argtypes = [vp]
    L.ioc_dist_merge.argtypes = [vp, C.POINTER(Params), C.c_char_p, C.POINTER(BatchView), i32, i64, pi32, pi8, pi64,
                                 C.POINTER(ClusterStats), C.POINTER(DistMergeTimes)]
    L.ioc_set_shard.argtypes = [vp, i32, i32, EXCHANGE_FN, vp]
    L.ioc_shard_exchanges.argtypes = [vp]
    L.ioc_shard_aligned_pairs.argtypes = [vp]
    L.ioc_shard_aligned_pairs.restype = C.c_int64
    L.ioc_dist_exchange.argtypes = [vp, vp, i64, i32]
    L.ioc_dist_set_shard.argtypes = [vp, i32]
    L.ioc_align_set_verdict_threshold.argtypes = [vp, C.c_double]
    _lib = L
    return L
