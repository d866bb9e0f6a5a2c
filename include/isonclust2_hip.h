/*
 * isonclust2_hip.h — C ABI of the MI355X-native read->cluster assignment path of isONclust2.
 *
 * The reference has no plugin/FFI interface; its seam for this path is the C++ call
 *     StrandedCluster getBestCluster(rightId, leftBatch, rightBatch, sharedMinTab)   src/cluster.h:18-20
 * made once per read inside ClusterSortedReads (src/cluster.cpp:166), plus the index mutators
 * AddMinimizers (src/cluster.cpp:180, src/minimizer.cpp:31-42) and the sort-stage feeders
 * (src/qualscore.cpp:39-136).  This header is what a C++ maintainer binds instead: plain pointers
 * and sizes, no C++/torch types, every call returns 0 or a negative ioc_status and never throws.
 *
 * One context per GPU; a context is used by one host thread at a time (the reference `cluster`
 * is single-threaded and non-reentrant: globals at src/cluster.cpp:21-23, src/minimizer.cpp:15).
 *
 * Data model on the device (all SoA, 32-bit):
 *   queries   = the right batch's clusterable entries in loop order (src/cluster.cpp:115), each with
 *               forward and reverse minimizer lists (value, position; Index == ordinal,
 *               src/minimizer.cpp:78-123), HPC length, error-rate cell and integer pass threshold;
 *   targets   = L existing left clusters (ids 0..L-1, from the persisted MinDB) followed by the
 *               queries themselves as tentative new clusters (id L+j) — with consensus off a
 *               representative never changes (src/cluster.cpp:263-265), so (Size, totalMapped) of
 *               (query j, target t) is independent of every clustering decision;
 *   index     = open-addressed hash  minimizer value -> posting list of target ids.
 */
#ifndef ISONCLUST2_HIP_H
#define ISONCLUST2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ioc_ctx ioc_ctx;

typedef enum {
    IOC_OK = 0,
    IOC_ERR_ARG = -1,       /* bad argument / shape */
    IOC_ERR_HIP = -2,       /* HIP runtime error (ioc_last_error has the text) */
    IOC_ERR_STATE = -3,     /* call order violated */
    IOC_ERR_CAPACITY = -4,  /* a documented device-side limit was exceeded, or device memory ran out (the ioc_dist_* calls included) */
    IOC_ERR_TABLE = -5,     /* empirical probability table lookup failure (p_emp_prob.cpp:87-89) */
    IOC_ERR_NO_DEVICE = -6,
    IOC_ERR_INPUT = -7      /* input the reference would exit(1)/throw on */
} ioc_status;

/* ClsMode, src/args.h:7 */
enum { IOC_MODE_SAHLIN = 0, IOC_MODE_FAST = 1, IOC_MODE_FURIOUS = 2, IOC_MODE_NONE = 3 };

/* The clustering parameters frozen at sort time (CmdArgs, src/args.h:9-37) that the path reads
 * (src/cluster.cpp:366-369, 534-536). */
typedef struct {
    int32_t k;                /* KmerSize */
    int32_t w;                /* WindowSize */
    int32_t min_shared;       /* MinShared */
    int32_t mode;             /* IOC_MODE_* */
    double min_fraction;      /* MinFraction */
    double mapped_threshold;  /* MappedThreshold */
    double min_prob_no_hits;  /* MinProbNoHits */
    double aligned_threshold; /* AlignedThreshold (host fallback only) */
} ioc_params;

/* ---- context -------------------------------------------------------------------------------- */
int ioc_ctx_create(int device, ioc_ctx** out);
void ioc_ctx_destroy(ioc_ctx* ctx);
/* Gives the aligner's scratch (the checkpoint arena: gigabytes after an alignment-mode batch) back to the driver; the next call
 * that needs it allocates again.  A one-shot process calls this as soon as its clustering call has returned: the driver wipes
 * released VRAM before it hands it out again (8 GB: ~0.4 s), and a process that starts right after this one would otherwise
 * wait for that inside its own first large hipMalloc (profiles/r05_cli_breakdown.txt). */
int ioc_ctx_trim(ioc_ctx* ctx);
/* Optional, for a process that runs ONE batch: has the code objects of the clustering path (and of the aligner, if
 * alignment_mode != 0) loaded by background threads now, beside the caller's own preparation, instead of at each file's first
 * launch.  Returns at once; nothing depends on it. */
int ioc_ctx_prewarm(ioc_ctx* ctx, int32_t alignment_mode);
const char* ioc_last_error(const ioc_ctx* ctx);
/* Run on a caller-owned HIP stream (hipStream_t passed as void*); NULL = the context's own stream. */
int ioc_set_stream(ioc_ctx* ctx, void* hip_stream);
int ioc_synchronize(ioc_ctx* ctx);

/* Parameters + the 15x15 integer gap-limit table, gap_limit[e_cl-1][e_rd-1] =
 * max{ n : pow(1 - P(e_cl, e_rd), n) >= MinProbNoHits }: the monotone predicate of
 * getMappedRatio (src/cluster.cpp:333-347) evaluated ONCE on the host with the host libm,
 * compared as integers on the device.  ioc_host_gap_limits() fills it from the table file. */
int ioc_set_params(ioc_ctx* ctx, const ioc_params* p, const int32_t gap_limit[225]);

/* ---- queries (right batch) ------------------------------------------------------------------- */
/* Host -> device upload of the query SoA.  off_fwd/off_rev: [n+1] element offsets into
 * min_val/min_pos (total = number of minimizers, fwd and rev, of all queries; the positions of a list ascend with the index,
 * as the extractor's do: getMappedRatio subtracts consecutive ones as unsigned numbers).  err_cell in 1..15 =
 * clamp(round(100 * HpcSeq.ErrorRate)) (src/p_emp_prob.cpp:66-84).  min_total[j] = smallest integer
 * T with float(double(T)/double(hpc_len[j])) >= MappedThreshold (src/cluster.cpp:390-400). */
int ioc_queries_upload(ioc_ctx* ctx, int32_t n, const int64_t* off_fwd, const int64_t* off_rev,
                       const uint32_t* min_val, const uint32_t* min_pos, int64_t total,
                       const uint32_t* hpc_len, const uint8_t* err_cell, const uint32_t* min_total);
/* Same, with every pointer already a device pointer on ctx's device (inputs resident in HBM,
 * e.g. produced by ioc_extract_minimizers); the context borrows them until the next upload/bind. */
int ioc_queries_bind_device(ioc_ctx* ctx, int32_t n, const int64_t* d_off_fwd, const int64_t* d_off_rev,
                            const uint32_t* d_min_val, const uint32_t* d_min_pos, int64_t total,
                            const uint32_t* d_hpc_len, const uint8_t* d_err_cell,
                            const uint32_t* d_min_total, const int64_t* h_off_fwd,
                            const int64_t* h_off_rev);

/* ---- left state (merge: `cluster -l L -r R`, src/main.cpp:247-261) ----------------------------- */
/* The persisted MinDB (src/minimizer.h:60-61) as CSR: n_keys distinct values, offs[n_keys+1],
 * postings = ascending cluster ids < n_clusters.  n_clusters = 0 resets to initial clustering. */
int ioc_left_load(ioc_ctx* ctx, int32_t n_clusters, const uint8_t* cls_err_cell, int64_t n_keys,
                  const uint32_t* keys, const int64_t* offs, const uint32_t* postings);

/* UpdateMinDB (src/minimizer.cpp:124-160, called at src/cluster.cpp:296 once a cluster's consensus replaced its
 * representative): left cluster `cls` leaves the posting lists of the values only old_min has and enters, at
 * its sorted place, the lists of the values only new_min has (both arrays: the representative's forward
 * minimizer VALUES, duplicates allowed).  Lists that become empty stay as keys, unseen values open new keys
 * (`db[m]`, :146, :156).  old_min must be what the index holds for the cluster — in the reference it always
 * is (AddMinimizers / the previous UpdateMinDB put it there) — otherwise IOC_ERR_INPUT.  new_err_cell (1..15,
 * 0 = unchanged) is the cell of the representative's re-weighted HPC error rate (src/consensus.cpp:56-58, 104).
 * Device-side rewrite of the CSR; the combined index must be rebuilt afterwards (ioc_index_build). */
int ioc_index_update(ioc_ctx* ctx, int32_t cls, const uint32_t* old_min, int64_t n_old, const uint32_t* new_min,
                     int64_t n_new, uint8_t new_err_cell);
/* The left MinDB as it stands on the device (after ioc_left_load / ioc_index_update), CSR with ascending keys,
 * keys with empty lists included.  Call with keys == NULL to size. */
int ioc_left_export(ioc_ctx* ctx, int64_t* n_keys, int64_t* n_postings, uint32_t* keys, int64_t* offs,
                    uint32_t* postings);
/* After a resolved pass (ioc_resolve, ioc_cluster_batch / _merge, chunked or not): the clusters as they stand,
 * i.e. the left clusters plus every query that opened one, in final ids, BECOME the context's left state, on the device.
 * The result is what ioc_index_export followed by ioc_left_load (with the representatives' err cells) would
 * have loaded: keys strictly ascending, posting lists strictly ascending, no empty lists, the per-cluster
 * sorted value sets, the err cell of every cluster, n_left_keys / n_left_post / L updated.  The queries are
 * released (built / scored / resolved false).  *n_clusters receives the new L (may be NULL).
 * IOC_ERR_STATE without a resolved pass.
 * No key and no posting travels to the host: the next pass runs against the resident left view (ioc_left_view::n_keys
 * == -1), ioc_index_update edits the adopted state, ioc_left_export reads it back.  (After ioc_cluster_consensus the
 * MinDB lives on the host — UpdateMinDB's edits are made there — and there is nothing to adopt: IOC_ERR_STATE.) */
int ioc_left_adopt(ioc_ctx* ctx, int32_t* n_clusters);

/* ---- the hot path ---------------------------------------------------------------------------- */
/* AddMinimizers for every tentative representative at once (src/minimizer.cpp:31-42): per-query
 * sorted distinct forward values, hash insert, posting lists. */
int ioc_index_build(ioc_ctx* ctx);
/* GetMinimizerHits + ConsolidateMinimizerHits + the Size part of SortMinimizerHits
 * (src/minimizer.cpp:44-76, src/cluster.cpp:609-636) for every query against every earlier
 * target: per-query candidate lists (target, strand, Size). */
int ioc_score(ioc_ctx* ctx);
/* getBestClusterMapping + getMappedRatio (src/cluster.cpp:324-406) for all queries, iterated to the
 * unique fixed point of the greedy loop (src/cluster.cpp:115-310).  Queries listed in
 * forced_* (host decisions: alignment fallback results in sahlin mode) are taken as given.
 * n_iter (optional) receives the number of parallel sweeps. */
int ioc_resolve(ioc_ctx* ctx, int32_t* n_iter);
/* Per query: target >= 0 joined target id (left cluster id, or L + index of the query that opened
 * the cluster), -1 = opens a new cluster; strand +1/-1 (0 for new); flags bit0 = order-dependent tie
 * (>= 2 passing candidates at the winning Size: host replays the libstdc++ order), bit1 = no
 * mapping hit but top >= MinShared (sahlin/furious: host alignment fallback, cluster.cpp:553-566). */
int ioc_get_decisions(ioc_ctx* ctx, int32_t* target, int8_t* strand, uint8_t* flags);
/* Per query, the Size below which the mapping walk never looks at a candidate: int(top * MinFraction) with
 * top = the largest Size among the current clusters (cluster.cpp:381-403), or INT32_MAX when the query has no
 * walk at all (top < MinShared, or a forced decision).  Valid after ioc_resolve. */
int ioc_get_cuts(ioc_ctx* ctx, int32_t* cut);
/* Host override of one query's decision (tie replay / alignment fallback); takes effect in the
 * next ioc_resolve. target -1 = new cluster. */
int ioc_force_decision(ioc_ctx* ctx, int32_t query, int32_t target, int32_t strand);
int ioc_clear_forced(ioc_ctx* ctx);
/* Verdicts of the alignment fallback (getBestClusterAln, src/cluster.cpp:461-515), one per query:
 * target[q] = INT32_MIN (none yet), -1 (no candidate aligned: opens a cluster) or the joined target with
 * strand[q] = +1/-1.  Unlike a forced decision a verdict is used by ioc_resolve only when the query's
 * mapping walk finds nothing although top >= MinShared (flags bit1 stays set), so verdicts may be
 * supplied speculatively for many queries at once.  target == NULL switches verdicts off. */
int ioc_set_aln_verdicts(ioc_ctx* ctx, const int32_t* target, const int8_t* strand);
/* With verdicts set, ioc_resolve also reports per query the candidates tied at the top Size among the
 * current clusters — the ones getBestClusterAln tries (cluster.cpp:481-489): count[n] and up to
 * IOC_TIE_SLOTS keys per query (keys[IOC_TIE_SLOTS * q + i] = target << 1 | (strand == -1), unordered);
 * more than that: ioc_query_candidates. */
#define IOC_TIE_SLOTS 16
int ioc_get_ties(ioc_ctx* ctx, uint32_t* count, uint32_t* keys);

/* The candidate list the SCORING kernels wrote for query q (before any resolve): key = target << 1 | strand (strand bit
 * 1 = reverse), size = Size, for every (target, strand) with Size >= int(MinShared * MinFraction), in target order — in fast
 * mode: with Size >= the smallest Size that can pass the query's mapped-fraction test at all (an upper bound of totalMapped
 * from the query's minimizer positions and gap limits; IOC_SCORE_KEEPQ=0 keeps the uniform threshold).
 * Returns the count (copies at most cap).  Test instrument: lets the two builds of the scoring kernel (with / without the
 * per-posting window test, ioc_timings::score_oob) be compared histogram by histogram. */
int ioc_scored_candidates(ioc_ctx* ctx, int32_t q, int32_t cap, uint32_t* key, uint32_t* size);
/* Full candidate table of one query against the targets that are clusters under the current
 * decisions, in the fields the reference's hit map holds (src/minimizer.cpp:44-76): target id,
 * strand, Size, Index of the first hitting read minimizer, and totalMapped (0xFFFFFFFF if not
 * evaluated; 0xFFFFFFFE if the candidate was rejected without an evaluation because an upper bound of its totalMapped —
 * (Size - 1) x the widest span of a passing gap + the widest head and tail — is below the query's threshold: it fails).
 * Returns the count (<= cap) or a negative status. */
int ioc_query_candidates(ioc_ctx* ctx, int32_t query, int32_t cap, int32_t* target, int8_t* strand,
                         uint32_t* size, uint32_t* first_index, uint32_t* total_mapped);

/* MinDB after clustering (AddMinimizers applied for every query that opened a cluster): CSR with
 * final cluster ids, keys ascending.  Call with keys == NULL to size (n_keys, n_postings): the CSR is
 * built and kept on the device then, and the call with the arrays copies it straight into them. */
int ioc_index_export(ioc_ctx* ctx, int64_t* n_keys, int64_t* n_postings, uint32_t* keys,
                     int64_t* offs, uint32_t* postings);

/* ---- sort-stage feeders (src/qualscore.cpp:39-136, src/hpc.cpp:4-32, src/kmer_index.cpp:5-17,
 *      src/minimizer.cpp:78-123) ------------------------------------------------------------------ */
/* CalcQualScore / CalcErrorRate for n reads (host pointers; offs[n+1] into qual).  score[i] < 0
 * mirrors FillQualScores' -1 (src/qualscore.cpp:22-34). */
int ioc_qual_scores(ioc_ctx* ctx, int32_t n, const int64_t* offs, const uint8_t* qual, int32_t k,
                    double* score, double* err_rate);
/* HomopolymerCompress + RevComp + KmerEncodeSeq x2 + GetKmerMinimizers x2 + CalcErrorRate(hpc quals)
 * for n reads.  Outputs stay on the device in the layout ioc_queries_bind_device takes; the host
 * receives lengths/offsets/error rates.  status[i]: 0 ok, 1 HPC length < 2k or < w
 * (src/qualscore.cpp:65-73), 2 non-ACGT base (RevComp throws, src/util.cpp:31-33). */
int ioc_extract_minimizers(ioc_ctx* ctx, int32_t n, const int64_t* offs, const uint8_t* seq,
                           const uint8_t* qual, int32_t k, int32_t w, uint32_t* hpc_len,
                           double* hpc_err, int64_t* off_fwd, int64_t* off_rev, int32_t* status);
/* Device->host copy of the HPC sequences / qualities of the last ioc_extract_minimizers (ASCII; read
 * i occupies [offs[i], offs[i] + hpc_len[i]) of the buffers, which have the size of the raw input). */
int ioc_extracted_hpc_download(ioc_ctx* ctx, char* hpc_seq, char* hpc_qual, int64_t cap);
/* Device->host copy of the minimizers produced by the last ioc_extract_minimizers. */
int ioc_extracted_download(ioc_ctx* ctx, uint32_t* min_val, uint32_t* min_pos, int64_t cap);
/* Make the extracted minimizers the current queries (no host round trip of the 8 B/minimizer SoA).
 * keep[i] != 0 selects read i (gates of src/cluster.cpp:116-160 applied by the caller). */
int ioc_queries_from_extracted(ioc_ctx* ctx, const uint8_t* keep, const uint8_t* err_cell,
                               const uint32_t* min_total);

/* ---- instrumentation ------------------------------------------------------------------------ */
typedef struct {
    float ms_build;    /* ioc_index_build, HIP events on the launch stream */
    float ms_score;    /* ioc_score (the dominant kernel)                  */
    float ms_resolve;  /* ioc_resolve                                      */
    int32_t resolve_iters;
    int32_t n_queries;
    int64_t n_minimizers;      /* probes M                                  */
    int64_t n_index_postings;  /* postings stored in the device index       */
    int64_t n_candidates;      /* candidate entries written by ioc_score    */
    int64_t n_mapped_evals;    /* (query,target,strand) mapped-ratio evaluations */
    int64_t postings_traversed;/* postings read by ioc_score (if counted)   */
    /* GPU alignment fallback, summed over the ioc_align_pairs calls since the last ioc_index_build
     * (HIP events around the two passes on the launch stream) */
    float ms_align_fwd;        /* k_align_fwd: score-only DP + checkpoints   */
    float ms_align_trace;      /* k_align_trace: tiled traceback + windows   */
    int64_t n_align_pairs;
    int64_t n_align_cells;     /* sum of query length x reference length     */
    int64_t n_align_refused;   /* pairs redone: version 2 refusals on aligner version 1, split pairs whole */
    /* the scoring kernel's variant (decided once, in ioc_ctx_create): 1 = counters at the end of the LDS allocation, no
     * window test (the hardware's bounds check drops what the test would reject), 0 = window test per posting.
     * score_oob_probe: result of the context's run-time probe of that hardware behaviour — 0 passed, > 0 failed (bit 0 a
     * word of some workgroup's LDS changed, bit 1 an in-bounds counter lost an add, bit 2 the probe did not finish),
     * -1 not run (IOC_SCORE_OOB=0 / 1 forces the variant).  A failed probe selects variant 0. */
    int32_t score_oob;
    int32_t score_oob_probe;
    /* the aligner's checkpoint arena as the last ioc_align_pairs call sized it (bytes), the launches (slices) it took, and the
     * version that ran: 2 = two pairs per wave, coarse checkpoints (the default), 1 = one pair per workgroup, fine checkpoints
     * (IOC_ALIGN_ARENA=fat, pairs with letters other than A C G T, pairs the 16-bit window of version 2 refused) */
    int64_t align_arena_bytes;
    int32_t align_slices;
    int32_t align_version;
    /* cells of the DP matrices the forward pass really computed (version 2 leaves out the tiles outside its certified corridor;
     * n_align_cells stays the reference's figure: every pair's whole matrix) */
    int64_t n_align_cells_computed;
} ioc_timings;
int ioc_get_timings(ioc_ctx* ctx, ioc_timings* out);
/* Instrumentation (one extra scoring launch, outside any timed region): the number of postings the
 * reference's GetMinimizerHits would traverse on this batch = sum over queries of Size over the
 * targets that are clusters — the H of the algorithmic-bytes figure. */
int ioc_count_reference_postings(ioc_ctx* ctx, int64_t* n_postings);

/* ---- host-side helpers (pure host code, no GPU needed) ----------------------------------------- */
/* Fill gap_limit[225] and p_shared[225] for (k, w) from the table file (isonclust2_amd/data/
 * pmin_shared.bin; rows selected as src/p_emp_prob.cpp:22-47).  Returns IOC_ERR_TABLE if no row
 * matches (k outside 10..30 etc.). */
int ioc_host_gap_limits(const char* table_path, int32_t k, int32_t w, double min_prob_no_hits,
                        int32_t* gap_limit, double* p_shared);
/* clamp(round(100*e)) in 1..15, src/p_emp_prob.cpp:66-84 + src/util.cpp:6-10 */
uint8_t ioc_host_err_cell(double err_rate);
/* smallest T with float(double(T)/double(hpc_len)) >= mapped_threshold (src/cluster.cpp:390-400) */
uint32_t ioc_host_min_total(uint32_t hpc_len, double mapped_threshold);

/* ---- host alignment fallback (sahlin / furious; stays on the host, src/cluster.cpp:408-515) ------ */
/* Semi-global affine alignment replacing parasail_sg_trace_scan_16/32 + parasail_result_get_traceback
 * (src/cluster.cpp:413-419, 500-502): all four ends free, gap of length n costs open + (n-1)*extend;
 * comp receives the comparison string of the whole alignment (0x7C = identical bases, ' ' otherwise).
 * Returns its length (comp_cap >= qlen + rlen + 1).  Parity with parasail's tie-breaking is pinned only
 * by the reference's AlnRatioTest vector. */
int ioc_host_align(const char* query, int32_t qlen, const char* ref, int32_t rlen, int32_t match,
                   int32_t mismatch, int32_t gap_open, int32_t gap_extend, char* comp, int32_t comp_cap,
                   int32_t* score_out);
/* The same aligner — same cells, same walk — returning the alignment itself: one operation byte per column of comp, in forward
 * order, NUL-terminated (ops_cap >= qlen + rlen + 1); returns the length.
 *   '='  query base and reference base, equal   (comp: 0x7C)      'I'  query base against a gap
 *   'X'  query base and reference base, differ                    'D'  reference base against a gap
 *   'i' / 'd'  the same as 'I' / 'D' in a free end gap; order: leading i, leading d, the walk, trailing i, trailing d
 * comp is this string with '=' -> 0x7C and every other byte -> ' '.  This is what to diff against parasail's traceback. */
int ioc_host_align_ops(const char* query, int32_t qlen, const char* ref, int32_t rlen, int32_t match,
                       int32_t mismatch, int32_t gap_open, int32_t gap_extend, char* ops, int32_t ops_cap,
                       int32_t* score_out);
/* The same aligner restricted to a corridor of tiles, with the certificate of its result: what version 2 of the GPU aligner
 * computes under a corridor, stated on the host.  Band b holds the rows (r0, r0 + band_rows[b]] (r0: the heights before it; they
 * add up to qlen or more), strip p the columns (p strip_cols, (p + 1) strip_cols]; tile (b, p) is computed iff plo[b] <= p <= phi[b].
 * out[0 .. 8): restricted score, end row, end column | parent bound, start bound, exit bound (INT32_MIN: no such cell; parent
 * bound INT32_MAX: a skipped cell on the diagonal) | tiles skipped, tiles.  The restricted alignment is the alignment whenever
 * out[0] > min(out[3], max(out[4], out[5])).  ops (may be null, else ops_cap >= qlen + rlen + 1): the restricted alignment's
 * operation bytes; returns their length (0 without ops). */
int ioc_host_align_corridor(const char* query, int32_t qlen, const char* ref, int32_t rlen, int32_t match, int32_t mismatch,
                            int32_t gap_open, int32_t gap_extend, const int32_t* band_rows, int32_t nbands, int32_t strip_cols,
                            const int32_t* plo, const int32_t* phi, char* ops, int32_t ops_cap, int32_t* out);
/* Run-length text of an operation string ("12=1X3I...", end gaps as runs of i / d), NUL-terminated; returns its length,
 * IOC_ERR_CAPACITY if cap is too small (2 bytes per operation + 1 always suffice), IOC_ERR_ARG for a byte that is no operation. */
int64_t ioc_host_ops_to_cigar(const char* ops, int64_t len, char* out, int64_t cap);
/* What an operation string says about its alignment, in integers (parasail's _stats family gives matches, similar and length;
 * this is that and the gaps).  The WALK is the part from the first to the last byte of "=XID"; the free end gaps lie before and
 * behind it.  Leading bytes are the bytes before the first walk byte, trailing bytes the ones after the last; a string without a
 * walk byte counts all its bytes as leading.  A run is maximal over ONE byte value: 'I' next to 'i' or to 'D' ends it. */
typedef struct {
    int32_t length;       /* all bytes of the operation string */
    int32_t columns;      /* bytes in "=XID" */
    int32_t matches;      /* '=' */
    int32_t mismatches;   /* 'X' */
    int32_t ins, del;     /* 'I' bytes, 'D' bytes */
    int32_t ins_runs, del_runs;        /* maximal runs of 'I' / of 'D' */
    int32_t longest_ins, longest_del;  /* longest such run, 0 if none */
    int32_t lead_i, lead_d, trail_i, trail_d;  /* 'i' / 'd' among the leading / trailing bytes: the alignment takes the query's
                                                * bases [lead_i, query length - trail_i) and the reference's [lead_d, reference
                                                * length - trail_d) */
    int32_t reserved[2];  /* written as 0 */
} ioc_aln_stats;          /* 64 bytes */
/* The definition of the statistics (the device's k_ops_stats is tested against it); runs on the CPU.  IOC_ERR_ARG for a byte
 * that is no operation (as ioc_host_ops_to_cigar) or len >= 2^31; len == 0 gives all zeros. */
int ioc_host_ops_stats(const char* ops, int64_t len, ioc_aln_stats* out);
/* One row of a pileup: what the reads of a cluster say at one position of their reference.  A reference of length R owns R + 1
 * consecutive rows; row p is reference position p IN THE FRAME OF THE OPERATION STRING (the reverse complement of the stored
 * sequence where the pair sets ref_revcomp; the query is never complemented).  Walk a string with r = reference bases and
 * q = query bases consumed so far: 'd' r++; 'i' q++; '=' / 'X' add 1 to row r in the channel of query[q] (a, c, g, t; `other`
 * for any other byte), r++, q++; 'D' del of row r += 1, r++; 'I' ins_bases of row r += 1, and ins_runs of row r += 1 where
 * the byte before it is not 'I', q++.  So insertions belong to the position they stand in front of, row R holds insertion
 * counts only, and a + c + g + t + other + del is a row's depth. */
typedef struct {
    uint32_t a, c, g, t, other;
    uint32_t del;
    uint32_t ins_runs, ins_bases;
} ioc_pileup_col;         /* 32 bytes */
/* The definition of the pileup (the device's k_ops_pileup is tested against it); runs on the CPU.  ADDS the string's counts to
 * cols[0 .. rlen].  IOC_ERR_ARG, with cols untouched, for a byte that is no operation, for a string that does not consume
 * exactly qlen query bases and rlen reference bases, and for len >= 2^31. */
int ioc_host_ops_pileup(const char* ops, int64_t len, const char* query, int32_t qlen, int32_t rlen, ioc_pileup_col* cols);
/* What the reads insert in front of a row, beside ioc_pileup_col's ins_runs / ins_bases: a second record per row, R + 1 rows for
 * a reference of R bases.  An 'I' byte that is the j-th byte of its maximal run of 'I' (j from 0) adds 1 to
 * slot[j][channel of query[q]] of row r where j < IOC_PILE_INS_SLOTS, else to `longer`.  For one string, per row: the sum over
 * slot[0] is ins_runs, the sum over all slots plus `longer` is ins_bases. */
#define IOC_PILE_INS_SLOTS 6
typedef struct {
    uint32_t slot[IOC_PILE_INS_SLOTS][5]; /* [s][a,c,g,t,other]: reads whose insertion in front of this row has an (s+1)-th base, by that base */
    uint32_t longer;                      /* inserted bases at index >= IOC_PILE_INS_SLOTS */
    uint32_t reserved;                    /* 0 */
} ioc_pileup_ins;                          /* 128 bytes */
/* The definition of the insertion table (the ins variant of k_ops_pileup is tested against it): the walk of
 * ioc_host_ops_pileup, the same inputs refused (ins untouched), ADDS to ins[0 .. rlen]. */
int ioc_host_ops_pileup_ins(const char* ops, int64_t len, const char* query, int32_t qlen, int32_t rlen, ioc_pileup_ins* ins);
/* What a consensus call made of one reference (ioc_host_pileup_call and the device's call kernels). */
typedef struct {
    int32_t out_len;              /* bytes written */
    int32_t n_sub, n_del, n_ins;  /* positions called as another base / as deleted; inserted bases emitted */
    int32_t n_low;                /* positions below min_depth, kept as the frame has them (quality 0) */
    int32_t reserved[3];
} ioc_polish_stats;               /* 32 bytes */
/* The definition of the consensus call: the majority call over the two tables of one reference (`frame`, rlen bases, in the
 * frame of the tables).  depth(p) = a + c + g + t + other + del of row p; all arithmetic in 64 bits.  For p = 0 .. rlen:
 *  - insertions in front of p: D = depth(p) for p < rlen, depth(rlen - 1) for p == rlen, 0 for rlen == 0.  For s = 0 .. 5 in
 *    turn, n = the sum of slot[s]: the slots of the row stop unless D >= min_depth and 2n > D; else the first maximal channel
 *    of slot[s] in the order A C G T other (written 'N') is emitted with quality min(40, 40 max / D), and n_ins counts it;
 *  - the base, for p < rlen: depth(p) < min_depth: frame[p] with quality 0, n_low.  Else m = the largest of the six counters;
 *    the winner is the channel of frame[p] if its count is m, else the first maximal one in the order A C G T other del.  del:
 *    nothing is emitted, n_del; the frame's channel: frame[p] as it is; another: its letter ('N' for other), n_sub.  Quality
 *    min(40, 40 m / depth(p)).
 * Qualities are written as 33 + q.  Returns the length written (also st->out_len; st may be NULL); IOC_ERR_ARG for
 * min_depth < 1, rlen < 0 or a NULL table / frame / output that is needed; IOC_ERR_CAPACITY, with nothing written, for
 * cap < rlen + IOC_PILE_INS_SLOTS * (rlen + 1). */
int64_t ioc_host_pileup_call(const ioc_pileup_col* cols, const ioc_pileup_ins* ins, const char* frame, int32_t rlen,
                             int32_t min_depth, char* out_seq, char* out_qual, int64_t cap, ioc_polish_stats* st);
/* ---- the quality-weighted pileup and call: every vote counts by the base quality of the read that casts it ----
 * The weight of a quality byte b (as a FASTQ line has it): w(b) = 1 for b <= 34, else min(b - 33, 93) — the Phred value, at
 * least 1, so that no base of a read is ever without a vote.  Integer weights: the sums are as reproducible as the counts. */
uint32_t ioc_host_qual_weight(uint8_t b);
/* The definition of the weighted pileup (the weighted variant of k_ops_pileup is tested against it): the walk of
 * ioc_host_ops_pileup over a query with one quality byte per base (`qual`, qlen bytes).  The same inputs are refused with the
 * tables untouched, and a NULL qual with qlen > 0.  ADDS to wcols[0 .. rlen] and, where wins is not NULL, to wins[0 .. rlen];
 * the records are those of the counts, the counters hold sums of weights modulo 2^32.  '=' / 'X': the channel of query[q] in
 * row r += w(qual[q]).  'D': del of row r += the smaller of w(qual[q - 1]) (where q > 0) and w(qual[q]) (where q < qlen), 1 if
 * neither exists.  'I', the j-th byte of its maximal run: wins[r].slot[j][channel] += w(qual[q]) for j < IOC_PILE_INS_SLOTS,
 * else wins[r].longer += w(qual[q]).  'i' / 'd' add nothing; ins_runs / ins_bases of wcols are not touched. */
int ioc_host_ops_pileup_weighted(const char* ops, int64_t len, const char* query, const char* qual, int32_t qlen, int32_t rlen,
                                 ioc_pileup_col* wcols, ioc_pileup_ins* wins);
/* The definition of the weighted call.  `cols` (the counts) gates, the weights decide: Dc(p) = depth of cols[p], Dw(p) = the
 * same sum of six counters of wcols[p], in 64 bits.  For p = 0 .. rlen:
 *  - insertions in front of p: (Dc, Dw) of row p for p < rlen, of row rlen - 1 for p == rlen, (0, 0) for rlen == 0.  For
 *    s = 0 .. 5 in turn, n = the sum of wins[p].slot[s]: the slots stop unless Dc >= min_depth, Dw > 0 and 2n > Dw; else the
 *    first maximal channel of the slot in the order A C G T other ('N') is emitted with quality min(40, 40 max / Dw), n_ins;
 *  - the base, for p < rlen: Dc(p) < min_depth or Dw(p) == 0: frame[p] with quality 0, n_low.  Else m = the largest of the six
 *    counters of wcols[p]; the winner is the channel of frame[p] if its weight is m, else the first maximal one in the order
 *    A C G T other del; emitted, counted and given its quality min(40, 40 m / Dw(p)) as in ioc_host_pileup_call.
 * Capacity bound, refusals, the record and the 33 + q encoding as in ioc_host_pileup_call.  With every quality byte <= 34, or
 * all of them equal, the weighted call is the majority call byte for byte. */
int64_t ioc_host_pileup_call_weighted(const ioc_pileup_col* cols, const ioc_pileup_col* wcols, const ioc_pileup_ins* wins,
                                      const char* frame, int32_t rlen, int32_t min_depth, char* out_seq, char* out_qual, int64_t cap,
                                      ioc_polish_stats* st);
/* ---- the variable sites of a reference and every read's alleles at them: where the reads of a cluster disagree, and which
 * read is on which side.  All arithmetic in 64-bit integers; no floats. ----
 * The projection of one operation string on its reference: what ONE read says at every row.  `base` and `insf` are rlen + 1
 * bytes each; the call sets base[0 .. rlen] to IOC_ALLELE_NONE and insf[0 .. rlen] to 0 and then walks the string as
 * ioc_host_ops_pileup does (r / q: reference / query bases consumed): 'd' r++; 'i' q++; '=' / 'X' base[r] = the channel of
 * query[q] (0 .. 4 for A C G T other), r++, q++; 'D' base[r] = IOC_ALLELE_DEL, r++; 'I' insf[r] = 1 where the byte before it is
 * not 'I', q++.  So base[r] != IOC_ALLELE_NONE exactly where the read covers row r, and the sum of the projections of many reads
 * is their pileup: the six counters of ioc_pileup_col count the values 0 .. 5 of base[r], ins_runs counts insf[r] (of strings
 * with at most one run of 'I' in front of a row, as every aligner's are: a second run there would count again).  The inputs
 * ioc_host_ops_pileup refuses are refused (IOC_ERR_ARG), with both outputs untouched. */
#define IOC_ALLELE_DEL 5
#define IOC_ALLELE_NONE 7
int ioc_host_ops_project(const char* ops, int64_t len, const char* query, int32_t qlen, int32_t rlen, uint8_t* base, uint8_t* insf);
/* The insertion part of a read's projection: WHICH bases it inserts in front of every row.  `slots` holds
 * IOC_PILE_INS_SLOTS * (rlen + 1) bytes, slot-major: slots[j * (rlen + 1) + r].  The call sets all of them to 0 and then walks the
 * string exactly as ioc_host_ops_pileup_ins does: an 'I' byte that is the j-th (from 0) of its maximal run of 'I', standing in
 * front of row r and taking query[q], stores 1 + the channel of query[q] (1 .. 5 for A C G T other) at slots[j][r] where
 * j < IOC_PILE_INS_SLOTS, and nothing otherwise.  Nothing is ever cleared: a second run in front of the same row overwrites, in
 * string order.  The inputs ioc_host_ops_pileup refuses are refused (IOC_ERR_ARG), with `slots` untouched. */
int ioc_host_ops_project_ins(const char* ops, int64_t len, const char* query, int32_t qlen, int32_t rlen, uint8_t* slots);
/* One read's planes — `base` as ioc_host_ops_project writes it, `slots` as ioc_host_ops_project_ins does — ADDED to the two tables
 * of its reference, rlen + 1 rows each: base[r] in 0 .. 4 adds 1 to that channel of cols[r], IOC_ALLELE_DEL adds 1 to del,
 * IOC_ALLELE_NONE adds nothing; a slot byte s in 1 .. 5 at slots[j][r] adds 1 to ins[r].slot[j][s - 1] and 1 to cols[r].ins_bases,
 * and a non-zero slots[0][r] adds 1 to cols[r].ins_runs; `longer` is never touched.  Any other byte, a negative rlen or a NULL:
 * IOC_ERR_ARG, with both tables untouched.
 * The relation to the pileup: for a string with at most one run of 'I' in front of any row — every string an aligner returns is
 * one — the tables piled from its planes equal ioc_host_ops_pileup and ioc_host_ops_pileup_ins of the string in every field but
 * two: ins_bases, which counts at most IOC_PILE_INS_SLOTS bases per run here, and `longer`, which stays 0.  The consensus call
 * reads neither (pile_call_row), so ioc_host_pileup_call gives the same sequence, qualities and record from either pair of tables.
 * That is what the planes are kept for: the tables of ANY subset of a cluster's reads can be added up after the alignments are
 * gone — the two sides of a split (ioc_planes_polish, ioc_align_pairs_split_polish). */
int ioc_host_planes_pile(const uint8_t* base, const uint8_t* slots, int32_t rlen, ioc_pileup_col* cols, ioc_pileup_ins* ins);
/* The weight part of a read's projection: the weight of every vote the read casts, kept beside its planes.  `wbase` holds rlen + 1
 * bytes and `wslots` IOC_PILE_INS_SLOTS * (rlen + 1), slot-major like `slots` of ioc_host_ops_project_ins.  The call sets all of
 * them to 0 and then walks the string as ioc_host_ops_pileup_weighted does: a '=' / 'X' at row r taking query[q] stores
 * w(qual[q]) (ioc_host_qual_weight) at wbase[r]; a 'D' at row r stores the deletion weight of ioc_host_ops_pileup_weighted — the
 * smaller of the weights of the query bases on its two sides where they exist, 1 where neither does; the j-th 'I' of its run,
 * j < IOC_PILE_INS_SLOTS, stores w(qual[q]) at wslots[j][r].  A weight is 1 .. 93, so a byte holds one, and 0 says "no vote".
 * Nothing is ever cleared: a second run in front of the same row overwrites, in string order.  What ioc_host_ops_pileup_weighted
 * refuses is refused (IOC_ERR_ARG), with both outputs untouched. */
int ioc_host_ops_project_weights(const char* ops, int64_t len, const char* query, const char* qual, int32_t qlen, int32_t rlen, uint8_t* wbase,
                                 uint8_t* wslots);
/* One read's planes and weight planes ADDED to the two tables of weights of its reference, rlen + 1 rows each: base[r] in 0 .. 5
 * adds wbase[r] to that counter (a c g t other del) of wcols[r]; a slot byte s in 1 .. 5 at slots[j][r] adds wslots[j][r] to
 * wins[r].slot[j][s - 1].  ins_runs and ins_bases of wcols and `longer` of wins are never touched, and the sums are modulo 2^32.
 * What ioc_host_planes_pile refuses, a NULL weight plane and a NULL table: IOC_ERR_ARG, with both tables untouched.
 * The relation to the weighted pileup: for a string with at most one run of 'I' in front of any row the tables piled this way
 * from ioc_host_ops_project / _project_ins / _project_weights equal those of ioc_host_ops_pileup_weighted in every field but
 * `longer`, which the weighted call (ioc_host_pileup_call_weighted) does not read.  So the weighted consensus of ANY subset of a
 * cluster's reads can be called after the alignments are gone: group-segment (g, h) of ioc_planes_polish_groups_weighted is
 * ioc_host_pileup_call_weighted(gcols, gwcols, gwins, frame of g, min_depth) with gcols from ioc_host_planes_pile and gwcols /
 * gwins from this function over the pairs of segment g in group h. */
int ioc_host_planes_pile_weighted(const uint8_t* base, const uint8_t* slots, const uint8_t* wbase, const uint8_t* wslots, int32_t rlen,
                                  ioc_pileup_col* wcols, ioc_pileup_ins* wins);
/* One variable site.  kind IOC_SITE_BASE: the alleles are the channels 0 .. 5 (A C G T other del) of row `row`; kind
 * IOC_SITE_INS: the alleles are 0 (no insertion in front of row `row`) and 1 (one).  depth / n_major / n_minor are the 64-bit
 * values of the definition below, saturated at 2^32 - 1. */
#define IOC_SITE_BASE 0
#define IOC_SITE_INS 1
typedef struct {
    int32_t row, kind;
    int32_t major, minor;
    uint32_t depth, n_major, n_minor;
    uint32_t reserved; /* 0 */
} ioc_pile_site;       /* 32 bytes */
/* The definition of the sites of one reference from its table of counts (rlen + 1 rows).  depth(p) as in ioc_host_pileup_call;
 * D(p) = depth(p) for p < rlen, depth(rlen - 1) for p == rlen, 0 for rlen == 0; need(D) = max(min_alt, (min_pct * D + 99) / 100).
 * For p = 0 .. rlen in turn, the insertion site of row p before its base site:
 *  - insertion site: with = ins_runs(p), without = D(p) > with ? D(p) - with : 0.  A site iff D(p) >= min_depth,
 *    with >= need(D(p)) and without >= need(D(p)).  major = 1 where with > without, else 0 (a tie goes to "absent"); depth = D(p);
 *  - base site, p < rlen: iff depth(p) >= min_depth and n_minor >= need(depth(p)), where major is the first maximal of the six
 *    counters in the order A C G T other del and minor the first maximal of the other five in that order.
 * The first max_sites sites in this order are written to `out`; returns how many were written, and *n_found (may be NULL) is how
 * many there were: n_found > max_sites says that the list was cut.  IOC_ERR_ARG for min_depth < 1, min_alt < 1, min_pct outside
 * 1 .. 50, max_sites < 1, rlen < 0 or a NULL cols / out. */
int64_t ioc_host_pileup_sites(const ioc_pileup_col* cols, int32_t rlen, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                              int32_t max_sites, ioc_pile_site* out, int64_t* n_found);
/* The alleles of one read (its projection) at n_sites sites of its reference: out[s] = base[row] at a base site; at an insertion
 * site insf[row] where the read spans the row — base[row] != IOC_ALLELE_NONE for row < rlen, rlen > 0 and
 * base[rlen - 1] != IOC_ALLELE_NONE for row == rlen — else IOC_ALLELE_NONE.  IOC_ERR_ARG for a negative count or length, a NULL
 * that is needed, a row outside 0 .. rlen, a base site at row rlen and a kind that is neither; `out` is then untouched. */
int ioc_host_site_alleles(const uint8_t* base, const uint8_t* insf, int32_t rlen, const ioc_pile_site* sites, int32_t n_sites,
                          uint8_t* out);
/* ---- the split of a cluster's reads in two by linked variable sites: which sites vary together, and which side of that
 * pattern each read is on.  Integers only. ----
 * One segment: n_sites kept sites and n_reads reads; `alleles` is read-major, alleles[i * n_sites + s] the allele of read i at
 * site s, as ioc_host_site_alleles writes it.
 *  - mark:    m(i, s) = +1 where the byte equals sites[s].minor, else -1 where it equals sites[s].major, else 0 (a third allele,
 *             IOC_ALLELE_NONE, any other byte).
 *  - linkage: d(s, t) = the sum over the reads of m(i, s) * m(i, t): reads that agree minus reads that disagree, among those that
 *             have a say at both sites.  link(s) = the sum of |d(s, t)| over t != s with |d(s, t)| >= min_link (64 bits).
 *  - seed:    the first site with the largest link.  Without sites, or with a largest link of 0, there is NO SPLIT: seed -1,
 *             every phase 0, every group IOC_SPLIT_NONE, every vote 0.
 *  - phase:   phase(seed) = +1; for t != seed, phase(t) = sign(d(seed, t)) where |d(seed, t)| >= min_link, else 0.
 *  - vote:    vote(i) = the sum over t of phase(t) * m(i, t).  Read i is in group 1 where vote >= min_margin, in group 0 where
 *             vote <= -min_margin, else IOC_SPLIT_NONE.  Group 1 starts as the side that carries the seed's minor allele.
 *  - rounds:  exactly `rounds` times, no early exit: g(i) = +1 / -1 / 0 for a read of group 1 / group 0 / neither;
 *             dg(t) = the sum over the reads of g(i) * m(i, t); phase(t) = sign(dg(t)) where |dg(t)| >= min_link, else 0 (the
 *             seed's too); then the vote again.  This carries the split along a reference that no read spans.
 * out_link[s] = link(s), out_phase[s] and out_group[i] / out_vote[i] are the final ones; the record: seed, n_linked (sites whose
 * final phase is not 0), n_reads, the reads of group 0, of group 1 and of neither, and link(seed) (0 without a split).  Any of
 * out_link / out_phase / out_vote may be NULL.  IOC_ERR_ARG, with nothing written, for min_link < 1, min_margin < 1, rounds
 * outside 0 .. 64, a negative count and a NULL that is needed (out_seg; out_group with reads; sites with sites; alleles with
 * both).  This function is the plain triple loop, O(n_sites^2 * n_reads): it is the definition, ioc_site_split.hip the fast
 * form.  Whether a split is "real" is the caller's reading of n_linked, n_group0 and n_group1: the library applies no verdict. */
#define IOC_SPLIT_NONE 255
typedef struct {
    int32_t seed, n_linked;
    int32_t n_reads, n_group0, n_group1, n_none;
    int64_t seed_link;
} ioc_split_seg; /* 32 bytes */
int ioc_host_alleles_split(const ioc_pile_site* sites, int32_t n_sites, const uint8_t* alleles, int32_t n_reads, int32_t min_link,
                           int32_t min_margin, int32_t rounds, int64_t* out_link, int8_t* out_phase, uint8_t* out_group,
                           int32_t* out_vote, ioc_split_seg* out_seg);
int32_t ioc_host_gap_open(double e1_plus_e2);                    /* setGapOpen,  src/cluster.cpp:425-440 */
/* Which kernel family the batched GPU aligner gives a pair of four-letter sequences with these scoring parameters (a pair with
 * another letter always takes 0): 0 the comparing kernel (32-bit cells), 1 the query-profile kernel with 32-bit cells, 2 version 2
 * (query profiles, 16-bit cells) may take it.  With cm = match + gap_extend + gap_open and cx = mismatch + gap_extend + gap_open:
 * 1 and 2 need 0 <= cm, cx <= 255; 2 also gap_open >= gap_extend and max(cm, cx) <= 31.  No result depends on the family. */
int ioc_host_align_route(int32_t match, int32_t mismatch, int32_t gap_extend, int32_t gap_open);
double ioc_host_aln_ratio(const char* comp, int32_t comp_len, double e, uint32_t slen, uint32_t k);
                                                                  /* getAlnRatio, src/cluster.cpp:442-459 */

/* ---- the same alignment on the GPU, batched (getBestClusterAln's ParasailAlign + getAlnRatio,
 * src/cluster.cpp:408-423, 442-459, 498-507) ------------------------------------------------------- */
/* One pair = read `query` against representative `ref` (indices into the sequence pool), the reference
 * optionally reverse-complemented (RevComp, src/util.cpp:13-38; cluster.cpp:491-495); e = sum of the two
 * raw error rates (cluster.cpp:497), which selects the gap-open penalty (setGapOpen) and the per-window
 * match limit floor((1-e)k).  Results are bit-identical to ioc_host_align + ioc_host_aln_ratio. */
typedef struct {
    int32_t query;
    int32_t ref;
    int32_t ref_revcomp;
    int32_t reserved;   /* 0, or a HINT > 0: any measure of how much alike the caller expects the two sequences to be that can be
                         * compared across the pairs of one call (the cluster drivers pass the query's cut, i.e. its top count of
                         * shared minimizers).  The aligner schedules pairs hinted far below the call's median together; no result
                         * depends on it. */
    double e;
} ioc_aln_pair;
/* Upload the sequence pool (concatenated raw sequences, offs[n_seqs + 1], offs[0] == 0). */
int ioc_align_set_pool(ioc_ctx* ctx, int32_t n_seqs, const char* seqs, const int64_t* offs);
/* Align n_pairs pairs; any of the outputs may be NULL.  out_windows = number of qualifying k-windows
 * (`aligned` of getAlnRatio), out_ratio = out_windows / query length (its return value).
 * Accepted scoring parameters, for this call and every ioc_align_pairs_* form: gap_extend >= 0;
 * w = max(|match|, |mismatch|) + 2 gap_extend + 5 at most 2^24; and w x (query length + reference length) at most 2^30 for
 * every pair with two non-empty sequences (match 2, mismatch -2, gap_extend 1: every pair the pool can hold).  Within that
 * range the results are ioc_host_align's, whatever the sign of the parameters, gap_extend above gap_open included.  Anything
 * else is refused with IOC_ERR_ARG before an output is written. */
int ioc_align_pairs(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match,
                    int32_t mismatch, int32_t gap_extend, int32_t* out_score, int64_t* out_windows,
                    double* out_ratio);
/* ioc_align_pairs + the alignments themselves (the operation bytes of ioc_host_align_ops, byte for byte, relative to the
 * reverse-complemented reference where ref_revcomp is set).  The bytes of pair i are out_ops[ops_off[i] .. ops_off[i + 1])
 * — packed, forward order, not NUL-terminated; ops_off has n_pairs + 1 entries.  ops_cap >= ioc_align_ops_bound(...) (the sum
 * over the pairs of query length + reference length; negative ioc_status for a pair outside the pool), else IOC_ERR_CAPACITY
 * and nothing is written.  The counts are always exact: the verdict threshold below is not applied to this call (and stays
 * set for the next ioc_align_pairs).  IOC_ALIGN_VARIANT=carry has no walk: this call takes the traced route regardless.
 * Any of out_score / out_windows / out_ratio may be NULL.  The device buffer of the bytes shares the checkpoint arena's
 * budget: a call whose bound does not fit beside the arena runs in slices. */
int64_t ioc_align_ops_bound(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs);
int ioc_align_pairs_ops(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match,
                        int32_t mismatch, int32_t gap_extend, int32_t* out_score, int64_t* out_windows,
                        double* out_ratio, char* out_ops, int64_t ops_cap, int64_t* ops_off);
/* ioc_align_pairs + the statistics of the alignments (ioc_host_ops_stats of what ioc_align_pairs_ops would return for the same
 * pairs, field by field), reduced ON THE DEVICE: the walks write their bytes as for ioc_align_pairs_ops, a kernel of its own
 * (k_ops_stats) counts them there, and 64 bytes per pair come back in place of the bytes themselves.  An emitting call like
 * ioc_align_pairs_ops: always exact, the verdict threshold not applied, IOC_ALIGN_VARIANT=carry not honoured, the device buffer
 * of the bytes counted against the checkpoint arena's budget.  out_stats (n_pairs records, zeroed first) must not be NULL when
 * n_pairs > 0; any of out_score / out_windows / out_ratio may be. */
int ioc_align_pairs_stats(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match,
                          int32_t mismatch, int32_t gap_extend, int32_t* out_score, int64_t* out_windows,
                          double* out_ratio, ioc_aln_stats* out_stats);
/* ioc_align_pairs + the pileup of the alignments on their references, reduced ON THE DEVICE (k_ops_pileup): pair i adds what
 * ioc_host_ops_pileup makes of its operation string and its query into rows row_base[i] .. row_base[i] + reference length of
 * out_cols (n_rows records, zeroed first).  Pairs that share a row_base are piled together; they must then have references of
 * one length, taken in one frame — the caller's business.  Every pair adds exactly once, whichever run answered it.
 * IOC_ERR_ARG, with nothing written, for row_base[i] < 0, row_base[i] + reference length + 1 > n_rows, n_rows < 0, and a NULL
 * row_base or out_cols with n_pairs > 0.  out_stats != NULL: the records of ioc_align_pairs_stats as well, from the same
 * alignments.  An emitting call like ioc_align_pairs_stats: always exact, the verdict threshold not applied,
 * IOC_ALIGN_VARIANT=carry not honoured; the device table (32 bytes per row) and the operation bytes count against the
 * checkpoint arena's budget.  Any of out_score / out_windows / out_ratio may be NULL. */
int ioc_align_pairs_pileup(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match,
                           int32_t mismatch, int32_t gap_extend, int32_t* out_score, int64_t* out_windows,
                           double* out_ratio, ioc_aln_stats* out_stats, const int64_t* row_base, int64_t n_rows,
                           ioc_pileup_col* out_cols);
/* The consensus call of many references at once ON THE DEVICE (ioc_pile_call.hip), from host tables that are uploaded: segment
 * g is a reference of rlen[g] bases, its frame at frames + frame_off[g], its rlen[g] + 1 rows of `cols` / `ins` from the sum
 * over the earlier segments of (rlen + 1) on.  Segment g's sequence and qualities, as ioc_host_pileup_call defines them, stand
 * at out_seq / out_qual + out_off[g] .. out_off[g + 1] (packed, in segment order; out_off has n_segs + 1 entries), its record in
 * out_stats[g] (may be NULL).  For callers who add pileups up over several calls before they call.  IOC_ERR_ARG for
 * min_depth < 1, a negative rlen or a NULL array that is needed; IOC_ERR_CAPACITY, with nothing written, for cap below the
 * sum of the segments' bounds (rlen + IOC_PILE_INS_SLOTS * (rlen + 1) each), and for a segment whose bound exceeds 2^31 - 1. */
int ioc_pileup_call(ioc_ctx* ctx, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off,
                    const ioc_pileup_col* cols, const ioc_pileup_ins* ins, int32_t min_depth, char* out_seq, char* out_qual,
                    int64_t cap, int64_t* out_off, ioc_polish_stats* out_stats);
/* A segment of ioc_align_pairs_polish: the pool sequence that is its frame, reverse-complemented where ref_revcomp is set. */
typedef struct {
    int32_t ref;
    int32_t ref_revcomp;
} ioc_polish_seg;
/* ioc_align_pairs + the polished consensus of every segment: the pairs are aligned, pair i is piled into both tables (the ins
 * variant of k_ops_pileup) at the rows of segment seg_of_pair[i], the segments are called on the device where the tables lie,
 * and the sequences, qualities, offsets and records come back as from ioc_pileup_call (out_polish: n_segs records).  The tables
 * come back only where asked for: out_cols / out_ins (sum of frame length + 1 rows, may be NULL).  A segment without pairs
 * returns its frame with quality 0 throughout.  An emitting call like ioc_align_pairs_pileup: always exact, the verdict
 * threshold not applied, IOC_ALIGN_VARIANT=carry not honoured; both device tables (160 bytes per row) count against the
 * checkpoint arena's budget.  IOC_ERR_ARG, with nothing written, for a pair whose reference length differs from its segment's
 * frame, seg_of_pair outside the segments, a segment or pair outside the pool and min_depth < 1; IOC_ERR_CAPACITY for cap
 * below the sum of the per-segment bounds.  out_stats and any of out_score / out_windows / out_ratio may be NULL. */
int ioc_align_pairs_polish(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch,
                           int32_t gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio,
                           ioc_aln_stats* out_stats, int32_t n_segs, const ioc_polish_seg* segs, const int32_t* seg_of_pair,
                           int32_t min_depth, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off,
                           ioc_polish_stats* out_polish, ioc_pileup_col* out_cols, ioc_pileup_ins* out_ins);
/* One quality byte per byte of the current pool, at the same offsets (n_bytes: the pool's total, else IOC_ERR_ARG): what
 * ioc_align_pairs_polish_weighted weights the reads' votes by.  A NULL `quals` drops them; every ioc_align_set_pool drops them. */
int ioc_align_set_pool_qual(ioc_ctx* ctx, const char* quals, int64_t n_bytes);
/* ioc_pileup_call with the weighted decision (ioc_host_pileup_call_weighted per segment): `cols` gates, `wcols` / `wins` decide;
 * all three are uploaded, rows as in ioc_pileup_call.  The same refusals, and a NULL wcols / wins with n_segs > 0. */
int ioc_pileup_call_weighted(ioc_ctx* ctx, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off,
                             const ioc_pileup_col* cols, const ioc_pileup_col* wcols, const ioc_pileup_ins* wins, int32_t min_depth,
                             char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_stats);
/* ioc_align_pairs_polish by weight: pair i is piled by the weighted variant of k_ops_pileup — the counts into a first table as
 * ioc_align_pairs_polish piles them (bit-identical), the weights of ioc_host_ops_pileup_weighted, under the qualities of
 * ioc_align_set_pool_qual, into two more — and the segments are called on the device as ioc_host_pileup_call_weighted defines.
 * The tables come back only where asked for (out_cols, out_wcols, out_wins; each may be NULL).  An emitting call like the
 * others: always exact, no verdict threshold, IOC_ALIGN_VARIANT=carry not honoured, all three device tables (192 bytes per
 * row) counted against the checkpoint arena's budget, every pair added exactly once.  Refuses, with nothing written, what
 * ioc_align_pairs_polish refuses, and with IOC_ERR_ARG a pool without qualities. */
int ioc_align_pairs_polish_weighted(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match,
                                    int32_t mismatch, int32_t gap_extend, int32_t* out_score, int64_t* out_windows,
                                    double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs, const ioc_polish_seg* segs,
                                    const int32_t* seg_of_pair, int32_t min_depth, char* out_seq, char* out_qual, int64_t cap,
                                    int64_t* out_off, ioc_polish_stats* out_polish, ioc_pileup_col* out_cols,
                                    ioc_pileup_col* out_wcols, ioc_pileup_ins* out_wins);
/* The sites of many references at once ON THE DEVICE (ioc_pile_sites.hip), from a host table that is uploaded: segment g is a
 * reference of rlen[g] bases, its rows laid out as in ioc_pileup_call.  Segment g's sites, as ioc_host_pileup_sites defines them
 * (at most max_sites of them), stand at out_sites[site_off[g] .. site_off[g + 1]) — packed, in segment order; site_off has
 * n_segs + 1 entries — and n_found[g] is how many it has in all.  IOC_ERR_ARG for what ioc_host_pileup_sites refuses;
 * IOC_ERR_CAPACITY, with nothing written, for sites_cap below the sum over the segments of min(max_sites, 2 * rlen + 1). */
int ioc_pileup_sites(ioc_ctx* ctx, int32_t n_segs, const int32_t* rlen, const ioc_pileup_col* cols, int32_t min_depth,
                     int32_t min_alt, int32_t min_pct, int32_t max_sites, ioc_pile_site* out_sites, int64_t sites_cap,
                     int64_t* site_off, int64_t* n_found);
/* ioc_align_pairs + the variable sites of every segment and every pair's alleles at them, all ON THE DEVICE: the pairs are
 * aligned, pair i is piled into the table of counts at the rows of segment seg_of_pair[i] (k_ops_pileup) and projected into two
 * byte planes of its own (k_ops_project: ioc_host_ops_project of its operation string, 2 * (reference length + 1) bytes), the
 * sites of every segment are found where the table lies (ioc_host_pileup_sites: out_sites, site_off, n_found as from
 * ioc_pileup_sites), and pair i's alleles at the kept sites of its segment (ioc_host_site_alleles) stand at
 * out_alleles[allele_off[i] .. allele_off[i + 1]) — one byte per (read, site); allele_off has n_pairs + 1 entries.  What comes
 * back is that, not the alignments.  Segments as in ioc_align_pairs_polish, and its refusals (a pair whose reference length
 * differs from its segment's frame, seg_of_pair outside the segments, a segment or pair outside the pool — that the pairs of
 * a segment take their references in one frame stays the caller's business, as there); IOC_ERR_ARG as well for the thresholds
 * ioc_host_pileup_sites refuses.  IOC_ERR_CAPACITY, with nothing written, for sites_cap below the
 * sum over the segments of min(max_sites, 2 * rlen + 1) and alleles_cap below the sum over the pairs of the same bound of their
 * segment.  A segment without pairs has no sites.  out_cols (the table, sum of rlen + 1 rows), out_stats and any of out_score /
 * out_windows / out_ratio may be NULL.  An emitting call like the others: always exact, no verdict threshold,
 * IOC_ALIGN_VARIANT=carry not honoured; the table (32 bytes per row) and the planes count against the checkpoint arena's budget,
 * every pair is added and projected exactly once. */
int ioc_align_pairs_alleles(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch,
                            int32_t gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio,
                            ioc_aln_stats* out_stats, int32_t n_segs, const ioc_polish_seg* segs, const int32_t* seg_of_pair,
                            int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_sites, ioc_pile_site* out_sites,
                            int64_t sites_cap, int64_t* site_off, int64_t* n_found, uint8_t* out_alleles, int64_t alleles_cap,
                            int64_t* allele_off, ioc_pileup_col* out_cols);
/* The split of many segments at once ON THE DEVICE (ioc_site_split.hip: bit planes and popcounts, no atomics, every output word
 * has one writer), from host tables that are uploaded: segment g has the sites sites[site_off[g] .. site_off[g + 1]) and the
 * pairs i with seg_of_pair[i] == g as its reads, in ascending i; pair i's alleles stand at alleles[allele_off[i] ..
 * allele_off[i + 1]), one byte per site of its segment (the layout ioc_align_pairs_alleles returns).  Per segment what
 * ioc_host_alleles_split defines: out_link / out_phase per site (at the sites' positions), out_group / out_vote per pair, out_seg
 * per segment; any of out_link / out_phase / out_vote may be NULL.  IOC_ERR_ARG, with nothing written, for what the host function
 * refuses, seg_of_pair outside the segments, offsets that do not start at 0 or descend, and an allele_off row whose length is not
 * its segment's site count. */
int ioc_alleles_split(ioc_ctx* ctx, int32_t n_segs, int32_t n_pairs, const int32_t* seg_of_pair, const ioc_pile_site* sites,
                      const int64_t* site_off, const uint8_t* alleles, const int64_t* allele_off, int32_t min_link,
                      int32_t min_margin, int32_t rounds, int64_t* out_link, int8_t* out_phase, uint8_t* out_group,
                      int32_t* out_vote, ioc_split_seg* out_seg);
/* ioc_align_pairs_alleles with the split run where the alleles lie: the sites, site_off and n_found come back as from that call,
 * and the split's outputs as from ioc_alleles_split (out_link / out_phase: sites_cap entries; out_group / out_vote: n_pairs;
 * out_seg: n_segs; out_group and out_seg are needed, the others may be NULL).  out_alleles (with alleles_cap) and out_cols are
 * optional: NULL, not copied; allele_off (n_pairs + 1 entries) always comes back.  The same refusals and capacity checks
 * (alleles_cap is checked where out_alleles is given), and those of ioc_host_alleles_split.  Every pair is aligned, piled and projected exactly once.
 * The split's own device memory — the bit planes (16 bytes per site and 64 reads of its segment), 21 bytes per site, 21 per pair
 * and 32 per segment — is allocated after the walks have finished, so it does not count against the checkpoint arena's budget. */
int ioc_align_pairs_split(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch,
                          int32_t gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats,
                          int32_t n_segs, const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_depth, int32_t min_alt,
                          int32_t min_pct, int32_t max_sites, ioc_pile_site* out_sites, int64_t sites_cap, int64_t* site_off,
                          int64_t* n_found, uint8_t* out_alleles, int64_t alleles_cap, int64_t* allele_off, ioc_pileup_col* out_cols,
                          int32_t min_link, int32_t min_margin, int32_t rounds, int64_t* out_link, int8_t* out_phase,
                          uint8_t* out_group, int32_t* out_vote, ioc_split_seg* out_seg);
/* The polished consensus of each side of a split, from the reads' planes, ON THE DEVICE.  Group-segment 2 g + h (segment g, group
 * h in {0, 1}) is ioc_host_pileup_call(frame of g, min_depth) on the tables piled (ioc_host_planes_pile) from the planes of the
 * pairs i with seg_of_pair[i] == g and group[i] == h; pairs in IOC_SPLIT_NONE are in no table, and a group-segment without reads
 * returns its frame with quality 0 throughout.  The library applies no verdict on whether the split is real.
 * This entry works from host planes, which are uploaded: segment g has rlen[g] bases and its frame at frames + frame_off[g] (as
 * for ioc_pileup_call); pair i's rows start at the sum over the earlier pairs of (their segment's rlen + 1), P rows in all, and
 * the planes are base[P] and slots[IOC_PILE_INS_SLOTS * P], slot-major over the whole array (slot j of row x at slots[j * P + x]).
 * k_plane_pile adds the planes of every group's reads up (a lane per row, the waves of a workgroup share the reads, no atomics:
 * every table word has one writer) and the call kernels of ioc_pileup_call run over the 2 * n_segs group-segments: out_off has
 * 2 * n_segs + 1 entries, out_polish (may be NULL) 2 * n_segs records, and out_gcols / out_gins (optional, both or either) receive
 * the tables, the sum over g of 2 * (rlen[g] + 1) rows, in group-segment order.  Plane bytes other than those the two projections
 * write count for nothing.  IOC_ERR_ARG, with nothing written, for min_depth < 1, a negative count, length or frame offset,
 * seg_of_pair outside the segments, a group byte other than 0, 1 or IOC_SPLIT_NONE and a NULL array that is needed;
 * IOC_ERR_CAPACITY, with nothing written, for cap below twice the sum of the segments' bounds (ioc_pileup_call) and for a segment
 * whose bound exceeds 2^31 - 1. */
int ioc_planes_polish(ioc_ctx* ctx, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off,
                      int32_t n_pairs, const int32_t* seg_of_pair, const uint8_t* group, const uint8_t* base, const uint8_t* slots,
                      int32_t min_depth, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_polish,
                      ioc_pileup_col* out_gcols, ioc_pileup_ins* out_gins);
/* The same for ANY NUMBER of groups a segment: the consensus of every isoform of a cluster.  Segment g has n_groups[g] >= 0 groups
 * and pair i is in group[i] of its segment, -1 .. n_groups[seg_of_pair[i]] - 1 (-1: in no table).  The group-segments are numbered
 * in segment order — segment g's are gseg_off[g] .. gseg_off[g + 1], gseg_off the prefix sum of n_groups, G = gseg_off[n_segs] in
 * all — and group-segment (g, h) is ioc_host_pileup_call(frame of g, min_depth) on the tables piled (ioc_host_planes_pile) from the
 * planes of the pairs i with seg_of_pair[i] == g and group[i] == h; it owns the rows of both tables from the sum over the earlier
 * group-segments of (rlen of their segment + 1) on.  A group-segment without reads returns its frame with quality 0 throughout.
 * With n_groups[g] == 2 everywhere this is the row and index layout of ioc_planes_polish.  The library applies no verdict on whether
 * an isoform is real.  The planes are host planes laid out as for ioc_planes_polish.  k_group_pile (ioc_group_pile.hip) adds them
 * up: a workgroup per 64 rows of a group-segment that has reads walks that group's own member list — the lists are made on the
 * host, 4 bytes a pair — with two members in flight per wave, no atomics, one writer per table word; the call kernels of
 * ioc_pileup_call run over the G group-segments.  out_off has G + 1 entries, out_polish (may be NULL) G records, and out_gcols /
 * out_gins (optional, both or either) receive the tables, the sum over g of n_groups[g] * (rlen[g] + 1) rows.  IOC_ERR_ARG, with
 * nothing written, for what ioc_planes_polish refuses, a negative n_groups[g], a group[i] outside -1 .. n_groups[seg] - 1 and a G
 * above 2^31 - 1; IOC_ERR_CAPACITY, with nothing written, for cap below the sum over g of n_groups[g] * the bound of segment g
 * (ioc_pileup_call) and for a segment whose bound exceeds 2^31 - 1. */
int ioc_planes_polish_groups(ioc_ctx* ctx, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off,
                             const int32_t* n_groups, int32_t n_pairs, const int32_t* seg_of_pair, const int32_t* group,
                             const uint8_t* base, const uint8_t* slots, int32_t min_depth, char* out_seq, char* out_qual, int64_t cap,
                             int64_t* out_off, ioc_polish_stats* out_polish, ioc_pileup_col* out_gcols, ioc_pileup_ins* out_gins);
/* ioc_planes_polish_groups with every read's vote counted by its weight: the quality-weighted consensus of every isoform of a
 * cluster.  wbase / wslots are the host weight planes of the pairs (ioc_host_ops_project_weights), laid out as base / slots are and
 * uploaded beside them.  Group-segment (g, h) is ioc_host_pileup_call_weighted(gcols, gwcols, gwins, frame of g, min_depth), gcols
 * piled by ioc_host_planes_pile and gwcols / gwins by ioc_host_planes_pile_weighted from the pairs i with seg_of_pair[i] == g and
 * group[i] == h; numbering, row ownership and the group without reads (its frame at quality 0) are those of
 * ioc_planes_polish_groups.  k_group_pile_weighted (ioc_group_pile_weighted.hip) adds up the three tables, 14 bytes a member and
 * row, and the weighted mode of the call kernels runs over the G group-segments.  out_gcols / out_gwcols / out_gwins (each
 * optional) receive the tables: ins_runs / ins_bases of gwcols and `longer` / `reserved` of gwins are 0, and gcols is what
 * ioc_planes_polish_groups returns.  With n_groups[g] == 2 everywhere this is the weighted consensus of both sides of a split.
 * IOC_ERR_ARG / IOC_ERR_CAPACITY, with nothing written, for what ioc_planes_polish_groups refuses, and IOC_ERR_ARG for a NULL
 * wbase or wslots with n_pairs > 0. */
int ioc_planes_polish_groups_weighted(ioc_ctx* ctx, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off,
                                      const int32_t* n_groups, int32_t n_pairs, const int32_t* seg_of_pair, const int32_t* group,
                                      const uint8_t* base, const uint8_t* slots, const uint8_t* wbase, const uint8_t* wslots, int32_t min_depth,
                                      char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_polish,
                                      ioc_pileup_col* out_gcols, ioc_pileup_col* out_gwcols, ioc_pileup_ins* out_gwins);
/* ioc_align_pairs_split with the consensus of both groups of every segment called where the planes lie: everything
 * ioc_align_pairs_split returns comes back unchanged, and behind the split k_plane_pile and the call kernels run over the planes
 * the walks left — k_ops_project's base plane and the six slot planes of k_ops_project_ins, 8 bytes per row and pair in all,
 * which count against the checkpoint arena's budget like the table — with the groups the split just made: out_seq / out_qual /
 * out_off / out_polish / out_gcols / out_gins as from ioc_planes_polish, the frame of segment g being its representative as the
 * pairs were aligned against it.  Every pair is aligned, piled and projected exactly once: no read is aligned a second time for
 * its group's consensus.  The group tables (160 bytes per row and group-segment) are reserved after the walks have finished, like
 * the split's memory.  The refusals of ioc_align_pairs_split and of ioc_planes_polish (polish_min_depth < 1, cap, a NULL out_off,
 * NULL out_seq / out_qual where something may be written); nothing is written on any of them. */
int ioc_align_pairs_split_polish(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch,
                                 int32_t gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio,
                                 ioc_aln_stats* out_stats, int32_t n_segs, const ioc_polish_seg* segs, const int32_t* seg_of_pair,
                                 int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_sites, ioc_pile_site* out_sites,
                                 int64_t sites_cap, int64_t* site_off, int64_t* n_found, uint8_t* out_alleles, int64_t alleles_cap,
                                 int64_t* allele_off, ioc_pileup_col* out_cols, int32_t min_link, int32_t min_margin, int32_t rounds,
                                 int64_t* out_link, int8_t* out_phase, uint8_t* out_group, int32_t* out_vote, ioc_split_seg* out_seg,
                                 int32_t polish_min_depth, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off,
                                 ioc_polish_stats* out_polish, ioc_pileup_col* out_gcols, ioc_pileup_ins* out_gins);
/* Verdict mode.  The clustering loop only ever asks whether out_ratio >= AlignedThreshold (src/cluster.cpp:503).  With a
 * threshold > 0 set here, the traceback of a pair may stop as soon as that comparison is decided — the count of good windows
 * has reached the smallest count whose ratio passes (what is still to come can only add), or can no longer reach it (every
 * further column of the alignment ends at most one more window) — and out_windows / out_ratio are then lower bounds that
 * compare with the threshold exactly as the full counts would (out_score is always exact).  <= 0 (the default): exact
 * counts.  The cluster drivers (ioc_cluster_batch / merge / consensus) switch it on around their own alignment batches
 * unless IOC_ALIGN_VERDICT=0. */
int ioc_align_set_verdict_threshold(ioc_ctx* ctx, double aligned_threshold);

/* The minimizer lists of the entries `entries[0..n_idx)` of the context's CURRENT queries (ioc_queries_upload /
 * ioc_queries_from_extracted / the batch of the last ioc_cluster_batch), gathered on the device into caller-owned
 * DEVICE buffers in the compact layout of ioc_batch_view (all forward lists, then all reverse lists): what a rank
 * contributes to the merge's all-gather — the representatives' records never leave HBM (src/cluster.cpp:537: a right
 * cluster is matched through its representative's Mins / RevMins).  off_fwd / off_rev [n_idx + 1] (host) receive the
 * offsets; cap = capacity of the two buffers in words.  Returns the number of words written or a negative status. */
/* Generation of the context's queries: changes whenever they are replaced (ioc_queries_upload, ioc_queries_bind_device,
 * ioc_queries_from_extracted, every ioc_cluster_* driver call).  A caller that keeps entry numbers of a batch for a later
 * ioc_gather_records_device compares the value it saw after the clustering call. */
int64_t ioc_queries_generation(const ioc_ctx* ctx);
int64_t ioc_gather_records_device(ioc_ctx* ctx, int32_t n_idx, const int32_t* entries, uint32_t* d_out_min,
                                  uint32_t* d_out_pos, int64_t cap, int64_t* off_fwd, int64_t* off_rev);

/* ---- host driver: ClusterSortedReads on flat arrays (src/cluster.cpp:67-322, consensus off) ------ */
typedef struct {
    /* right batch, one record per entry in loop order */
    int32_t n;
    const int64_t* off_fwd;    /* [n+1] */
    const int64_t* off_rev;    /* [n+1] */
    const uint32_t* min_val;
    const uint32_t* min_pos;
    int64_t total;
    const uint32_t* raw_len;   /* RawSeq length        */
    const uint32_t* hpc_len;   /* HpcSeq length        */
    const double* score;       /* RawSeq Score()       */
    const double* raw_err;     /* RawSeq ErrorRate()   */
    const double* hpc_err;     /* HpcSeq ErrorRate()   */
    const uint8_t* state;      /* 0 clusterable, 1 null placeholder (skipped, cluster.cpp:125) */
    double min_qual;           /* CmdArgs::MinQual     */
    /* merge only (right batch already clustered: one record per right cluster, the arrays above
     * describe its representative, cluster.cpp:537): */
    /* sahlin / furious only: raw sequences for the host alignment fallback (cluster.cpp:461-515) */
    const char* raw_seq;       /* RawSeq->Str() of all entries, concatenated; NULL in fast mode */
    const int64_t* raw_off;    /* [n+1] */
    const int32_t* n_members;  /* reads[i]->size() - 1; NULL = fresh reads */
    int32_t depth;             /* right Batch::Depth; the MinClsSize filter applies when > 0 (:119-123) */
    int32_t min_cls_size;      /* left SortArgs.MinClsSize after the -A override (main.cpp:329-331) */
    /* several clustered batches merged in ONE pass (the left fold ((b0 + b1) + b2) ... of freshly clustered batches makes
     * the decisions of one loop over b0's, b1's, ... representatives in that order: cluster.cpp:178-217 only appends):
     * entries with is_cluster[i] != 0 are the leftmost batch's clusters — they keep their cluster (ids in entry order)
     * without being matched, exactly as if they had come in through ioc_left_view.  NULL: none. */
    const uint8_t* is_cluster;
    /* != 0: min_val / min_pos are DEVICE pointers (e.g. the output of ioc_gather_records_device after an RCCL
     * all-gather); they are used in place and must stay valid until the context's queries are replaced.  Entries
     * that the gates skip must then carry no minimizers. */
    int32_t minimizers_on_device;
} ioc_batch_view;

/* Left batch of a merge (`cluster -l L -r R`): its clusters' representative HPC error rates and the
 * persisted MinDB as CSR (keys strictly ascending, posting lists strictly ascending cluster ids). */
typedef struct {
    int32_t n_clusters;
    const double* cls_hpc_err; /* [n_clusters] HpcSeq->ErrorRate() of each representative */
    int64_t n_keys;            /* -1 with keys == NULL: keep the left state that is on the device
                                  (ioc_left_load or ioc_left_adopt, then any ioc_index_update); n_clusters must match it */
    const uint32_t* keys;
    const int64_t* offs;       /* [n_keys+1] */
    const uint32_t* postings;
    /* sahlin / furious only: the representatives' raw sequences and raw error rates */
    const char* rep_seq;
    const int64_t* rep_off;    /* [n_clusters+1] */
    const double* cls_raw_err; /* RawSeq->ErrorRate() of each representative */
} ioc_left_view;

typedef struct {
    int64_t n_clusters;
    int64_t n_joined;
    int64_t n_gated;
    int64_t n_tie_replays;
    int64_t n_aln_invoked;   /* reads that reached the alignment fallback (ALN_INVOKED, cluster.cpp:21,559) */
    int32_t resolve_iters;
    int32_t aln_rounds;      /* verdict rounds of the alignment fallback driver */
    int64_t n_aln_pairs;     /* (read, candidate, strand) pairs actually aligned */
    int64_t n_aln_order_dep; /* verdicts that depended on the reference's candidate order */
    int64_t n_cons_invoked;  /* representatives replaced by a consensus (CONS_INVOKED, cluster.cpp:22,295) */
    int64_t n_cons_restarts; /* device passes of ioc_cluster_consensus (one + one per consensus event) */
} ioc_cluster_stats;

/* Initial clustering of one sorted batch (`cluster -l batch.cer`, src/main.cpp:262-275):
 * out_cls[i] = final cluster id of entry i (-1 if gated), out_strand[i] = MatchStrand after the
 * flips of src/cluster.cpp:235-246 (+1 for entries that open a cluster). */
int ioc_cluster_batch(ioc_ctx* ctx, const ioc_params* p, const char* table_path,
                      const ioc_batch_view* right, int32_t* out_cls, int8_t* out_strand,
                      ioc_cluster_stats* stats);
/* Merge (`cluster -l L -r R`, src/cluster.cpp:67-322 with both batches real): every right cluster's
 * representative is a query against the left MinDB; out_cls[i] = left cluster the right cluster i
 * ends up in (existing id, or a new id >= left->n_clusters in creation order, or -1 if filtered),
 * out_strand[i] = +1 / -1 (-1: every member's MatchStrand flips, :235-246).  left == NULL is
 * ioc_cluster_batch.  ioc_index_export afterwards returns the merged MinDB.  (The arrays of `right`
 * are read until the call returns: a large batch's reverse lists and positions are still being
 * uploaded, by a thread of the library, while the first kernels run.)
 * A right batch of more than 131 072 entries (one device pass: the all-pairs candidate tables grow with the square of the
 * entries) runs in chunks of that many, in order, each against the left state the chunks before it left behind — the
 * reference's one loop; the results are those of one pass.  Between two chunks the clustering so far is adopted as the left
 * state on the device (ioc_left_adopt); the call may start from a resident left state.  After such a call the context's resident queries are the last
 * chunk's (ioc_gather_records_device refuses).  No limit on a read's length: queries of more than 8192 forward minimizers
 * are sorted in global memory instead of LDS (src/minimizer.cpp:78-123 has plain vectors). */
int ioc_cluster_merge(ioc_ctx* ctx, const ioc_params* p, const char* table_path, const ioc_left_view* left,
                      const ioc_batch_view* right, int32_t* out_cls, int8_t* out_strand,
                      ioc_cluster_stats* stats);
/* ---- consensus mode (ConsMaxSize > 0; src/cluster.cpp:200-204, 263-309, src/consensus.cpp) -------------------- */
/* The partial-order graphs of the consensus (spoa in the reference) stay with the caller, behind the operations
 * the reference performs on them.  side 0 = leftBatch->ConsGs[idx] (idx = left cluster id), side 1 =
 * rightBatch->ConsGs[idx] (idx = right entry; merges).  Every callback returns >= 0, or < 0 to abort. */
typedef struct {
    const char* raw_seq;      /* the consensus = new RawSeq->Str() of the representative (consensus.cpp:93) */
    int32_t raw_len;
    char raw_qual;            /* every quality character of it (consensus.cpp:98-100) */
    double raw_err;           /* RawSeq->ErrorRate(): weighted mean (consensus.cpp:60-62) */
    double raw_score;         /* RawSeq->Score() = raw_err * length (consensus.cpp:96) */
    const char* hpc_seq;      /* HomopolymerCompress of the consensus */
    int32_t hpc_len;
    double hpc_err;           /* HpcSeq->ErrorRate(): weighted mean (consensus.cpp:56-58, 121) */
    const uint32_t* fwd_min;  /* Mins (Index = ordinal), consensus.cpp:123 */
    const uint32_t* fwd_pos;
    int32_t n_fwd;
    const uint32_t* rev_min;  /* RevMins, consensus.cpp:124 */
    const uint32_t* rev_pos;
    int32_t n_rev;
    int32_t entry;            /* right entry whose join triggered it (the name is cons_<BatchNr>_<entry>, cluster.cpp:280-282) */
} ioc_rep_record;
typedef struct {
    void* user;
    int (*create)(void* user, int side, int idx, const char* seq, int len);                 /* new graph + AddSeqToGraph(seq, 1), cluster.cpp:200-204 */
    int (*size)(void* user, int side, int idx);                                             /* sequences().size(); < 0: no such graph */
    int (*add)(void* user, int side, int idx, const char* seq, int len, unsigned weight);   /* AddSeqToGraph, consensus.cpp:76-81 */
    int (*consensus)(void* user, int side, int idx, char* out, int cap);                    /* GenerateConsensus -> length, consensus.cpp:87 */
    int (*purge)(void* user, int side, int idx, const char* seq, int len, unsigned weight); /* ConsPurge, consensus.cpp:128-137 */
    void (*rep_changed)(void* user, int32_t cls, const ioc_rep_record* rec);                /* optional: the pointers die with the call */
    /* OPTIONAL (NULL: every consensus is taken at once, as the reference does): a graph store that can DEFER consensus
     * requests and undo tagged operations lets the driver collect the consensus events of many clusters of a pass and
     * have their graph additions aligned in ONE batch (the reference's result is unchanged: the driver verifies, once
     * the new representatives are known, that no entry it walked past them could see one, and rolls back otherwise). */
    const struct ioc_consensus_spec_ops* spec;
} ioc_consensus_ops;
/* tag = the right-batch entry that caused the operation (ascending over a call of ioc_cluster_consensus) */
typedef struct ioc_consensus_spec_ops {
    int (*create_tagged)(void* user, int side, int idx, const char* seq, int len, int tag);
    int (*add_tagged)(void* user, int side, int idx, const char* seq, int len, unsigned weight, int tag);
    /* GenerateConsensus of graph (side, idx) as it is after the additions queued so far: computed by flush(), fetched
     * by collect() (returns the length) */
    int (*consensus_deferred)(void* user, int side, int idx, int tag);
    /* safe_tag: operations tagged below it are never rolled back — the store may work them off in the same batches */
    int (*flush)(void* user, int safe_tag);
    int (*collect)(void* user, int side, int idx, int tag, char* out, int cap);
    /* undo every operation tagged >= first_tag (graphs, queued additions, deferred results); commit: forget how to */
    int (*rollback)(void* user, int first_tag);
    int (*commit)(void* user);
} ioc_consensus_spec_ops;
typedef struct {
    int32_t cons_min_size;      /* CmdArgs::ConsMinSize */
    int32_t cons_max_size;      /* CmdArgs::ConsMaxSize; <= 0: no consensus (graphs are still created, as in the reference) */
    int32_t cons_period;        /* CmdArgs::ConsPeriod */
    int32_t left_depth;         /* leftBatch->Depth on entry: -1 for a freshly sorted batch (qualscore.cpp:102) */
    const int32_t* left_sizes;  /* cls[c]->size() of the left clusters (ConsPeriod test, cluster.cpp:267-271); NULL = 2 each */
} ioc_consensus_args;
/* ClusterSortedReads with the consensus branch: same inputs and outputs as ioc_cluster_merge (left host MinDB
 * required, right raw sequences required).  The device pipeline runs over all remaining entries; the host
 * walks the decisions in the reference's order up to the first join that replaces a representative
 * (UpdateClusterConsensus), re-minimizes the consensus on the GPU, applies UpdateMinDB and resumes behind that
 * entry.  ioc_index_export afterwards returns the final MinDB (emptied lists included, minimizer.cpp:150-152). */
int ioc_cluster_consensus(ioc_ctx* ctx, const ioc_params* p, const char* table_path, const ioc_left_view* left,
                          const ioc_batch_view* right, const ioc_consensus_args* args, const ioc_consensus_ops* ops,
                          int32_t* out_cls, int8_t* out_strand, ioc_cluster_stats* stats);

/* ---- a POA engine of its own behind those five operations (spoa is absent from the reference tree: parity with
 * spoa's alignments and consensus tie-breaks is unpinned).  Graphs and heaviest-bundle consensus on the host, the
 * sequence-to-graph DP (local, global or semi-global alignment — `cluster -A`, src/main.cpp:292-324 —, convex gaps as
 * two affine pieces, src/main.cpp:285-290: m 4, n -8, g -8, e -4, q -20, c -1) on the GPU.  Limits: sequences
 * < 2^20 bases, graphs < 2^21 nodes (more of either: IOC_ERR_CAPACITY from the operation that meets it), <= 127
 * predecessors per node; cell scores are int32 (negative in global and semi-global alignment).
 * The six scores: m >= 0, n <= 0, g <= e <= 0, q <= c <= 0 (a gap is never cheaper to open than to extend: the row scan
 * relies on it), and each within int8, -128 .. 127, the type the reference passes them in — with the two size limits
 * that keeps every cell's arithmetic inside int32 and apart from the engine's "no value" sentinel (derived at
 * ioc_poa_create_mode in ioc_poa.hip).  Anything else: IOC_ERR_ARG from create.
 * The DP's rows: 0 = a virtual source, 1..R = the nodes in topological order; columns 0..L = the read;
 * gap(k) = max(g + (k-1) e, q + (k-1) c).
 *   local:        H >= 0 everywhere (row 0 and column 0: 0); the best cell of the matrix ends it; the walk ends at a 0.
 *   global:       row 0: gap(j); column 0: the vertical moves from row 0; ends in column L of a sink (no out-edges);
 *                 the walk ends at (0, 0): read bases left on row 0 are insertions (-1, pos), nodes on column 0 (node, -1).
 *   semi-global:  row 0: gap(j); column 0: 0; ends in column L of any node or in any column of a sink; the walk ends on
 *                 row 0 or column 0 (a read head left on row 0 is unaligned, as in local alignment).
 * Among end cells the first maximum in (row, column) order wins.  A graph does not record the type that built it. ---- */
#define IOC_POA_LOCAL 0       /* numbered like `cluster -A` (spoa kSW) */
#define IOC_POA_GLOBAL 1      /* (kNW) */
#define IOC_POA_SEMI_GLOBAL 2 /* (kOV) */
typedef struct ioc_poa ioc_poa;
/* ioc_poa_create: local alignment.  ioc_poa_create_mode: mode = IOC_POA_*, anything else IOC_ERR_ARG. */
int ioc_poa_create(ioc_ctx* ctx, int32_t m, int32_t n, int32_t g, int32_t e, int32_t q, int32_t c, ioc_poa** out);
int ioc_poa_create_mode(ioc_ctx* ctx, int32_t mode, int32_t m, int32_t n, int32_t g, int32_t e, int32_t q, int32_t c, ioc_poa** out);
void ioc_poa_destroy(ioc_poa* poa);
/* fills user + create / size / add / consensus / purge + spec of *ops (rep_changed is left to the caller) */
void ioc_poa_bind(ioc_poa* poa, ioc_consensus_ops* ops);
/* inspection: a graph's nodes (letter, topological order) and weighted edges; the alignment (node id or -1,
 * position or -1, forward order) and score of the last `add`.  Returns the number of pairs. */
int ioc_poa_graph_export(ioc_poa* poa, int side, int idx, int32_t* n_nodes, int32_t* n_edges, char* bases, int32_t* rank,
                         int32_t* edge_from, int32_t* edge_to, int64_t* edge_w);
int ioc_poa_last_alignment(ioc_poa* poa, int32_t cap, int32_t* nodes, int32_t* pos, int32_t* score);
/* persistence across `.cer` files (one graph per cluster, src/serialize.h:21,37; the blob layout is this build's
 * own): save returns the size (out == NULL to size), load replaces graph (side, idx). */
int64_t ioc_poa_graph_save(ioc_poa* poa, int side, int idx, uint8_t* out, int64_t cap);
int ioc_poa_graph_load(ioc_poa* poa, int side, int idx, const uint8_t* in, int64_t len);
/* count graphs at once (idx[x] <- the blob in[x] of len[x] bytes), parsed on the host's cores; all or none. */
int ioc_poa_graph_load_many(ioc_poa* poa, int side, int32_t count, const int32_t* idx, const uint8_t* const* in, const int64_t* len);

/* The same pipeline on queries already resident on the device (bench: inputs in HBM). n entries
 * must all be clusterable.  Fast mode, or sahlin mode after ioc_resident_set_sequences. */
int ioc_cluster_resident(ioc_ctx* ctx, int32_t* out_cls, int8_t* out_strand, ioc_cluster_stats* stats);
/* Raw sequences (RawSeq->Str(), concatenated; raw_off[n + 1]) and raw error rates of the resident
 * queries, for the alignment fallback of sahlin mode (cluster.cpp:491-497). */
int ioc_resident_set_sequences(ioc_ctx* ctx, const char* raw_seq, const int64_t* raw_off, const double* raw_err);

/* ---- multi-GPU: the merge's exchange step over RCCL; one process and one context per GPU -------------
 * Initial clustering shards batches one per GPU and needs no communication (the reference pipeline runs one `cluster`
 * process per batch, README.md:105-117).  The merge (`cluster -l L -r R`, src/cluster.cpp:67-322 with two batches) matches a
 * right cluster through its representative's Mins / RevMins (src/cluster.cpp:537-539): what travels between GPUs is the
 * representatives' records.  A context owns one communicator; rank 0 makes the id and the host program ships its 128 bytes
 * to the other ranks however it likes (a file, a socket, MPI, torch.distributed). */
#define IOC_DIST_ID_BYTES 128
int ioc_dist_unique_id(uint8_t* id /* [IOC_DIST_ID_BYTES] */);
int ioc_dist_init(ioc_ctx* ctx, const uint8_t* id, int32_t rank, int32_t world);   /* ncclCommInitRank on the context's device */
int ioc_dist_shutdown(ioc_ctx* ctx);
int ioc_dist_info(const ioc_ctx* ctx, int32_t* rank, int32_t* world);              /* (0, 1) without a communicator */
/* collectives on the context's stream.  *_device: device buffers, HBM to HBM; the others stage host data through HBM and
 * return when the result is in the caller's arrays. */
int ioc_dist_allgather_device(ioc_ctx* ctx, const void* d_send, void* d_recv, int64_t bytes_per_rank);
/* ragged: rank r contributes counts[r] elements of esize bytes, landing at d_recv + displs[r] * esize on every rank; a
 * rank's d_send may be its own slot of d_recv.  counts / displs [world]: host arrays, identical on every rank. */
int ioc_dist_allgatherv_device(ioc_ctx* ctx, const void* d_send, void* d_recv, const int64_t* counts, const int64_t* displs,
                               int32_t esize);
int ioc_dist_allgather_i64(ioc_ctx* ctx, int64_t mine, int64_t* all /* [world] */);
/* ragged host records in rank order; sizes [world] receives the byte counts (recv == NULL: only the sizes) */
int ioc_dist_allgatherv_host(ioc_ctx* ctx, const void* send, int64_t bytes, void* recv, int64_t* sizes);
int ioc_dist_allreduce_max(ioc_ctx* ctx, double* x);
int ioc_dist_barrier(ioc_ctx* ctx);
typedef struct {
    float ms_exchange_lists;   /* the four ragged all-gathers of the minimizer lists (HIP events on the stream) */
    double ms_merge;           /* the one-pass merge on this rank (wall) */
    int64_t bytes_lists;       /* this rank's contribution: minimizer lists ... */
    int64_t bytes_records;     /* ... and per-representative records + raw sequences */
    int32_t sharded;           /* 1: score + resolve were sharded over the ranks (ioc_set_shard) */
    int32_t exchanges;         /* all-reduces the sharded resolve issued */
} ioc_dist_merge_times;
/* Sharded score + resolve (fast mode): with world > 1 the context scores and decides only the queries j with
 * j % world == rank (the same queries, index and forced decisions on every rank), and after each sweep of the resolve the
 * ranks' shares of `valid` and the sweep's control words are combined through `fn`: an in-place all-reduce over `count`
 * elements of DEVICE memory at d_buf, ordered after the work already on the context's stream (hip_stream) — kind
 * IOC_XCHG_MAX_U8 (bytes, maximum), IOC_XCHG_MIN_U32 (words, minimum) or IOC_XCHG_SUM_I32 (words, sum); non-zero = failure.
 * The decisions end up complete on every rank; they are those of the unsharded resolve (a query's decision depends on its
 * own candidates and on `valid` of earlier queries only).  sahlin / furious contexts and ioc_cluster_consensus ignore the
 * setting (their alignment rounds / windowed passes read per-query state of all queries); ioc_scored_candidates of a query
 * another rank owns reports no candidates.  world <= 1 or fn == NULL switches it off.  ioc_dist_merge installs an RCCL
 * exchange by itself (IOC_DIST_SHARD=0 keeps the replicated merge); the hook exists for other transports and for tests. */
#define IOC_XCHG_MAX_U8 0
#define IOC_XCHG_MIN_U32 1
#define IOC_XCHG_SUM_I32 2
typedef int (*ioc_exchange_fn)(void* user, void* d_buf, int64_t count, int32_t kind, void* hip_stream);
int ioc_set_shard(ioc_ctx* ctx, int32_t world, int32_t rank, ioc_exchange_fn fn, void* user);
/* all-reduces issued by the last ioc_resolve (0: it was not sharded) */
int32_t ioc_shard_exchanges(const ioc_ctx* ctx);
/* sahlin / furious: scoring and resolve stay replicated under ioc_set_shard (their tie sets read every query's candidates), the
 * ALIGNMENT rounds are shared out by owner of the query (a pair's result is a function of its two sequences, cluster.cpp:408-459);
 * the verdicts of a round travel as one summed word array through the same hook.  Pairs this rank has aligned since
 * ioc_set_shard: */
int64_t ioc_shard_aligned_pairs(const ioc_ctx* ctx);
/* The RCCL form of that exchange over the context's communicator (ioc_dist_init), on the context's stream: directly, and
 * installed as the context's shard setting with the communicator's world and rank (on = 0 removes it). */
int ioc_dist_exchange(ioc_ctx* ctx, void* d_buf, int64_t count, int32_t kind);
int ioc_dist_set_shard(ioc_ctx* ctx, int32_t on);

/* The merge of ALL ranks' freshly clustered batches (Depth 0), on every rank: the left fold ((b0 + b1) + b2) ... in rank order
 * makes the decisions of ONE greedy loop over the representatives of b0, b1, ... in which b0's are clusters from the start
 * (ioc_batch_view::is_cluster: src/cluster.cpp:178-217 only appends).  reps = THIS rank's cluster representatives, one record
 * each in cluster order (compact lists; min_val / min_pos host or device per reps->minimizers_on_device — e.g. the output of
 * ioc_gather_records_device; raw_seq / raw_off for sahlin / furious).  out_counts [world] receives the clusters of every
 * rank; out_cls / out_strand [sum of counts] the decision for every gathered representative in rank order, as
 * ioc_cluster_merge reports them (call with out_cls == NULL to learn the counts first).  ioc_index_export afterwards returns
 * the merged MinDB. */
int ioc_dist_merge(ioc_ctx* ctx, const ioc_params* p, const char* table_path, const ioc_batch_view* reps, int32_t min_cls_size,
                   int64_t out_cap, int32_t* out_cls, int8_t* out_strand, int64_t* out_counts, ioc_cluster_stats* stats,
                   ioc_dist_merge_times* times);

/* ---- Read correction: every read held against the pileup of its cluster ----
 * What one read looks like once its cluster has corrected it.  Inputs: the read's own planes — base[rlen + 1] as
 * ioc_host_ops_project writes it and slots[IOC_PILE_INS_SLOTS][rlen + 1], slot-major, as ioc_host_ops_project_ins does — the two
 * tables of its reference (rlen + 1 rows each), the reference itself (`frame`) and a rule {min_depth >= 1, min_alt >= 1, min_pct in
 * 1 .. 50, max_run in 0 .. 64}.  All integers.  depth(p) is the depth of ioc_host_pileup_call, D(p) and need(D) = max(min_alt,
 * ceil(min_pct * D / 100)) are those of ioc_host_pileup_sites; a plane byte neither projection writes counts for nothing; letters
 * are written by channel, "ACGTN".  A cluster holds a gene, not one molecule, so this is no majority vote: an allele that enough
 * reads share is kept.
 *  The base of row p < rlen, where own = base[p] is a channel or IOC_ALLELE_DEL; cnt[] is the row of cols:
 *   1. depth(p) < min_depth: "low" — the read's own base (nothing for a deletion) at quality 0; counted in n_low.
 *   2. cnt[own] >= need(depth(p)): "keep".
 *   3. otherwise w is the winner of ioc_host_pileup_call's base decision (the frame's channel where its count is maximal, else the
 *      first maximal of A C G T other del): w == own "keep", own a deletion "fill" with w, w a deletion "remove", else "sub" with w.
 *  The run guard: a maximal run of consecutive rows decided "fill" — rows the read does not cover and rows decided otherwise end
 *  it — of more than max_run rows turns back to "keep", row by row counted in n_guarded; "remove" likewise, on its own; "sub" never.
 *  (A read of an isoform that lacks an exon keeps lacking it.)  max_run 0 applies no fill and no remove at all.
 *  Keep emits the read's own base, sub and fill emit w, remove and a kept deletion emit nothing; an emitted base of channel c has
 *  quality min(40, 40 * cnt[c] / depth(p)).
 *  The insertions in front of row p, 0 <= p <= rlen, where the read spans the row (ioc_host_site_alleles), D = D(p):
 *   D < min_depth: the read's own slot bytes in slot order at quality 0.  Else for slot j = 0 .. 5 in turn, with n_j the sum of
 *   ins[p].slot[j], cons_j = cons_(j-1) and 2 * n_j > D (the call's prefix rule), letter_j the first maximal channel and own =
 *   slots[j][p]:  own set and ins[p].slot[j][own - 1] >= need(D): own is emitted;  own set and not supported: letter_j where cons_j
 *   holds (n_sub), else nothing (n_ins_drop);  own not set, cons_j, and max(D - n_j, 0) < need(D): letter_j (n_ins_add).  Quality:
 *   min(40, 40 * the slot's count of the emitted channel / D).
 * A row emits its insertions and then its base, 7 bytes at most.  Qualities are written as 33 + q: they say how much of the
 * cluster supports the base, not what the sequencer said. */
typedef struct {
    int32_t out_len, n_sub, n_fill, n_remove;
    int32_t n_ins_add, n_ins_drop, n_low, n_guarded;
} ioc_correct_stats;              /* 32 bytes */
/* The definition: one read.  Returns the length written to out_seq / out_qual (no terminator); *st (may be NULL) the record.
 * IOC_ERR_ARG for a rule outside the ranges above, rlen < 0 or a NULL array that is needed, IOC_ERR_CAPACITY for cap below
 * rlen + IOC_PILE_INS_SLOTS * (rlen + 1); nothing is written on either. */
int64_t ioc_host_read_correct(const uint8_t* base, const uint8_t* slots, int32_t rlen, const ioc_pileup_col* cols,
                              const ioc_pileup_ins* ins, const char* frame, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                              int32_t max_run, char* out_seq, char* out_qual, int64_t cap, ioc_correct_stats* st);
/* Every pair of many segments at once on the device, from host planes and host tables, all of which are uploaded: the segments,
 * their frames and the tables as for ioc_pileup_call, the pairs and their planes as for ioc_planes_polish.  k_read_correct
 * (ioc_read_correct.hip) takes a wave per pair, a lane per row: a count pass, a scan, and a write pass into a buffer as large as
 * the count says.  Pair i's corrected sequence and qualities stand packed at out_off[i] .. out_off[i + 1] of out_seq / out_qual
 * (out_off: n_pairs + 1 entries), its record in out_stats[i] (may be NULL); each as ioc_host_read_correct defines it.
 * IOC_ERR_ARG, with nothing written, for a rule outside its ranges, a negative count, length or frame offset, seg_of_pair outside
 * the segments and a NULL array that is needed; IOC_ERR_CAPACITY, with nothing written, for cap below the sum over the pairs of
 * their segment's bound (ioc_pileup_call) and for a segment whose bound exceeds 2^31 - 1. */
int ioc_planes_correct(ioc_ctx* ctx, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off,
                       const ioc_pileup_col* cols, const ioc_pileup_ins* ins, int32_t n_pairs, const int32_t* seg_of_pair,
                       const uint8_t* base, const uint8_t* slots, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_run,
                       char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_correct_stats* out_stats);
/* ioc_align_pairs_polish's alignment and pileup with every pair projected beside it (the base plane and the six slot planes, 8
 * bytes per row and pair, which count against the checkpoint arena's budget like the tables), and behind the walks k_read_correct
 * over the tables and the planes where they lie: scores, windows, ratio, out_stats, the segments and out_cols / out_ins (optional)
 * as from ioc_align_pairs_polish, out_seq / out_qual / out_off / out_correct per PAIR as from ioc_planes_correct, the frame of a
 * segment being its representative as the pairs were aligned against it.  Every pair is aligned, piled and projected exactly
 * once.  A pair without an alignment (an empty query or reference) has nothing in the planes and comes back empty.  The stage's
 * own memory is reserved after the walks.  The refusals of ioc_align_pairs_polish and of ioc_planes_correct; nothing is written. */
int ioc_align_pairs_correct(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch,
                            int32_t gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats,
                            int32_t n_segs, const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_depth, int32_t min_alt,
                            int32_t min_pct, int32_t max_run, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off,
                            ioc_correct_stats* out_correct, ioc_pileup_col* out_cols, ioc_pileup_ins* out_ins);

/* ---- Exon blocks: the stretches of a representative that some of its cluster's reads skip, and every read's isoform ----
 * One segment is a reference of rlen rows with n_reads reads, each read its base plane base[0 .. rlen] as ioc_host_ops_project
 * writes it: a byte of 0 .. 5 (a channel or IOC_ALLELE_DEL) covers the row, any other byte does not; row rlen takes part in
 * nothing.  A rule {min_gap >= 1, min_depth >= 1, min_alt >= 1, min_pct in 1 .. 50, min_block >= 1, max_blocks in 1 .. 32}.  All
 * integers.
 *  1. A long gap of a read: a maximal run of consecutive rows p < rlen with base[p] == IOC_ALLELE_DEL of at least min_gap rows (no
 *     upper length).  G_i(p) is 1 on the rows of read i's long gaps.
 *  2. The row table: D(p) the reads that cover row p, in(p) the sum of G_i(p); need(D) = max(min_alt, ceil(min_pct * D / 100)) as
 *     in ioc_host_pileup_sites.  Row p is variable iff D(p) >= min_depth, in(p) >= need(D(p)) and D(p) - in(p) >= need(D(p)).
 *  3. A block [first, end): a maximal run of variable rows of at least min_block rows.  In ascending order; the first max_blocks
 *     are kept, n_found says how many there were (n_found > max_blocks: the list was cut).
 *  4. A read's state at a kept block of len rows, of which it covers c and has s deleted (ANY deleted row, not only those of long
 *     gaps: one stray match cuts a long gap into pieces shorter than min_gap): c < len IOC_BLOCK_NONE, else 4 s >= 3 len
 *     IOC_BLOCK_SKIP, else 4 s <= len IOC_BLOCK_KEEP, else IOC_BLOCK_PART.
 *  5. The signature: key = the sum over the kept blocks b of state(b) << (2 b).  A read is complete when no state is NONE; a
 *     segment without blocks gives every read the complete key 0.
 *  6. The keys carried by at least min_alt complete reads are supported; in ascending UNSIGNED order they are the isoforms 0 ..
 *     n_groups - 1.  A complete read of a supported key: that isoform, IOC_ISO_DIRECT; of another key: -1, IOC_ISO_RARE.  An
 *     incomplete read with a state that is not NONE and exactly one supported key that agrees with it at every block where its
 *     state is not NONE: that isoform, IOC_ISO_ASSIGNED; any other incomplete read: -1, IOC_ISO_AMBIGUOUS.
 * No verdict on whether two isoforms are real is applied: that stays the reader's judgement of the counts. */
#define IOC_BLOCK_KEEP 0
#define IOC_BLOCK_SKIP 1
#define IOC_BLOCK_PART 2
#define IOC_BLOCK_NONE 3
#define IOC_ISO_DIRECT 0
#define IOC_ISO_ASSIGNED 1
#define IOC_ISO_RARE 2
#define IOC_ISO_AMBIGUOUS 3
#define IOC_BLOCKS_MAX 32
typedef struct {
    uint32_t depth, in_gap;       /* D(p) and in(p); rlen + 1 rows per segment, the last one zero */
} ioc_block_row;                  /* 8 bytes */
typedef struct {
    int32_t first, end;
    uint32_t n_keep, n_skip, n_part, n_none;  /* over the segment's reads */
    uint32_t reserved[2];
} ioc_pile_block;                 /* 32 bytes */
typedef struct {
    uint64_t key;
    int32_t group, how;
    int32_t first_row, end_row;   /* the first covered row and one past the last (0, 0: the read covers nothing) */
    int32_t n_gaps, gap_rows;     /* its long gaps and their rows */
} ioc_read_blocks;                /* 32 bytes */
typedef struct {
    int32_t n_blocks, n_found, n_groups, n_reads, n_direct, n_assigned, n_rare, n_ambiguous;
} ioc_blocks_seg;                 /* 32 bytes */
/* The definition: one segment, the planes read-major (n_reads x (rlen + 1) bytes), the plain loops above.  out_rows (may be NULL):
 * rlen + 1 rows; out_blocks: room for min(max_blocks, rlen) records, of which the first out_seg->n_blocks are written; out_reads:
 * n_reads records.  IOC_ERR_ARG, with nothing written, for a rule outside its ranges, a negative count or length and a NULL
 * pointer that is needed. */
int ioc_host_planes_blocks(const uint8_t* base, int32_t n_reads, int32_t rlen, int32_t min_gap, int32_t min_depth, int32_t min_alt,
                           int32_t min_pct, int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows, ioc_pile_block* out_blocks,
                           ioc_read_blocks* out_reads, ioc_blocks_seg* out_seg);
/* Many segments at once on the device, from host base planes, which are uploaded: the pairs' planes one behind the other as for
 * ioc_planes_polish, a segment's reads its pairs in ascending order.  The kernels of ioc_read_blocks.hip turn every plane into two
 * bit planes by ballot (covered, deleted) and work on those: run lengths carried across words, a lane per row for the table, a wave
 * per segment for the blocks, masked popcounts for the states, a wave per read for the isoforms; no atomics.  out_rows (may be NULL):
 * the segments' tables one behind the other, rlen[g] + 1 rows each; out_blocks: the kept blocks packed in segment order, segment
 * g's at block_off[g] .. block_off[g + 1] (n_segs + 1 entries); out_reads per pair, out_seg per segment; each as
 * ioc_host_planes_blocks defines it.  IOC_ERR_ARG, with nothing written, for what the definition refuses, seg_of_pair outside the
 * segments and a NULL pointer that is needed; IOC_ERR_CAPACITY, with nothing written, for blocks_cap below the sum over the segments
 * of min(max_blocks, rlen[g]). */
int ioc_planes_blocks(ioc_ctx* ctx, int32_t n_segs, const int32_t* rlen, int32_t n_pairs, const int32_t* seg_of_pair, const uint8_t* base,
                      int32_t min_gap, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t min_block, int32_t max_blocks,
                      ioc_block_row* out_rows, ioc_pile_block* out_blocks, int64_t blocks_cap, int64_t* block_off, ioc_read_blocks* out_reads,
                      ioc_blocks_seg* out_seg);
/* ioc_align_pairs_alleles' alignment — the table of counts, and k_ops_project into every pair's planes — and behind the walks the
 * block kernels over the planes where they lie: scores, windows, ratio, out_stats, the segments and out_cols (optional) as from
 * ioc_align_pairs_alleles, everything else as from ioc_planes_blocks.  Every pair is aligned, piled and projected exactly once.  The
 * stage's own memory is reserved after the walks.  The refusals of both calls; nothing is written. */
int ioc_align_pairs_blocks(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch,
                           int32_t gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats,
                           int32_t n_segs, const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth,
                           int32_t min_alt, int32_t min_pct, int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows,
                           ioc_pile_block* out_blocks, int64_t blocks_cap, int64_t* block_off, ioc_read_blocks* out_reads,
                           ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols);
/* ioc_align_pairs_blocks with the consensus of every isoform called where the planes lie: everything ioc_align_pairs_blocks returns
 * comes back unchanged, the pile projects the six slot planes of k_ops_project_ins beside the two (8 bytes per row and pair in all,
 * which count against the checkpoint arena's budget like the table), and behind the block kernels k_group_pile and the call kernels
 * run over the planes with the isoforms the block search just made.  Segment g's isoforms 0 .. min(n_groups, max_iso) - 1 are
 * called (max_iso >= 1), each from its direct and assigned reads as ioc_planes_polish_groups defines it at polish_min_depth, the
 * frame of segment g being its representative as the pairs were aligned against it; reads of a later isoform, rare reads and
 * ambiguous reads are in no table.  iso_off (n_segs + 1 entries) says which group-segments are segment g's: iso_off[g] ..
 * iso_off[g + 1]; out_off (room for iso_cap + 1 entries) and out_polish (may be NULL; iso_cap records) are indexed by group-segment.
 * How many isoforms there are is not known before the call: a segment has at most as many as reads, so iso_cap must be at least the
 * sum over g of min(max_iso, reads of g) and cap at least that sum weighted by the bound of segment g (ioc_pileup_call); there are
 * no table outputs for the same reason.  Every pair is aligned, piled and projected exactly once.  The group tables and the stage's
 * own memory are reserved after the walks.  The refusals of ioc_align_pairs_blocks; IOC_ERR_ARG for max_iso < 1, polish_min_depth <
 * 1, a negative cap or iso_cap, a NULL out_off or iso_off, NULL out_seq / out_qual where something may be written; IOC_ERR_CAPACITY
 * for iso_cap or cap below its bound and for a segment whose bound exceeds 2^31 - 1; nothing is written on any of them. */
int ioc_align_pairs_blocks_polish(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch,
                                  int32_t gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats,
                                  int32_t n_segs, const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth,
                                  int32_t min_alt, int32_t min_pct, int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows,
                                  ioc_pile_block* out_blocks, int64_t blocks_cap, int64_t* block_off, ioc_read_blocks* out_reads,
                                  ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols, int32_t max_iso, int32_t polish_min_depth,
                                  char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_polish,
                                  int64_t iso_cap, int64_t* iso_off);
/* ioc_align_pairs_blocks_polish with every isoform called by weight, under the qualities of ioc_align_set_pool_qual: the pile
 * projects the seven weight planes of k_ops_project_weights beside the eight (15 bytes per row and pair in all, which count
 * against the checkpoint arena's budget; a call of ioc_align_pairs_blocks_polish reserves what it always did), and behind the block
 * kernels k_group_pile_weighted and the weighted mode of the call kernels run: isoform h of segment g is called as
 * ioc_planes_polish_groups_weighted defines it.  Everything but the isoforms' sequences, qualities and polish records — scores,
 * statistics, blocks, rows, read and segment records, the table, iso_off — is what ioc_align_pairs_blocks_polish returns, byte for
 * byte; with all qualities equal, or all at or below '"' (34), the sequences are too.  Every pair is aligned, piled and projected
 * exactly once.  The refusals of ioc_align_pairs_blocks_polish, and IOC_ERR_ARG for a pool without qualities; nothing is written on
 * any of them. */
int ioc_align_pairs_blocks_polish_weighted(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match,
                                           int32_t mismatch, int32_t gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio,
                                           ioc_aln_stats* out_stats, int32_t n_segs, const ioc_polish_seg* segs, const int32_t* seg_of_pair,
                                           int32_t min_gap, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t min_block,
                                           int32_t max_blocks, ioc_block_row* out_rows, ioc_pile_block* out_blocks, int64_t blocks_cap,
                                           int64_t* block_off, ioc_read_blocks* out_reads, ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols,
                                           int32_t max_iso, int32_t polish_min_depth, char* out_seq, char* out_qual, int64_t cap,
                                           int64_t* out_off, ioc_polish_stats* out_polish, int64_t iso_cap, int64_t* iso_off);

/* ---- Insertion sites: the exons a cluster's reads carry and its representative lacks, and isoforms over blocks and sites ----
 * A block is a stretch of the representative that some reads skip; an exon the representative lacks is a long insertion, and the
 * slot planes hold six inserted bases a run.  The length plane keeps how many there were.
 *
 * The length plane of one read: ilen[0 .. rlen], r the reference bases consumed as in ioc_host_ops_project.  A maximal run of n 'I'
 * bytes in front of row r sets ilen[r] = min(n, 255); free-end 'i' bytes count for nothing; every other entry is 0.  (Two 'I' runs
 * are separated by a byte that consumes a reference base, so a row receives one run.)  IOC_ERR_ARG, with nothing written, for a
 * negative length, a NULL pointer that is needed, a byte outside "=XIDid" and a string that does not consume rlen reference bases. */
int ioc_host_ops_project_ilen(const char* ops, int64_t len, int32_t rlen, uint8_t* ilen);
/* One segment is a reference of rlen rows with n_reads reads, each read its base plane and its length plane, rlen + 1 bytes each.
 * Junction p lies in front of row p.  A rule {min_ins in 1 .. 255, slack in 0 .. 32, min_depth >= 1, min_alt >= 1, min_pct in 1 ..
 * 50, max_sites in 1 .. 32}.  All integers.
 *  1. Read i spans junction p, 1 <= p <= rlen - 1, iff its base plane covers rows p - 1 and p (a byte of 0 .. 5).  Junctions 0 and
 *     rlen are spanned by nobody.
 *  2. The windowed sum W_i(p): the sum of ilen_i[q] over q = max(p - slack, 0) .. min(p + slack, rlen), every q, spanned or not.
 *     (One 'I' run of min_ins bases is NOT the rule: at 8 % errors the aligner breaks a 40-base exon into runs of 19 + 14 a few
 *     rows apart, as a stray match cuts a long gap.)
 *  3. Near: N_i(p) = read i spans p and W_i(p) >= min_ins.
 *  4. The row table: S(p) the reads that span p, in(p) the sum of N_i(p); junction p is variable iff S(p) >= min_depth, in(p) >=
 *     need(S(p)) and S(p) - in(p) >= need(S(p)), need as in ioc_host_pileup_sites: the test of a block's rows.
 *  5. A site [first, end): a maximal run of variable junctions, of any length from 1 (the window widens a site to about 2 slack + 1
 *     junctions already).  In ascending order; the first max_sites are kept, n_found says how many there were.
 *  6. A read's state at a kept site: IOC_INS_NONE unless it spans every junction of the site, else IOC_INS_CARRY if N_i(p) holds
 *     for some p of the site, else IOC_INS_LACK.
 *  7. The site record: the three state counts, and len_min / len_max, the smallest and the largest over the carriers of each
 *     carrier's largest W_i(p) over the site's junctions (0 without carriers).
 *  8. key = the sum over the kept sites b of state(b) << (2 b); the mask has both bits of every site whose state is not NONE.
 *  9. The isoforms are step 6 of ioc_host_planes_blocks over PAIRS of words (pre_key, key): pre_key[i], pre_mask[i] per read and
 *     pre_full per segment are meant to be the block stage's key, its mask and the mask of a complete read of its blocks; with
 *     pre_key NULL all three are 0 and the stage stands on its own.  A read is complete iff its mask is that of all kept sites AND
 *     pre_mask[i] == pre_full.  A pair carried by at least min_alt complete reads is supported; the supported pairs are the
 *     isoforms 0 .. n_groups - 1 in ascending unsigned order, pre_key major, key minor.  Direct, rare, assigned and ambiguous as
 *     there: agreement is tested under both masks, and "a state that is not NONE" means that either mask is not 0.
 * 10. The read record: key, group, how (the COMBINED isoform), n_near the junctions with N_i, ins_bases the sum of ilen_i over the
 *     junctions the read spans.
 * What stays out: more than 32 sites, runs beyond 255 bases (they count as 255); alternative ends are a stage of their own
 * (ioc_host_reads_ends, below), which this one does not combine its isoforms with.  The sequence of an inserted
 * exon is the next section's.  20 bases and 8 junctions are choices made on simulated reads, not measured on real data. */
#define IOC_INS_LACK 0
#define IOC_INS_CARRY 1
#define IOC_INS_NONE 3
#define IOC_INSERTS_MAX 32
#define IOC_INS_SLACK_MAX 32
typedef struct {
    uint32_t span, in_ins;        /* S(p) and in(p); rlen + 1 rows per segment, rows 0 and rlen zero */
} ioc_insert_row;                 /* 8 bytes */
typedef struct {
    int32_t first, end;
    uint32_t n_carry, n_lack, n_none;  /* over the segment's reads */
    uint32_t len_min, len_max;
    uint32_t reserved;
} ioc_pile_insert;                /* 32 bytes */
typedef struct {
    uint64_t key;
    int32_t group, how;
    int32_t n_near, ins_bases;
    uint32_t reserved[2];
} ioc_read_inserts;               /* 32 bytes */
typedef struct {
    int32_t n_sites, n_found, n_groups, n_reads, n_direct, n_assigned, n_rare, n_ambiguous;
} ioc_inserts_seg;                /* 32 bytes */
/* The definition: one segment, both kinds of plane read-major (n_reads x (rlen + 1) bytes), the plain loops above.  out_rows (may
 * be NULL): rlen + 1 rows; out_sites: room for min(max_sites, max(rlen - 1, 0)) records, of which the first out_seg->n_sites are
 * written; out_reads: n_reads records.  pre_key and pre_mask: both or neither.  IOC_ERR_ARG, with nothing written, for a rule
 * outside its ranges, a negative count or length and a NULL pointer that is needed. */
int ioc_host_planes_inserts(const uint8_t* base, const uint8_t* ilen, int32_t n_reads, int32_t rlen, int32_t min_ins, int32_t slack,
                            int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_sites, const uint64_t* pre_key,
                            const uint64_t* pre_mask, uint64_t pre_full, ioc_insert_row* out_rows, ioc_pile_insert* out_sites,
                            ioc_read_inserts* out_reads, ioc_inserts_seg* out_seg);
/* Many segments at once on the device, from host planes laid out as for ioc_planes_blocks; pre_key / pre_mask per pair, pre_full per
 * segment, all three or none.  The kernels of ioc_read_inserts.hip turn every pair of planes into two bit planes (spans, near; the
 * windowed sum by a wave prefix sum) and work on those as the block kernels do; no atomics.  out_rows (may be NULL), out_sites packed
 * with site_off (n_segs + 1 entries), out_reads per pair, out_seg per segment, each as ioc_host_planes_inserts defines it.
 * IOC_ERR_ARG, with nothing written, for what the definition refuses, seg_of_pair outside the segments and a NULL pointer that is
 * needed; IOC_ERR_CAPACITY, with nothing written, for sites_cap below the sum over the segments of min(max_sites, max(rlen[g] - 1, 0)). */
int ioc_planes_inserts(ioc_ctx* ctx, int32_t n_segs, const int32_t* rlen, int32_t n_pairs, const int32_t* seg_of_pair, const uint8_t* base,
                       const uint8_t* ilen, int32_t min_ins, int32_t slack, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                       int32_t max_sites, const uint64_t* pre_key, const uint64_t* pre_mask, const uint64_t* pre_full,
                       ioc_insert_row* out_rows, ioc_pile_insert* out_sites, int64_t sites_cap, int64_t* site_off,
                       ioc_read_inserts* out_reads, ioc_inserts_seg* out_seg);
/* ioc_align_pairs_blocks with the length plane projected beside the base plane (k_ops_project_ilen: 3 bytes per row and pair in
 * all, which count against the checkpoint arena's budget; a call of ioc_align_pairs_blocks reserves what it always did) and, behind
 * the block kernels, the insert kernels with the block stage's keys and masks as pre_*, where they lie on the device.  Everything
 * ioc_align_pairs_blocks returns comes back unchanged, byte for byte; added are the rows (may be NULL), sites, site_off, read and
 * segment records of ioc_planes_inserts, group / how of the read records being the combined isoform.  The block search and the
 * site search share min_depth, min_alt and min_pct.  Every pair is aligned, piled and projected exactly once; the stage's memory is
 * reserved after the walks.  The refusals of both calls; nothing is written. */
int ioc_align_pairs_blocks_inserts(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch,
                                   int32_t gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats,
                                   int32_t n_segs, const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth,
                                   int32_t min_alt, int32_t min_pct, int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows,
                                   ioc_pile_block* out_blocks, int64_t blocks_cap, int64_t* block_off, ioc_read_blocks* out_reads,
                                   ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols, int32_t min_ins, int32_t slack, int32_t max_sites,
                                   ioc_insert_row* out_irows, ioc_pile_insert* out_sites, int64_t sites_cap, int64_t* site_off,
                                   ioc_read_inserts* out_ireads, ioc_inserts_seg* out_iseg);

/* ---- The sequence of an inserted exon: the consensus of the carriers' windows at every kept insertion site ----
 * The insert stage says who carries an exon the representative lacks; the slot planes keep six of its bases.  What the carriers
 * hold between two anchor rows of the representative is cut out of the reads themselves, aligned to one of them and called with
 * the call that exists.  Nothing is aligned against the representative again.
 *
 * The position plane of one read: qpos[0 .. rlen], 32-bit.  qpos[0] = 0; for r >= 1, qpos[r] is the number of bytes of "=XIi"
 * among all bytes up to and including the byte that consumes reference row r - 1.  The run of 'I' in front of row r therefore
 * begins at query[qpos[r]].  What ioc_host_ops_project_ilen refuses: IOC_ERR_ARG, with nothing written. */
int ioc_host_ops_project_qpos(const char* ops, int64_t len, int32_t rlen, uint32_t* qpos);
/* A global alignment of two short strings, both ends anchored, linear gaps (both strings hold the same exon between the same
 * anchors: a gap costs `gap` >= 0 a base, and affine gaps are left out).  H[0][j] = -j gap, H[i][0] = -i gap, H[i][j] = max(H[i-1]
 * [j-1] + (query[i-1] == ref[j-1] ? match : mismatch), H[i][j-1] - gap, H[i-1][j] - gap), plain integers.  The walk goes back from
 * (qlen, rlen) and takes the diagonal where it gives H, else 'D' (H[i][j-1] - gap: a reference base alone) where that does, else
 * 'I'; on row 0 'D', on column 0 'I'.  The bytes "=XID" in forward order in ops (qlen + rlen at most), their number returned; the
 * tie order is part of the definition, k_win_align returns the same alignment.  *out_score (may be NULL): H[qlen][rlen].
 * IOC_ERR_ARG for a negative length or gap, |match|, |mismatch| or gap above 2^20 and a NULL pointer that is needed;
 * IOC_ERR_CAPACITY for cap < qlen + rlen and for (qlen + 1)(rlen + 1) above 2^26. */
int64_t ioc_host_align_global_ops(const char* query, int32_t qlen, const char* ref, int32_t rlen, int32_t match, int32_t mismatch, int32_t gap,
                                  char* ops, int64_t cap, int32_t* out_score);
/* A read's window at a kept site [first, end) of a segment of rlen rows, all integers, `slack` the insert stage's:
 *   lo = max(first - slack, 1), hi = min(end + slack, rlen); the window rows are [lo, hi); read i's window is
 *   query_i[qpos_i[lo], qpos_i[hi]): the insertions at junctions lo .. hi - 1 and the read's bases on rows lo .. hi - 1.
 * Read i VOTES iff its state at the site is IOC_INS_CARRY, its base plane covers rows lo - 1 and hi - 1 (a byte of 0 .. 5) and its
 * window length is in 1 .. max_win, max_win in 1 .. IOC_WIN_MAX.  A carrier that fails coverage counts as n_short; one that covers
 * and fails the length test as n_long, and so does one whose window leaves its read (qpos[hi] < qpos[lo] or qpos[hi] > qlen_i: a
 * plane that is not this read's).  The TEMPLATE is the voter at index (n - 1) / 2 of the voters sorted ascending by (window
 * length, index): the lower median.  A site without a voter is not called: tlen = 0, template_pair = -1.
 * All carriers of a site vote together here, whichever isoform they are in: two different exons at one junction are told apart by
 * the section after this one (ioc_host_insert_window_variants), not by these calls.
 * The consensus of a site: every voter's window is aligned to the template's (ioc_host_align_global_ops, the template the
 * reference; the template to itself is all '='), its bytes projected (ioc_host_ops_project, ioc_host_ops_project_ins) and piled
 * (ioc_host_planes_pile); the site is ioc_host_pileup_call(those tables, the template's window, polish_min_depth).  The sequence
 * stands in the orientation the pairs were aligned in: the reverse complement's frame where the segment's ref_revcomp is set.
 * lo and hi come back: the consensus stands for the representative's rows [lo, hi). */
#define IOC_WIN_MAX 512
#define IOC_WIN_NONE 0   /* a read's class at a site: no carrier; a voter; a carrier that does not cover; one whose window is too long */
#define IOC_WIN_VOTER 1
#define IOC_WIN_SHORT 2
#define IOC_WIN_LONG 3
typedef struct {
    int32_t lo, hi;
    int32_t template_pair;        /* the pair (ioc_host_insert_windows: the read) whose window is the template, -1 without */
    int32_t tlen;                 /* its window's length, 0: the site is not called */
    uint32_t n_voters, n_short, n_long;
    uint32_t reserved;
} ioc_insert_window;              /* 32 bytes */
/* The definition of the windows of one segment: base planes and position planes read-major (n_reads x (rlen + 1) bytes / words),
 * qlen per read, the kept sites (first and end are read) and every read's key (ioc_read_inserts.key).  out_win: n_sites records;
 * out_class (may be NULL): a byte per read and site, read-major, IOC_WIN_*; out_start / out_len (may be NULL, both or neither): where
 * a VOTER's window begins in its read and how long it is, 0 elsewhere.  IOC_ERR_ARG, with nothing written, for slack outside 0 ..
 * 32, max_win outside 1 .. IOC_WIN_MAX, n_sites outside 0 .. 32, a site outside 1 <= first < end <= rlen, a negative count and a NULL
 * pointer that is needed. */
int ioc_host_insert_windows(const uint8_t* base, const uint32_t* qpos, const int32_t* qlen, int32_t n_reads, int32_t rlen,
                            const ioc_pile_insert* sites, int32_t n_sites, const uint64_t* keys, int32_t slack, int32_t max_win,
                            ioc_insert_window* out_win, uint8_t* out_class, uint32_t* out_start, uint32_t* out_len);
/* Many segments at once on the device, over the pool that is set (ioc_align_set_pool): pair i's read is pool sequence query[i], its
 * planes lie as for ioc_planes_inserts (base: bytes, qpos: 32-bit words, reference length + 1 each, the pairs one behind the other),
 * sites packed with site_off (n_segs + 1 entries) and keys per pair as ioc_planes_inserts returned them.  The kernels of
 * ioc_insert_windows.hip: k_win_bounds (a wave per pair, a lane per site), k_win_template (a wave per site: the lower median by
 * counting smaller (length, pair) over the members), k_win_align (a wave per voter and site: the recurrence above with a lane per
 * template column, two direction bits a cell, and the walk back, which writes the voter's base plane and slot planes in the
 * template's frame), then k_group_pile with a group per site and k_pile_call, both unchanged.  No atomics.
 * Outputs, per site in site order (n = site_off[n_segs]): out_win (template_pair: the pair of the call); out_seq / out_qual packed
 * with out_off (n + 1 entries); out_stats; out_cols / out_ins (may be NULL, both or neither): the sites' tables, site x from the
 * sum over the earlier sites of (tlen + 1) on, room for n (max_win + 1) rows.  IOC_ERR_ARG, with nothing written, for what the
 * definitions refuse, polish_min_depth < 1, a query outside the pool, seg_of_pair outside the segments, site_off that does not
 * ascend from 0 and a NULL pointer that is needed; IOC_ERR_CAPACITY, with nothing written, for cap below n (7 max_win + 6). */
int ioc_planes_insert_windows(ioc_ctx* ctx, int32_t n_segs, const int32_t* rlen, int32_t n_pairs, const int32_t* seg_of_pair, const int32_t* query,
                              const uint8_t* base, const uint32_t* qpos, const ioc_pile_insert* sites, const int64_t* site_off, const uint64_t* keys,
                              int32_t slack, int32_t max_win, int32_t match, int32_t mismatch, int32_t gap, int32_t polish_min_depth,
                              ioc_insert_window* out_win, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_stats,
                              ioc_pileup_col* out_cols, ioc_pileup_ins* out_ins);
/* ioc_align_pairs_blocks_inserts with the position plane projected beside the other two (k_ops_project_qpos: four more bytes per
 * row and pair, which count against the checkpoint arena's budget; the calls that exist reserve what they always did) and, behind
 * the insert kernels, the window kernels over the planes where they lie.  Everything ioc_align_pairs_blocks_inserts returns comes
 * back unchanged, byte for byte; added are the outputs of ioc_planes_insert_windows over the sites kept, with win_match /
 * win_mismatch / win_gap as its scoring triple.  win_cap must hold (sum over the segments of min(max_sites, max(rlen - 1, 0))) x
 * (7 max_win + 6), which is known before the call.  Every pair is aligned once.  The refusals of both calls; nothing is written. */
int ioc_align_pairs_blocks_inserts_seq(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch,
                                       int32_t gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats,
                                       int32_t n_segs, const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth,
                                       int32_t min_alt, int32_t min_pct, int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows,
                                       ioc_pile_block* out_blocks, int64_t blocks_cap, int64_t* block_off, ioc_read_blocks* out_reads,
                                       ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols, int32_t min_ins, int32_t slack, int32_t max_sites,
                                       ioc_insert_row* out_irows, ioc_pile_insert* out_sites, int64_t sites_cap, int64_t* site_off,
                                       ioc_read_inserts* out_ireads, ioc_inserts_seg* out_iseg, int32_t max_win, int32_t win_match,
                                       int32_t win_mismatch, int32_t win_gap, int32_t polish_min_depth, ioc_insert_window* out_win, char* out_wseq,
                                       char* out_wqual, int64_t win_cap, int64_t* out_woff, ioc_polish_stats* out_wstats);

/* ---- Two exons at one junction: the variants of an insertion site ----
 * The window stage lets all carriers of a site vote together.  Where they carry two different exons (mutually exclusive exons), the
 * voters are split in two here, each variant gets a consensus of its own, every read a second key and the isoforms are counted again.
 * The rule: the window rule {slack, max_win, match, mismatch, gap}, min_agree in 1 .. 100, and min_alt >= 1 and min_pct in 1 .. 50,
 * the insert stage's.  All integers.  Per kept site:
 *  1. The AGREEMENT of an alignment is #'=' - #'X' - #'D' - #'I' over its bytes (ioc_host_ops_agreement).  A voter of qlen bases is
 *     NEAR a template of tlen bases iff its agreement a from ioc_host_align_global_ops(voter, template) has a >= 1 and 100 a >=
 *     min_agree max(qlen, tlen).  A template is NEAR itself, a = tlen.
 *  2. Round A: the classes, the template and lo / hi are ioc_host_insert_windows' and come back unchanged.  Every voter is tested
 *     against template A; n_far voters are not NEAR.
 *  3. Round B runs iff n_far >= need and n_voters - n_far >= need, need = need(n_voters) as in ioc_host_pileup_sites with this
 *     rule's min_alt and min_pct.  Template B is the lower median of the FAR voters by (window length, index); every far voter is
 *     tested against it: n_b of them are NEAR it, n_other are not.
 *  4. The site SPLITS iff round B ran and n_b >= need.  At a split site the near voters are variant A, the far voters near
 *     template B variant B, the rest OTHER: they vote nowhere.  At a site that does not split every voter is variant A, the far
 *     ones included, and the site's consensus is ioc_planes_insert_windows', byte for byte.  (Where round B did not run, n_b and
 *     n_other are 0 and template_pair_b is -1; where it ran and the site does not split, they say what it found.)
 *  5. The consensus of a variant: the window stage's chain over its voters and its template (project, pile, ioc_host_pileup_call
 *     with the template's window as the frame).  A site has two slots, 2 x for A and 2 x + 1 for B; slot B is empty where the site
 *     does not split.
 *  6. key2 is the read's insert key with its state changed at every SPLIT site: a variant-B voter gets IOC_INS_CARRY_B, an OTHER
 *     voter IOC_INS_NONE, a carrier that is no voter (IOC_WIN_SHORT, IOC_WIN_LONG) IOC_INS_NONE — nobody knows which exon it holds
 *     —, everything else stays.  mask2 has both bits of every site whose state is not NONE.
 *  7. The isoforms again: step 9 of ioc_host_planes_inserts over (pre_key, key2), (pre_mask, mask2) and pre_full
 *     (ioc_host_key_isoforms, which that definition calls as well).
 * min_agree 45 is a choice made on simulated windows, not measured on real data: 8 + exon + 9 bases, scoring 2 / -2 / 2, 8 % errors
 * in voter and template, 60 trials a shape.  The lowest 100 a / max between two copies of one exon against the highest between two
 * different exons: 57 / 33 at 60 and 60 bases, 59 / 31 at 60 and 45, 61 / 22 at 120 and 100.  At 30 bases and below the ranges
 * overlap (49 / 42), at 15 % errors they touch (35 / 31): exons under about 40 bases and reads beyond about 10 % errors are outside
 * what the default separates.
 * What stays out: more than two variants, a quality-weighted variant call and re-clustering.  ioc_host_isoform_splice reads state 2
 * as "does not carry"; the splice that takes each variant's own slot is ioc_host_isoform_splice_variants, further down.  State 2
 * appears in the outputs of the calls of this section alone. */
#define IOC_INS_CARRY_B 2
#define IOC_WINVAR_NONE 0    /* a read's variant at a site: no voter; variant A; variant B; a voter near neither template */
#define IOC_WINVAR_A 1
#define IOC_WINVAR_B 2
#define IOC_WINVAR_OTHER 3
#define IOC_WINVAR_MIN_AGREE 45
typedef struct {
    int32_t split;                /* 1: the site splits */
    int32_t template_pair_b;      /* the pair (ioc_host_insert_window_variants: the read) whose window is template B, -1 without */
    int32_t tlen_b;
    uint32_t n_a, n_b, n_other;   /* n_a: the voters of variant A (all of them where the site does not split) */
    uint32_t n_far;
    uint32_t reserved;
} ioc_window_variant;             /* 32 bytes */
typedef struct {
    uint64_t key2;
    int32_t group, how;
} ioc_read_variants;              /* 16 bytes */
typedef struct {
    int32_t n_sites, n_split, n_groups, n_reads, n_direct, n_assigned, n_rare, n_ambiguous;
} ioc_variants_seg;               /* 32 bytes */
/* *out = #'=' - #'X' - #'D' - #'I' over the bytes; 'i' and 'd' count for nothing.  IOC_ERR_ARG, with nothing written, for a negative
 * length, a NULL pointer that is needed and a byte outside "=XIDid". */
int ioc_host_ops_agreement(const char* ops, int64_t len, int32_t* out);
/* The isoforms of n_reads reads from two-word keys: read i is complete iff mask[i] == full and pre_mask[i] == pre_full; a pair
 * (pre_key, key) carried by at least min_alt complete reads is supported, the supported pairs are the groups 0 .. n - 1 in
 * ascending unsigned order, pre_key major; direct, rare, assigned and ambiguous as step 9 of ioc_host_planes_inserts has them.
 * pre_key and pre_mask: both or neither (then all three are 0).  out_group / out_how per read; out_counts: n_groups, n_direct,
 * n_assigned, n_rare, n_ambiguous.  IOC_ERR_ARG, with nothing written, for a negative count, min_alt < 1 and a NULL pointer that is
 * needed. */
int ioc_host_key_isoforms(const uint64_t* pre_key, const uint64_t* pre_mask, uint64_t pre_full, const uint64_t* key, const uint64_t* mask,
                          uint64_t full, int32_t n_reads, int32_t min_alt, int32_t* out_group, int32_t* out_how, int32_t* out_counts);
/* The definition, one segment: ioc_host_insert_windows' inputs, the reads' bytes (read i is reads[read_off[i] .. read_off[i + 1]),
 * which must be qlen[i] long), the scoring triple and the rule.  out_win: n_sites records; out_var: n_sites records; out_variant: a
 * byte per read and site, read-major, IOC_WINVAR_*; out_agree (may be NULL): two words per read and site, [(i n_sites + k) 2 + round],
 * INT32_MIN where the round did not align the read; out_seq / out_qual (may be NULL, both or neither, and then out_off and
 * out_stats are not written): the 2 n_sites slots packed with out_off (2 n_sites + 1 entries), out_stats a record per slot, cap what
 * seq and qual hold each; out_key2 / out_mask2 per read.  IOC_ERR_ARG, with nothing written, for what ioc_host_insert_windows
 * refuses, a scoring triple ioc_host_align_global_ops refuses, min_agree outside 1 .. 100, min_alt < 1, min_pct outside 1 .. 50,
 * polish_min_depth < 1, read_off that does not fit qlen and a NULL pointer that is needed; IOC_ERR_CAPACITY, with nothing written,
 * for cap below 2 n_sites (7 max_win + 6). */
int ioc_host_insert_window_variants(const uint8_t* base, const uint32_t* qpos, const int32_t* qlen, int32_t n_reads, int32_t rlen,
                                    const ioc_pile_insert* sites, int32_t n_sites, const uint64_t* keys, const char* reads,
                                    const int64_t* read_off, int32_t slack, int32_t max_win, int32_t match, int32_t mismatch, int32_t gap,
                                    int32_t polish_min_depth, int32_t min_agree, int32_t min_alt, int32_t min_pct,
                                    ioc_insert_window* out_win, ioc_window_variant* out_var, uint8_t* out_variant, int32_t* out_agree,
                                    char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_stats,
                                    uint64_t* out_key2, uint64_t* out_mask2);
/* Many segments at once on the device: ioc_planes_insert_windows' arguments, the rule, and pre_key / pre_mask per pair with pre_full
 * per segment (all three or none), the block stage's.  The kernels of ioc_window_variants.hip behind those of the window stage:
 * k_win_agree (a wave per alignment: the agreement from the voter's base plane in the template's frame as k_win_align left it,
 * nothing is aligned or walked again), k_win_template_far (template B: k_win_template's ranking over the far voters), k_win_align
 * again for round B, k_win_decide (a wave per site), k_win_rekey (a wave per pair) and the isoform count of ioc_read_stage.h over
 * key2 / mask2; then k_group_pile with a group per (site, variant) and k_pile_call.  No atomics.
 * Outputs, n = site_off[n_segs]: out_win and out_var per site; out_seq / out_qual packed with out_off (2 n + 1 entries: slot 2 x is
 * site x's variant A, 2 x + 1 its B) and out_stats per slot; out_variant: IOC_INSERTS_MAX bytes per pair, byte k the pair's variant
 * at site k of its segment (0 behind the segment's sites); out_agree (may be NULL): 2 IOC_INSERTS_MAX words per pair, [2 k + round];
 * out_reads per pair (key2 and the isoform counted again) and out_seg per segment.  The refusals of ioc_planes_insert_windows and of
 * the definition; IOC_ERR_CAPACITY, with nothing written, for cap below 2 n (7 max_win + 6).
 * RESTRICTION: the pool's sequences are taken to hold A C G T and N alone (upper case).  k_win_agree compares channels (A C G T
 * other), the definition compares bytes: two DIFFERENT bytes outside A C G T in one column of an alignment — 'R' against 'N', 'a'
 * against 'c' — count as '=' on the device and as 'X' in the definition, so the device's agreement of such a pair is too high by two
 * a column and a site may fail to split.  Nothing checks this (ioc_align_set_pool takes any bytes): a caller with IUPAC codes or
 * lower case maps them to N first.  It holds for ioc_align_pairs_blocks_inserts_variants as well. */
int ioc_planes_insert_window_variants(ioc_ctx* ctx, int32_t n_segs, const int32_t* rlen, int32_t n_pairs, const int32_t* seg_of_pair,
                                      const int32_t* query, const uint8_t* base, const uint32_t* qpos, const ioc_pile_insert* sites,
                                      const int64_t* site_off, const uint64_t* keys, int32_t slack, int32_t max_win, int32_t match,
                                      int32_t mismatch, int32_t gap, int32_t polish_min_depth, int32_t min_agree, int32_t min_alt,
                                      int32_t min_pct, const uint64_t* pre_key, const uint64_t* pre_mask, const uint64_t* pre_full,
                                      ioc_insert_window* out_win, ioc_window_variant* out_var, char* out_seq, char* out_qual, int64_t cap,
                                      int64_t* out_off, ioc_polish_stats* out_stats, uint8_t* out_variant, int32_t* out_agree,
                                      ioc_read_variants* out_reads, ioc_variants_seg* out_seg);

/* ioc_align_pairs_blocks_inserts_seq with the variant kernels behind the window kernels, over the planes where they lie.  Everything
 * ioc_align_pairs_blocks_inserts_seq returns comes back unchanged, byte for byte — the window call's own consensus of a site, all
 * voters voting, is one more group of the pile over round A's planes —; added are the outputs of ioc_planes_insert_window_variants
 * over the sites kept, the block stage's keys, masks and full masks serving as pre_* and min_alt / min_pct being the searches'.
 * var_cap must hold twice what win_cap must.  Every pair is aligned once, every voter once a round.  The refusals of both calls;
 * nothing is written. */
int ioc_align_pairs_blocks_inserts_variants(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch,
                                            int32_t gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats,
                                            int32_t n_segs, const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth,
                                            int32_t min_alt, int32_t min_pct, int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows,
                                            ioc_pile_block* out_blocks, int64_t blocks_cap, int64_t* block_off, ioc_read_blocks* out_reads,
                                            ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols, int32_t min_ins, int32_t slack, int32_t max_sites,
                                            ioc_insert_row* out_irows, ioc_pile_insert* out_sites, int64_t sites_cap, int64_t* site_off,
                                            ioc_read_inserts* out_ireads, ioc_inserts_seg* out_iseg, int32_t max_win, int32_t win_match,
                                            int32_t win_mismatch, int32_t win_gap, int32_t polish_min_depth, ioc_insert_window* out_win, char* out_wseq,
                                            char* out_wqual, int64_t win_cap, int64_t* out_woff, ioc_polish_stats* out_wstats, int32_t min_agree,
                                            ioc_window_variant* out_var, char* out_vseq, char* out_vqual, int64_t var_cap, int64_t* out_voff,
                                            ioc_polish_stats* out_vstats, uint8_t* out_variant, int32_t* out_agree, ioc_read_variants* out_vreads,
                                            ioc_variants_seg* out_vseg);

/* ---- The full-length sequence of a combined isoform: the windows of the exons it carries spliced into its consensus ----
 * ioc_host_pileup_call calls an isoform in the representative's frame, where an exon the representative lacks is six slot bases at
 * most; the window stage returns that exon's consensus beside the anchor rows lo and hi it stands between.  The splice puts the two
 * together, for ONE isoform of one segment:
 *   cols / ins, frame, rlen, min_depth: the isoform's tables (ioc_host_planes_pile of its reads) and what ioc_host_pileup_call takes;
 *   key: the insert key of its direct reads (ioc_read_inserts.key), state at site b = (key >> 2 b) & 3;
 *   win: the records of the segment's n_sites kept sites (lo, hi and tlen are read), n_sites in 0 .. IOC_INSERTS_MAX;
 *   win_seq / win_qual / win_off: the sites' called windows, site b's bytes at win_off[b] .. win_off[b + 1] (n_sites + 1 entries).
 *  1. The sites in ascending order.  Site b is IOC_SPLICE_LACK where the key's state at b is not IOC_INS_CARRY; else
 *     IOC_SPLICE_UNCALLED where tlen == 0; else IOC_SPLICE_OVERLAP where lo is below the hi of the last DONE site of this isoform
 *     (the windows of sites closer than 2 slack overlap; the earlier one wins); else IOC_SPLICE_DONE.
 *  2. The output is ioc_host_pileup_call's walk over p = 0 .. rlen, except that for every DONE site the insertions in front of rows
 *     lo .. hi - 1 and the bases of rows lo .. hi - 1 are neither emitted nor counted in the record, and in their place, at row lo,
 *     stand the window's sequence and qualities as they are: the window is "the insertions at junctions lo .. hi - 1 and the read's
 *     bases on rows lo .. hi - 1".  The insertions in front of row hi come from the tables as always.
 *  3. An isoform with no DONE site is ioc_host_pileup_call byte for byte, record included.
 * st (may be NULL): n_sub, n_del, n_ins and n_low over the rows that were called, out_len everything written, windows included.
 * out_sites (n_sites records): the state, and for a DONE site where its window's bytes begin in the isoform's sequence and how many
 * they are, -1 and 0 otherwise.  out_sstats (may be NULL): rows_replaced is the sum of hi - lo and spliced_bytes of len over the DONE
 * sites.  Returns the length written.  IOC_ERR_ARG for what ioc_host_pileup_call refuses, n_sites outside 0 .. IOC_INSERTS_MAX, a
 * record outside 1 <= lo < hi <= rlen or with tlen < 0, a win_off that does not ascend and a NULL pointer that is needed;
 * IOC_ERR_CAPACITY for cap below rlen + IOC_PILE_INS_SLOTS * (rlen + 1) + win_off[n_sites] - win_off[0]; nothing is written on any. */
#define IOC_SPLICE_LACK 0
#define IOC_SPLICE_DONE 1
#define IOC_SPLICE_UNCALLED 2
#define IOC_SPLICE_OVERLAP 3
typedef struct {
    int32_t state;                /* IOC_SPLICE_* */
    int32_t at, len;              /* DONE: the window's first byte in the isoform's sequence and its length; else -1 and 0 */
    int32_t reserved;
} ioc_splice_site;                /* 16 bytes */
typedef struct {
    int32_t n_done, n_uncalled, n_overlap;
    int32_t rows_replaced, spliced_bytes;
    int32_t reserved[3];
} ioc_splice_stats;               /* 32 bytes */
int64_t ioc_host_isoform_splice(const ioc_pileup_col* cols, const ioc_pileup_ins* ins, const char* frame, int32_t rlen, int32_t min_depth,
                                uint64_t key, const ioc_insert_window* win, int32_t n_sites, const char* win_seq, const char* win_qual,
                                const int64_t* win_off, char* out_seq, char* out_qual, int64_t cap, ioc_polish_stats* st,
                                ioc_splice_site* out_sites, ioc_splice_stats* out_sstats);
/* Every isoform of many segments at once on the device, from host planes laid out as for ioc_planes_polish_groups (rlen, frames,
 * frame_off, n_groups, seg_of_pair, group, base, slots as there; G group-segments in segment order).  iso_key: a key per
 * group-segment; win: the segments' window records packed with site_off (n_segs + 1 entries, at most IOC_INSERTS_MAX a segment);
 * win_seq / win_qual packed with win_off (site_off[n_segs] + 1 entries), all as ioc_planes_insert_windows returns them.
 * Group-segment (g, h) is ioc_host_isoform_splice over the tables ioc_host_planes_pile makes of its pairs, iso_key of (g, h) and
 * the sites of g.  k_group_pile adds the planes up; then the kernels of ioc_iso_splice.hip: k_splice_plan (a wave per
 * group-segment, a lane per site: the states, the site records and a list of at most 32 intervals), k_splice_call in a count
 * pass, the scan of the call kernels, and k_splice_call in a write pass (a workgroup per group-segment, a lane per row; a window's
 * bytes are copied by the whole workgroup).  No atomics: every byte has one writer and its place is a function of the tables and
 * the plan.  out_seq / out_qual packed with out_off (G + 1 entries); out_polish and out_sstats (may be NULL) G records each;
 * out_splice packed with splice_off (G + 1 entries): group-segment (g, h) has a record per kept site of g; out_gcols / out_gins
 * (optional) the group tables as from ioc_planes_polish_groups.  IOC_ERR_ARG, with nothing written, for what
 * ioc_planes_polish_groups and the definition refuse, site_off or win_off that does not ascend from 0, a segment with more than
 * IOC_INSERTS_MAX sites and a NULL pointer that is needed; IOC_ERR_CAPACITY, with nothing written, for cap below the sum over g of
 * n_groups[g] * (the call's bound of segment g + the bytes of g's windows), for a group-segment whose bound exceeds 2^31 - 1 and for
 * splice_cap below the sum over g of n_groups[g] * the sites of g. */
int ioc_planes_isoforms_full(ioc_ctx* ctx, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off,
                             const int32_t* n_groups, int32_t n_pairs, const int32_t* seg_of_pair, const int32_t* group, const uint8_t* base,
                             const uint8_t* slots, const uint64_t* iso_key, const ioc_insert_window* win, const int64_t* site_off,
                             const char* win_seq, const char* win_qual, const int64_t* win_off, int32_t min_depth, char* out_seq,
                             char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_polish, ioc_splice_stats* out_sstats,
                             ioc_splice_site* out_splice, int64_t splice_cap, int64_t* splice_off, ioc_pileup_col* out_gcols,
                             ioc_pileup_ins* out_gins);
/* ioc_align_pairs_blocks_inserts_seq with the six slot planes projected beside base, length and position (13 bytes per row and pair,
 * which count against the checkpoint arena's budget; the calls that exist reserve what they always did), behind the window kernels
 * k_group_pile over the COMBINED isoforms (ioc_read_inserts.group: the first min(n_groups, max_iso) of a segment, each from its
 * direct and assigned reads as ioc_align_pairs_blocks_polish takes them), and then the splice kernels: isoform h of segment g is
 * ioc_host_isoform_splice over its tables, the key of its lowest-numbered direct read (all direct reads of a group carry the same
 * key) and the windows of g the same call just made, the frame being g's representative as the pairs were aligned against it.
 * polish_min_depth serves the windows and the isoforms.  Everything ioc_align_pairs_blocks_inserts_seq returns comes back byte for
 * byte; added are iso_off (n_segs + 1 entries: segment g's group-segments are iso_off[g] .. iso_off[g + 1]) and, indexed by
 * group-segment, out_seq / out_qual with out_off, out_polish, out_sstats (either may be NULL) and out_splice with splice_off, as
 * ioc_planes_isoforms_full returns them.  The room is known before the call: iso_cap at least the sum over g of k_g = min(max_iso,
 * reads of g) — out_off and splice_off hold iso_cap + 1 entries —, splice_cap the sum of k_g * s_g with s_g = min(max_sites,
 * max(rlen_g - 1, 0)), and cap the sum of k_g * (the call's bound of rlen_g + s_g * (7 max_win + 6)).  That is 3590 bytes a site at
 * max_win 512 and 32 sites a segment where nothing is known; a caller who knows its data keeps it small with max_sites (a cluster
 * seldom has more than a few insertion sites), with max_win (the longest exon expected plus 2 slack + 1 rows) and with batches of
 * segments.  Every pair is aligned, piled and projected exactly once.  The refusals of ioc_align_pairs_blocks_inserts_seq;
 * IOC_ERR_ARG for max_iso < 1, a negative cap, splice_cap or iso_cap and a NULL pointer that is needed; IOC_ERR_CAPACITY for iso_cap,
 * splice_cap or cap below its bound and for an isoform whose bound exceeds 2^31 - 1; nothing is written on any of them. */
int ioc_align_pairs_isoforms_full(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch,
                                  int32_t gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats,
                                  int32_t n_segs, const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth,
                                  int32_t min_alt, int32_t min_pct, int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows,
                                  ioc_pile_block* out_blocks, int64_t blocks_cap, int64_t* block_off, ioc_read_blocks* out_reads,
                                  ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols, int32_t min_ins, int32_t slack, int32_t max_sites,
                                  ioc_insert_row* out_irows, ioc_pile_insert* out_sites, int64_t sites_cap, int64_t* site_off,
                                  ioc_read_inserts* out_ireads, ioc_inserts_seg* out_iseg, int32_t max_win, int32_t win_match,
                                  int32_t win_mismatch, int32_t win_gap, int32_t polish_min_depth, ioc_insert_window* out_win, char* out_wseq,
                                  char* out_wqual, int64_t win_cap, int64_t* out_woff, ioc_polish_stats* out_wstats, int32_t max_iso,
                                  char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_polish,
                                  ioc_splice_stats* out_sstats, ioc_splice_site* out_splice, int64_t splice_cap, int64_t* splice_off,
                                  int64_t iso_cap, int64_t* iso_off);

/* ---- The full-length sequence by variant: every exon's own window spliced in ----
 * ioc_host_isoform_splice over the variant stage's outputs.  Its inputs are that function's, except that
 *   key is a read's key2 (ioc_read_variants.key2);
 *   var holds the segment's ioc_window_variant records beside win (split and tlen_b are read);
 *   slot_seq / slot_qual / slot_off are the variant stage's slots in place of one window a site: 2 n_sites + 1 entries, slot 2 b
 *   is site b's variant A and 2 b + 1 its B.
 * Rule 1 becomes, for site b in ascending order with state s = (key >> 2 b) & 3: s == IOC_INS_CARRY takes slot 2 b and the template
 * length win[b].tlen; s == IOC_INS_CARRY_B takes slot 2 b + 1 and the template length var[b].split ? var[b].tlen_b : 0 (a key that
 * claims B where nothing split makes the site UNCALLED, not an error); any other state is IOC_SPLICE_LACK.  Then as before:
 * UNCALLED where that template length is 0, OVERLAP where lo lies below the hi of the last DONE site (lo and hi are the site's, the
 * same for both variants), otherwise DONE.  Rules 2 and 3, the records, the statistics and the capacity rule are
 * ioc_host_isoform_splice's with "the window" read as "the slot's bytes"; which variant a DONE site took is the key's state there.
 * Put differently: the result is ioc_host_isoform_splice over the key with every 2 turned into 1, win with tlen replaced as above
 * and the chosen slot of every site as that site's window.  IOC_ERR_ARG for what ioc_host_isoform_splice refuses, a NULL var with
 * n_sites > 0, a slot_off that does not ascend, a var[b].split outside 0 / 1 and a negative tlen_b; IOC_ERR_CAPACITY for cap below
 * rlen + IOC_PILE_INS_SLOTS * (rlen + 1) + slot_off[2 n_sites] - slot_off[0]; nothing is written on any. */
int64_t ioc_host_isoform_splice_variants(const ioc_pileup_col* cols, const ioc_pileup_ins* ins, const char* frame, int32_t rlen, int32_t min_depth,
                                         uint64_t key, const ioc_insert_window* win, const ioc_window_variant* var, int32_t n_sites,
                                         const char* slot_seq, const char* slot_qual, const int64_t* slot_off, char* out_seq, char* out_qual,
                                         int64_t cap, ioc_polish_stats* st, ioc_splice_site* out_sites, ioc_splice_stats* out_sstats);
/* ioc_planes_isoforms_full by variant: its arguments, except that iso_key holds a key2 per group-segment, var is packed with site_off
 * like win, and slot_seq / slot_qual / slot_off (2 site_off[n_segs] + 1 entries, as ioc_planes_insert_window_variants returns them)
 * stand in place of win_seq / win_qual / win_off.  Group-segment (g, h) is ioc_host_isoform_splice_variants over the tables
 * ioc_host_planes_pile makes of its pairs.  The kernels are ioc_planes_isoforms_full's; the plan kernel runs in its slot-aware
 * instantiation (a lane loads its window record, its variant record and both ends of its chosen slot), the call passes are the same
 * code.  The refusals and the capacity rule are ioc_planes_isoforms_full's, with "the bytes of g's windows" read as the bytes of g's
 * slots, plus what the definition refuses about var and slot_off (which must ascend from 0). */
int ioc_planes_isoforms_full_variants(ioc_ctx* ctx, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off,
                                      const int32_t* n_groups, int32_t n_pairs, const int32_t* seg_of_pair, const int32_t* group,
                                      const uint8_t* base, const uint8_t* slots, const uint64_t* iso_key, const ioc_insert_window* win,
                                      const ioc_window_variant* var, const int64_t* site_off, const char* slot_seq, const char* slot_qual,
                                      const int64_t* slot_off, int32_t min_depth, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off,
                                      ioc_polish_stats* out_polish, ioc_splice_stats* out_sstats, ioc_splice_site* out_splice,
                                      int64_t splice_cap, int64_t* splice_off, ioc_pileup_col* out_gcols, ioc_pileup_ins* out_gins);
/* ioc_align_pairs_blocks_inserts_variants and ioc_align_pairs_isoforms_full in one fused call: the arguments of the first followed by
 * max_iso and the isoform outputs of the second.  The six slot planes are projected as for the full call; the isoforms piled are
 * those counted again (ioc_read_variants.group: the first min(ioc_variants_seg.n_groups, max_iso) of a segment, direct and assigned
 * reads), the key of isoform h is key2 of its lowest-numbered direct read, and the splice runs the slot-aware plan over the slots the
 * same call just made.  Everything ioc_align_pairs_blocks_inserts_variants returns comes back byte for byte.  Where no site is kept
 * anywhere, and where sites are kept and none splits (key2 == key, slot 2 b is the window call's consensus), the isoform outputs are
 * ioc_align_pairs_isoforms_full's byte for byte.  iso_cap, splice_cap and cap follow ioc_align_pairs_isoforms_full's formulas — one
 * slot a site is taken, and a slot holds at most 7 max_win + 6 bytes, so a cap that passes before the call is never refused behind
 * the variant stage —, var_cap is the variant call's.  Every pair is aligned, piled and projected once, every voter aligned once
 * a round.  The refusals of both calls; nothing is written. */
int ioc_align_pairs_isoforms_full_variants(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch,
                                           int32_t gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats,
                                           int32_t n_segs, const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth,
                                           int32_t min_alt, int32_t min_pct, int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows,
                                           ioc_pile_block* out_blocks, int64_t blocks_cap, int64_t* block_off, ioc_read_blocks* out_reads,
                                           ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols, int32_t min_ins, int32_t slack, int32_t max_sites,
                                           ioc_insert_row* out_irows, ioc_pile_insert* out_sites, int64_t sites_cap, int64_t* site_off,
                                           ioc_read_inserts* out_ireads, ioc_inserts_seg* out_iseg, int32_t max_win, int32_t win_match,
                                           int32_t win_mismatch, int32_t win_gap, int32_t polish_min_depth, ioc_insert_window* out_win, char* out_wseq,
                                           char* out_wqual, int64_t win_cap, int64_t* out_woff, ioc_polish_stats* out_wstats, int32_t min_agree,
                                           ioc_window_variant* out_var, char* out_vseq, char* out_vqual, int64_t var_cap, int64_t* out_voff,
                                           ioc_polish_stats* out_vstats, uint8_t* out_variant, int32_t* out_agree, ioc_read_variants* out_vreads,
                                           ioc_variants_seg* out_vseg, int32_t max_iso, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off,
                                           ioc_polish_stats* out_polish, ioc_splice_stats* out_sstats, ioc_splice_site* out_splice,
                                           int64_t splice_cap, int64_t* splice_off, int64_t iso_cap, int64_t* iso_off);

/* ---- Alternative ends: where the reads of a cluster start and stop on their representative, and the variants that makes ----
 * A read that starts late or stops early has state IOC_BLOCK_NONE at the blocks it does not reach; this stage says where the ends
 * lie: start sites (an alternative first exon or start site), stop sites (an early polyadenylation site), which reads go on beyond
 * the representative there, and which (earlier isoform, start site, stop site) triples enough reads carry.
 *
 * The extent of one read, from its operation string: first_row / end_row the first row the base plane of ioc_host_ops_project
 * covers and one past the last ((0, 0) if it covers none: these are first_row / end_row of ioc_host_planes_blocks' read record),
 * head the 'i' bytes before the first walk byte (lead_i of ioc_host_ops_stats) and tail trail_i: the bases the read has in front of
 * and behind what it aligns.  The refusals of ioc_host_ops_project_ilen (IOC_ERR_ARG, nothing written). */
typedef struct {
    int32_t first_row, end_row, head, tail;
} ioc_read_extent;                /* 16 bytes */
int ioc_host_ops_extent(const char* ops, int64_t len, int32_t rlen, ioc_read_extent* out);
/* One segment is a reference of rlen rows with n_reads extents and, optionally, pre_group[i] >= -1 per read (NULL: all 0), meant
 * to be the isoform of an earlier stage.  A rule {slack in 0 .. 32, min_over >= 1, min_depth >= 1, min_alt >= 1, min_pct in 1 ..
 * 100, max_sites in 1 .. 32, max_variants >= 1}.  All integers.
 *  1. Read i takes part iff end_row > first_row; N is the number of reads that take part, a_i its first_row and z_i its end_row.
 *  2. hs(p), p = 0 .. rlen: the reads that take part with a_i == p; he(p) the same for z_i == p.
 *  3. Ws(p): the sum of hs(q) over q = max(p - slack, 0) .. min(p + slack, rlen); We(p) the same for he.
 *  4. Row p is a start row iff N >= min_depth and Ws(p) >= need(N), need(N) = max(min_alt, ceil(min_pct * N / 100)) as in
 *     ioc_host_pileup_sites — one-sided here: an end site is a site even if every read uses it.  Stop rows likewise with We.
 *  5. A start site [first, end): a maximal run of start rows.  In ascending order; the first max_sites are kept, n_found says how
 *     many there were.  Stop sites likewise.  Two true ends fewer than about 2 slack rows apart become ONE site.
 *  6. A read's distance to a kept start site b: 0 if first_b <= a_i < end_b, first_b - a_i below it, a_i - end_b + 1 above it.  Its
 *     start site is the b with the smallest distance <= slack, the lower b on a tie; -1 if there is none or the read takes no part.
 *     Its stop site likewise with z_i.  (The reach of slack is needed: with slack 1 and need 2, reads at rows 0 and 2 make row 1 the
 *     only start row, and both must land in site [1, 2).)
 *  7. The site record: n_reads the reads whose site it is; n_over those of them with head >= min_over (a start site) or tail >=
 *     min_over (a stop site) — reads that go on beyond what the representative has there: a start site at row 0 with a high n_over
 *     says the representative is the short one, one elsewhere a replaced first exon rather than a shorter transcript —; peak_row the
 *     row of [first, end) with the largest hs (stop site: he), the lowest on a tie, and peak_reads its count; kind 0 start, 1 stop.
 *  8. A read is placed when pre_group, start site and stop site are all >= 0.  The triples carried by at least min_alt placed reads
 *     are supported; in ascending order (pre_group major, then start site, then stop site) they are the variants.  The first
 *     max_variants are kept, n_found says how many there were.  A read's variant is the index of its triple among the kept, else -1.
 * No verdict on whether a variant is real is applied.  The sequence of a variant comes from what exists: the reads' `variant` as
 * `group` of ioc_planes_polish_groups; rows below its min_depth keep the representative's base, so that call trims nothing.
 * The defaults — slack 10, min_over 20, min_depth 3, min_alt 3, min_pct 10, max_sites 32, max_variants 64 — are choices made on
 * simulated reads, not measured on real data.  What stays out: telling two ends closer than 2 slack apart, a verdict on
 * degradation against real start sites, re-clustering. */
#define IOC_ENDS_MAX 32
#define IOC_ENDS_SLACK_MAX 32
#define IOC_END_START 0
#define IOC_END_STOP 1
typedef struct {
    int32_t first, end;
    uint32_t n_reads, n_over;
    int32_t peak_row;
    uint32_t peak_reads;
    int32_t kind;
    uint32_t reserved;
} ioc_end_site;                   /* 32 bytes */
typedef struct {
    int32_t pre_group, start_site, stop_site;
    uint32_t n_reads;
} ioc_end_variant;                /* 16 bytes */
typedef struct {
    int32_t start_site, stop_site, variant, reserved;
} ioc_read_ends;                  /* 16 bytes */
typedef struct {
    int32_t n_reads, n_starts, n_starts_found, n_stops, n_stops_found, n_variants, n_variants_found, n_placed;
} ioc_ends_seg;                   /* 32 bytes; n_reads is N */
typedef struct {
    uint32_t starts, stops, w_starts, w_stops;  /* hs, he, Ws, We; rlen + 1 rows per segment */
} ioc_end_row;                    /* 16 bytes */
/* The definition: one segment, the plain loops above.  out_rows (may be NULL): rlen + 1 rows; out_starts / out_stops: room for
 * min(max_sites, rlen + 1) records each, of which the first out_seg->n_starts / n_stops are written; out_variants: room for
 * min(max_variants, n_reads) records, of which the first out_seg->n_variants are written; out_reads: n_reads records.  IOC_ERR_ARG,
 * with nothing written, for a rule outside its ranges, a negative count or length, pre_group[i] < -1, an extent with first_row <
 * 0, end_row > rlen, end_row < first_row, head < 0 or tail < 0, and a NULL pointer that is needed. */
int ioc_host_reads_ends(const ioc_read_extent* extents, const int32_t* pre_group, int32_t n_reads, int32_t rlen, int32_t slack,
                        int32_t min_over, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_sites, int32_t max_variants,
                        ioc_end_row* out_rows, ioc_end_site* out_starts, ioc_end_site* out_stops, ioc_end_variant* out_variants,
                        ioc_read_ends* out_reads, ioc_ends_seg* out_seg);
/* Many segments at once on the device, from host arrays, which are uploaded: extents (and pre_group, or NULL) per pair, a segment's
 * reads its pairs in ascending order.  The kernels of ioc_read_ends.hip: the two histograms by integer adds into zeroed rows, the
 * windowed sums by a wave prefix sum with a halo, start and stop rows as bit planes by ballot, the runs of set bits across words, a
 * wave per read for its nearest sites, a wave per kept site for its counts and its peak, and the variants as the isoforms of the
 * block stage over one 64-bit key a read.  out_rows (may be NULL): the segments' tables one behind the other; out_sites: segment
 * g's start sites at site_off[2 g] .. site_off[2 g + 1], its stop sites at site_off[2 g + 1] .. site_off[2 g + 2] (2 n_segs + 1
 * entries); out_variants packed with var_off (n_segs + 1 entries); out_reads per pair, out_seg per segment; each as
 * ioc_host_reads_ends defines it, byte for byte.  IOC_ERR_ARG, with nothing written, for what the definition refuses, seg_of_pair
 * outside the segments and a NULL pointer that is needed; IOC_ERR_CAPACITY, with nothing written, for sites_cap below the sum over g
 * of 2 min(max_sites, rlen[g] + 1) and for variants_cap below the sum over g of min(max_variants, reads of g). */
int ioc_reads_ends(ioc_ctx* ctx, int32_t n_segs, const int32_t* rlen, int32_t n_pairs, const int32_t* seg_of_pair,
                   const ioc_read_extent* extents, const int32_t* pre_group, int32_t slack, int32_t min_over, int32_t min_depth,
                   int32_t min_alt, int32_t min_pct, int32_t max_sites, int32_t max_variants, ioc_end_row* out_rows,
                   ioc_end_site* out_sites, int64_t sites_cap, int64_t* site_off, ioc_end_variant* out_variants, int64_t variants_cap,
                   int64_t* var_off, ioc_read_ends* out_reads, ioc_ends_seg* out_seg);
/* ioc_align_pairs_blocks with the ends stage behind the block kernels: everything ioc_align_pairs_blocks returns comes back
 * unchanged, byte for byte; added are out_extents per pair — first_row / end_row the block record's, head / tail lead_i / trail_i of
 * the pair's statistics record, for which k_ops_stats runs over every slice whether or not out_stats is asked; out_extents[i] is
 * ioc_host_ops_extent of what ioc_align_pairs_ops returns for pair i, all zero for a pair without an alignment — and the outputs of
 * ioc_reads_ends over them, pre_group being the block stage's group, read where it lies on the device.  The block search and the
 * ends share min_depth and min_alt; min_pct is each stage's own (ends_min_pct).  Every pair is aligned, piled and projected exactly
 * once; the stage's memory is reserved after the walks.  The refusals of both calls; nothing is written. */
int ioc_align_pairs_blocks_ends(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch,
                                int32_t gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats,
                                int32_t n_segs, const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_gap, int32_t min_depth,
                                int32_t min_alt, int32_t min_pct, int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows,
                                ioc_pile_block* out_blocks, int64_t blocks_cap, int64_t* block_off, ioc_read_blocks* out_reads,
                                ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols, int32_t slack, int32_t min_over, int32_t ends_min_pct,
                                int32_t max_sites, int32_t max_variants, ioc_read_extent* out_extents, ioc_end_row* out_erows,
                                ioc_end_site* out_sites, int64_t sites_cap, int64_t* site_off, ioc_end_variant* out_variants,
                                int64_t variants_cap, int64_t* var_off, ioc_read_ends* out_ereads, ioc_ends_seg* out_eseg);

/* ---- Read correction by isoform: every read held against the tables of its own isoform, long insertions kept ----
 * ioc_host_read_correct holds a read against the pileup of its whole cluster and cannot take a read whose alignment inserts more
 * than IOC_PILE_INS_SLOTS bases in a row.  Here the tables are those of the read's isoform, and such a run is carried through as
 * the read has it while the rest of the read is corrected.
 *
 * The definition, one read: ioc_host_read_correct's inputs, the read's length plane ilen[rlen + 1] (ioc_host_ops_project_ilen),
 * its position plane qpos[rlen + 1] (ioc_host_ops_project_qpos) and the read itself, query[qlen].  All integers.
 *  A row p, 0 <= p <= rlen, with ilen[p] > IOC_PILE_INS_SLOTS is a long row: its insertion step emits query[qpos[p] .. qpos[p] +
 *  ilen[p]) as the read has it, each byte at quality 0 ('!'), whatever the depth; the slot rule is not applied at that row and it
 *  adds nothing to n_sub, n_ins_add or n_ins_drop.  Its base, and every other row, is exactly ioc_host_read_correct's: the base
 *  decision, the run guard (long rows neither start nor end a run) and the qualities.  With no long row the output is
 *  ioc_host_read_correct's, byte for byte.  n_long_runs counts the long rows, n_long_bases their bytes.
 *  The pair is unresolved — out_len 0, nothing written, every counter 0 and IOC_ISOC_UNRESOLVED set in flags; not an error of the
 *  call — where some ilen[p] == 255 (the plane's cap: the length is not known), where a long row has qpos[p] + ilen[p] > qlen (a
 *  plane that is not this read's) and where a long row stands at a row the read does not span (as ioc_host_read_correct spans).
 *  The long runs of a read do not overlap, so together they are no longer than the read, which is what the bound on cap counts
 *  on: planes whose long rows sum to more than qlen are not this read's either, and the pair is unresolved likewise.
 *  `table` is the batched calls' to set; the definition writes 0. */
#define IOC_ISOC_UNRESOLVED 1
typedef struct {
    int32_t out_len, n_sub, n_fill, n_remove;
    int32_t n_ins_add, n_ins_drop, n_low, n_guarded;
    int32_t table;                /* the group-segment held against, or -1 - segment for the cluster's table */
    int32_t n_long_runs, n_long_bases;
    int32_t flags;
} ioc_iso_correct_stats;          /* 48 bytes */
/* Returns the length written (0 for an unresolved pair); *st (may be NULL) the record.  IOC_ERR_ARG for what ioc_host_read_correct
 * refuses, a NULL ilen or qpos, qlen < 0 and a NULL query with qlen > 0; IOC_ERR_CAPACITY for cap below rlen + IOC_PILE_INS_SLOTS *
 * (rlen + 1) + qlen; nothing is written on either. */
int64_t ioc_host_read_correct_long(const uint8_t* base, const uint8_t* slots, const uint8_t* ilen, const uint32_t* qpos, int32_t rlen,
                                   const ioc_pileup_col* cols, const ioc_pileup_ins* ins, const char* frame, const char* query,
                                   int32_t qlen, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_run, char* out_seq,
                                   char* out_qual, int64_t cap, ioc_iso_correct_stats* st);
/* Every pair of many segments at once on the device, from host planes.  The segments and their frames as for ioc_pileup_call;
 * n_groups, group and seg_of_pair as for ioc_planes_polish_groups (gseg_off its numbering, G group-segments in all); query[i] a
 * sequence of the pool that is set, as for ioc_planes_insert_windows; base, slots, ilen (a byte a row) and qpos (a word a row) the
 * pairs' planes laid out as for ioc_planes_polish.
 *  Which table: T(g, h) is piled (ioc_host_planes_pile) from the planes of the pairs of segment g in group h, T(g, *) from all
 *  pairs of segment g whatever their group.  Pair i of segment g is held against T(g, group[i]) where group[i] >= 0 and that group
 *  has at least min_depth members (table = gseg_off[g] + group[i]), else against T(g, *) (table = -1 - g): what
 *  ioc_planes_correct does for every read.  Pair i is ioc_host_read_correct_long over that table and the frame of g.
 * k_group_pile (ioc_group_pile.hip) piles the G + n_segs tables — the extra one per segment lists all of its pairs, and is left
 * empty where no pair of the segment is held against it —, and
 * k_iso_correct_count / k_iso_correct_emit (ioc_iso_correct.hip) take a wave per pair, a lane per row: a count pass, a scan, and
 * a write pass in which the whole wave copies a long run from the pool.  Pair i's bytes stand at out_off[i] .. out_off[i + 1] of
 * out_seq / out_qual (out_off: n_pairs + 1 entries), its record in out_stats[i] (may be NULL).
 * IOC_ERR_ARG, with nothing written, for what ioc_planes_correct and ioc_planes_polish_groups refuse and for a query outside the
 * pool; IOC_ERR_CAPACITY, with nothing written, for cap below the sum over the pairs of (their segment's bound + their query's
 * length) and for a segment whose bound exceeds 2^31 - 1. */
int ioc_planes_correct_groups(ioc_ctx* ctx, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off,
                              const int32_t* n_groups, int32_t n_pairs, const int32_t* seg_of_pair, const int32_t* group,
                              const int32_t* query, const uint8_t* base, const uint8_t* slots, const uint8_t* ilen,
                              const uint32_t* qpos, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_run,
                              char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_iso_correct_stats* out_stats);
/* ioc_align_pairs_blocks with the correction by isoform behind the block kernels: everything ioc_align_pairs_blocks returns comes
 * back unchanged, byte for byte; the pile projects the slot, length and position planes as well (12 bytes per row and pair, which
 * count against the checkpoint arena's budget; a call of ioc_align_pairs_blocks reserves what it always did), and behind the block
 * kernels ioc_planes_correct_groups' kernels run over the planes where they lie, with ioc_read_blocks.group as the groups and the
 * block stage's n_groups, under the rule correct_*.  out_seq / out_qual / out_off / out_correct per PAIR as from
 * ioc_planes_correct_groups.  Every pair is aligned, piled and projected exactly once; the stage's memory is reserved after the
 * walks.  The refusals of both calls; nothing is written. */
int ioc_align_pairs_blocks_correct(ioc_ctx* ctx, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch,
                                   int32_t gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio,
                                   ioc_aln_stats* out_stats, int32_t n_segs, const ioc_polish_seg* segs, const int32_t* seg_of_pair,
                                   int32_t min_gap, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t min_block,
                                   int32_t max_blocks, ioc_block_row* out_rows, ioc_pile_block* out_blocks, int64_t blocks_cap,
                                   int64_t* block_off, ioc_read_blocks* out_reads, ioc_blocks_seg* out_seg, ioc_pileup_col* out_cols,
                                   int32_t correct_min_depth, int32_t correct_min_alt, int32_t correct_min_pct, int32_t correct_max_run,
                                   char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_iso_correct_stats* out_correct);

#ifdef __cplusplus
}
#endif
#endif /* ISONCLUST2_HIP_H */
