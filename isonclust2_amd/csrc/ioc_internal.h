// ioc_internal.h — the context's layout and the device helpers shared by the host code of every translation unit: the C ABI
// (ioc_capi.cpp and the host halves of ioc_extract.hip, ioc_update.hip, ioc_align_gpu.hip, ioc_poa.hip), the drivers on top of it
// (ioc_host.cpp, ioc_consensus.cpp) and the multi-GPU binding (ioc_dist.cpp).  Not part of the public C ABI
// (include/isonclust2_hip.h).
#ifndef IOC_INTERNAL_H
#define IOC_INTERNAL_H

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <map>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "ioc_align_plan.h"
#include "ioc_sink_plan.h"
#include "isonclust2_hip.h"

// A block of device memory and its owner: freed when the DevBuf goes (a member of a context with the context, a local at the end
// of its scope), movable, not copyable.  No DevBuf has static storage: the destructor calls into HIP, which a destructor
// that runs after the runtime's teardown must not do.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    void release();  // hipFree now (no synchronisation of its own: the caller knows what may still use the block)
    template <class T>
    T* as() const
    {
        return static_cast<T*>(p);
    }
};

// IOC_POISON=<byte>: every fresh device allocation of the library is filled with that byte (debug aid: a kernel that reads
// memory nobody wrote gives results that change with the byte; a fresh process otherwise sees zero-filled VRAM and hides it)
void ioc_poison(void* p, size_t bytes);

struct ioc_dist_state;  // ioc_dist.cpp: the context's RCCL communicator

// The control words kernels and host share: the first 256 bytes of b_misc (kernels get pointers INTO this block: the byte
// positions are part of no interface, but index build, scoring, resolve and the timings must agree on them) ...
struct IocMisc {
    uint32_t build_err;  // index build: the table is full (the hash build tries again with a larger one)
    uint32_t pad0[7];
    uint32_t first_changed;        // resolve, per sweep: first query whose `valid` changed (0xFFFFFFFF: none)
    uint32_t q_count;              // ... fill of the work queue, first half of a sweep
    uint32_t incomplete;           // ... the queue overflowed: the same sweep again
    uint32_t q_count2;             // ... fill of the work queue, second half
    uint32_t pad1[4];
    unsigned long long traversed;  // scoring: postings traversed (IOC_COUNT_TRAVERSED)
    uint32_t pad2[14];
    unsigned long long n_evals;    // resolve: totalMapped evaluations of the call
    uint32_t pad3[14];
    unsigned long long audit_sum;  // ioc_count_reference_postings
    uint32_t pad4[14];
};
static_assert(sizeof(IocMisc) == 256 && offsetof(IocMisc, first_changed) == 32 && offsetof(IocMisc, traversed) == 64 &&
                  offsetof(IocMisc, n_evals) == 128 && offsetof(IocMisc, audit_sum) == 192,
              "kernels are handed pointers to these bytes");
// ... and the words of the 256 pinned bytes of h_pin they are read back into.  One copy per sweep brings IocMisc from
// first_changed through n_evals to the start of h_pin; the build's read-back lies inside that window (a build and a sweep are never
// in flight together), the sorted build's postings count beyond it (it is read when the timings are asked for).
constexpr size_t IOC_PIN_BYTES = 256;
constexpr size_t IOC_SWEEP_BYTES = offsetof(IocMisc, n_evals) + 8 - offsetof(IocMisc, first_changed);
enum : uint32_t {
    IOC_PIN_FIRST_CHANGED = 0,
    IOC_PIN_INCOMPLETE = (offsetof(IocMisc, incomplete) - offsetof(IocMisc, first_changed)) / 4,
    IOC_PIN_BUILD = 8,  // two words: (real pairs, runs) of the sorted build, (error word, padded postings) of the hash build
    IOC_PIN_EVALS = (offsetof(IocMisc, n_evals) - offsetof(IocMisc, first_changed)) / 4,  // two words
    IOC_PIN_NPOST = 40,  // the sorted build's padded postings
};
static_assert(IOC_SWEEP_BYTES == 104 && IOC_PIN_INCOMPLETE == 2 && IOC_PIN_EVALS == 24 && IOC_PIN_NPOST * 4 >= IOC_SWEEP_BYTES && IOC_PIN_NPOST * 4 + 4 <= IOC_PIN_BYTES, "h_pin layout");

struct ioc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    std::string err;
    DevBuf b_misc;              // IocMisc; behind it ioc_gather_records_device's list table
    uint32_t* h_pin = nullptr;  // IOC_PIN_BYTES of pinned host memory (IOC_PIN_*): the read-backs of the build and of the resolve's sweeps

    // ---- parameters (ioc_set_params) ----
    bool have_params = false;
    ioc_params params{};
    int32_t h_glim[225]{};
    DevBuf b_glim;
    int32_t keep = 1;  // candidates with Size < keep can never be evaluated (cluster.cpp:376-389)

    // ---- queries ----
    int32_t n = 0;
    int64_t total = 0;
    bool borrowed = false;
    std::vector<int64_t> h_off_fwd, h_off_rev, h_doff;
    const int64_t* d_off_fwd = nullptr;
    const int64_t* d_off_rev = nullptr;
    const uint32_t* d_min = nullptr;
    const uint32_t* d_pos = nullptr;
    const uint32_t* d_hpc_len = nullptr;
    const uint8_t* d_err_cell = nullptr;
    const uint32_t* d_min_total = nullptr;
    DevBuf b_off_fwd, b_off_rev, b_min, b_pos, b_hpc_len, b_err_cell, b_min_total, b_doff;
    int32_t max_fwd = 0, max_rev = 0;
    uint64_t query_gen = 0;  // bumped whenever the context's queries are replaced (ioc_queries_generation)
    bool chunked_call = false;  // the last ioc_cluster_merge ran its right batch in chunks: the resident queries are the last chunk's
    // ioc_cluster_merge (caller's arrays valid for the whole call): the index build needs the forward minimizer values
    // only, the scoring the reverse ones too, the resolve the positions — the latter two go up on a copy stream from a
    // thread of their own while the first kernels run (ioc_queries_upload, ioc_wait_uploads)
    bool defer_uploads = false;
    std::thread up_thread;
    hipStream_t copy_stream = nullptr;
    std::atomic<int> up_stage{2};  // 1: all minimizer values are in HBM, 2: the positions too
    std::atomic<bool> up_failed{false};  // a copy of the upload thread failed (up_err holds the text): set before the stage moves on
    std::string up_err;

    // ---- left state ----
    int32_t L = 0;
    int64_t n_left_keys = 0, n_left_post = 0;
    DevBuf b_left_err, b_lkeys, b_loffs, b_lpost, b_lslot;
    // left clusters' value sets (transposed MinDB), built by ioc_left_load
    DevBuf b_lset_off, b_lset_val;
    std::vector<int64_t> h_lset_off;  // host copy of the value-set offsets (ioc_index_update)
    // ioc_left_adopt builds the next left state here and swaps it in: the blocks the swap retires serve the adoption after it
    DevBuf b_alt_err, b_alt_keys, b_alt_offs, b_alt_set_off, b_alt_set_val, b_adopt_work;

    // ---- index (ioc_index_build) ----
    bool built = false;
    uint32_t cap = 0;  // power of two; slot `cap` is reserved for the key 0xFFFFFFFF
    DevBuf b_keys, b_cnt, b_off, b_fill, b_rows, b_post, b_dvals, b_dcount, b_dslot, b_scan;
    DevBuf b_qinfo;  // two words per slot: length + epoch cuts (ioc_kernels.hip, index_lookup)
    DevBuf b_dlong;  // the long queries' values gathered / sorted (iock_distinct_long)
    DevBuf b_bsort;  // the sorted build's arena (ioc_build_sort.hip)
    int64_t n_post = 0;
    int post16 = 0;  // postings stored as uint16_t (L + N <= 65535)

    // ---- scoring (ioc_score) ----
    bool scored = false;
    DevBuf b_cand_key, b_cand_size, b_cand_mapped, b_cand_count, b_part, b_top_all, b_pmins, b_pbnd;
    int64_t cand_capacity = 0;
    DevBuf b_gap_bound, b_keep_q;  // k_gap_bounds' table of the current queries; the per-query compaction threshold (fast mode)
    uint64_t gap_bound_gen = ~0ull;  // query_gen the table was computed for (ioc_set_params resets it)
    bool gap_bound_cut = false;      // ... with keep_q written
    bool keep_q_on = false;          // the candidate lists of the last ioc_score were cut at b_keep_q
    std::vector<uint32_t> h_keep_q;  // host copy, fetched when a candidate table is exported
    int score_oob = 0, score_oob_probe = -1;  // k_score_part's variant and the probe behind it (ioc_ctx_create)
    int score_part32 = 0;  // u32 partials forced (IOC_PART32) in the last ioc_score: ioc_count_reference_postings' audit uses it too

    // ---- resolve (ioc_resolve, ioc_get_decisions) ----
    bool resolved = false;
    DevBuf b_valid0, b_valid1, b_dec_target, b_dec_strand, b_flags, b_forced_t, b_forced_s, b_queue, b_cut, b_diag;
    int cur_valid = 0;
    std::vector<int32_t> h_forced_t;
    std::vector<int8_t> h_forced_s;
    bool forced_dirty = false;
    bool forced_host_clear = false, forced_dev_clear = false;  // nothing forced in the host arrays / in what the device holds (no upload then)
    // verdicts of the alignment fallback (ioc_set_aln_verdicts) and the candidates tied at the top Size (ioc_get_ties)
    DevBuf b_aln_t, b_aln_s, b_tie_count, b_tie_keys;
    std::vector<int32_t> h_aln_t;
    std::vector<int8_t> h_aln_s;
    bool aln_verdicts = false, aln_dirty = false;
    // warm start: first query whose alignment verdict changed since the last resolve (n: none; -1: no
    // resolved state to start from).  Everything before it keeps its decision (it depends on earlier queries only).
    int32_t warm_first = -1;
    uint8_t* h_pin_big = nullptr;  // pinned staging for the per-call read-backs of n-sized arrays (decisions)
    size_t h_pin_big_cap = 0;
    DevBuf b_qhist, b_qfirst, b_qout, b_qlist;  // ioc_query_candidates: the query's hit table (kept between calls)

    // ---- ioc_index_export result of the current resolve ----
    DevBuf b_exp_cid, b_exp_cnt, b_exp_off, b_exp_out, b_exp_work;  // final ids, per-slot counts / offsets, compact postings
    bool exp_valid = false;   // exp_keys / exp_offs / exp_post hold the export (consensus driver; IOC_EXPORT_HOST_ORDER)
    bool exp_dev = false;     // the export is ready ON THE DEVICE: exp_nrows keys at b_exp_work + exp_o_keys, exp_nrows + 1 int64
                              // offsets at + exp_o_offs, exp_total postings in b_exp_out (copied straight into the caller's arrays)
    int32_t exp_clusters = 0;  // clusters of the exported state: L + the queries that opened one
    uint32_t exp_nrows = 0;
    uint64_t exp_total = 0;
    size_t exp_o_keys = 0, exp_o_offs = 0;
    std::vector<uint32_t> exp_keys, exp_post;
    std::vector<int64_t> exp_offs;

    // ---- extraction (K1) outputs ----
    DevBuf x_min, x_pos, x_off_fwd, x_off_rev, x_hpc_len, x_hseq, x_hqual;
    std::vector<int64_t> xh_offs;
    int32_t x_n = 0;
    int64_t x_total = 0;
    std::vector<int64_t> xh_off_fwd, xh_off_rev;
    std::vector<uint32_t> xh_hpc_len;
    std::vector<int32_t> xh_status;
    std::vector<uint8_t> x_keep;

    // ---- GPU alignment fallback (ioc_align_gpu.hip) ----
    DevBuf a_pool, a_pairs, a_order, a_out, a_bnd, a_lrow, a_ck, a_cko, a_ends, a_ends2, a_xflags, a_prof, a_ops;
    DevBuf a_ostats;  // ioc_align_pairs_stats: the records of a slice (k_ops_stats)
    DevBuf a_pile_ins;  // ioc_align_pairs_polish: the second table, what the reads insert (the ins variant of k_ops_pileup)
    DevBuf a_call;      // ioc_pileup_call, ioc_align_pairs_polish: segments, offsets, records and the called bytes (ioc_pile_call.hip); the
                        // read correction's write pass: [sequence][qualities], as many bytes as its count pass found
    DevBuf a_pile_w;    // ioc_align_pairs_polish_weighted: the tables of weights, [wcols][wins] of the call's rows (ioc_pileup_call_weighted: wcols
                        // alone, wins where ioc_pileup_call has ins)
    DevBuf a_qual;      // ioc_align_set_pool_qual: one quality byte per byte of a_pool ...
    bool aln_qual_set = false;  // ... which it holds for the current pool
    DevBuf a_planes;  // ioc_align_pairs_alleles: every pair's projection, [base planes][ins planes] (k_ops_project)
                      // and, for ioc_align_pairs_split_polish, [slot planes x 6] behind them (k_ops_project_ins) and, for
                      // ioc_align_pairs_blocks_polish_weighted, [weight planes x 7] behind those (k_ops_project_weights)
    DevBuf a_split;   // ioc_alleles_split, ioc_align_pairs_split: member lists, bit planes, per-site and per-pair words (ioc_site_split.hip)
    DevBuf a_gpile;   // ioc_planes_polish, ioc_align_pairs_split_polish: the group-segments, their work items and tables (k_plane_pile) and,
                      // from host planes, the uploaded member lists and planes; ioc_planes_polish_groups, ioc_align_pairs_blocks_polish: the
                      // same of k_group_pile, with every group's own member list; ioc_planes_polish_groups_weighted,
                      // ioc_align_pairs_blocks_polish_weighted: the same of k_group_pile_weighted, with the uploaded weight planes and gwcols / gwins
    DevBuf a_correct; // ioc_planes_correct, ioc_align_pairs_correct: segments, pairs, offsets, records and the corrected bytes (ioc_read_correct.hip) and,
                      // from host planes, the uploaded planes
    DevBuf a_inserts; // ioc_planes_inserts, ioc_align_pairs_blocks_inserts: the tables, bit planes and records of ioc_read_inserts.hip and, uploaded, both planes
    DevBuf a_windows; // ioc_planes_insert_windows, ioc_align_pairs_blocks_inserts_seq: the tables, the (pair, site) entries and the records of
                      // k_win_bounds / k_win_template and, uploaded, both planes; the alignments' items, planes and direction words share a_gpile
                      // with the group pile behind them
    DevBuf a_winvar;  // ioc_planes_insert_window_variants: the flags, agreements, records and variant bytes of ioc_window_variants.hip, key2 / mask2 and the
                      // recount's records and, uploaded, pre_key / pre_mask / pre_full and round A's entries; round A's alignments lie in a_gpile
    DevBuf a_winvar_b; // ... round B's items, entries, planes and direction words, and the group pile of the (site, variant) slots behind both rounds
    DevBuf a_rends;   // ioc_reads_ends, ioc_align_pairs_blocks_ends: the tables, histograms, bit planes and records of ioc_read_ends.hip and, uploaded,
                      // the extents and pre_group
    DevBuf a_splice;  // ioc_planes_isoforms_full, ioc_align_pairs_isoforms_full: keys, windows, plans, records and the spliced bytes (ioc_iso_splice.hip)
    DevBuf a_blocks;  // ioc_planes_blocks, ioc_align_pairs_blocks: segments, pairs, member lists, bit planes, tables and records (ioc_read_blocks.hip) and,
                      // from host planes, the uploaded planes
    DevBuf a_pile;    // ioc_align_pairs_pileup: the table of the call's rows (k_ops_pileup adds into it, slice after slice)
    std::vector<uint8_t> aln_other;  // per pool sequence: holds a byte other than A C G T
    std::vector<int64_t> aln_offs;
    hipStream_t side_stream = nullptr;  // the aligner's helper launch for the wrong candidates, beside the first traceback launch
    hipEvent_t ev_side[2]{};
    size_t aln_lds_max = 0, aln_lds_max2 = 0;  // dynamic LDS a k_align_fwd<true/false> workgroup may reserve (residency cap)
    double aln_verdict_thr = -1.0;  // ioc_align_set_verdict_threshold (<= 0: exact counts)
    CorridorFit aln_fit[4];              // the aligner's corridor model (ioc_align_plan.h), fed by ioc_align_gpu.hip's learn_corridor
    int32_t aln_fit_sig[3] = {0, 0, 0};  // (match, mismatch, gap_extend) the sums belong to

    // ---- host drivers (ioc_host.cpp, ioc_consensus.cpp) ----
    // raw sequences of the resident queries (ioc_resident_set_sequences): sahlin on ioc_cluster_resident
    std::string res_seq;
    std::vector<int64_t> res_off;
    std::vector<double> res_err;
    bool have_res_seq = false;
    bool res_pool_ready = false;  // a_pool holds exactly res_seq
    std::vector<uint32_t> h_min_total;  // host copy of d_min_total for ioc_cluster_resident's tie replays, of queries `h_min_total_gen`
    uint64_t h_min_total_gen = ~0ull;
    bool want_dep_sets = false;  // (ioc_cluster_consensus: run_pipeline leaves last_order_dep / last_dep_set)
    std::vector<uint8_t> last_order_dep;  // per query of the last run_pipeline: its decision hangs on the reference's hit ORDER (a tie at the top Size, or several candidates that align)
    std::vector<std::vector<std::pair<int32_t, int8_t>>> last_dep_set;  // ... and the (cluster, strand) candidates among which that order picks the first
    // alignment results kept across the device passes of ioc_cluster_consensus (see AlnDriver)
    std::vector<uint64_t> aln_qid, aln_lid;  // sequence identity of every right entry / left representative
    std::map<std::pair<uint64_t, uint64_t>, double> aln_cache;

    // ---- instrumentation ----
    hipEvent_t ev[6]{};
    ioc_timings tm{};

    // ---- multi-GPU (ioc_dist.cpp) ----
    ioc_dist_state* dist = nullptr;
    DevBuf b_dist_min, b_dist_pos;  // the gathered representatives' minimizer lists of ioc_dist_merge (used in place as queries)
    // sharded score + resolve (ioc_set_shard): this rank owns the queries j with j % shard_world == shard_rank
    int shard_world = 1, shard_rank = 0;
    ioc_exchange_fn shard_fn = nullptr;
    void* shard_user = nullptr;
    bool scored_sharded = false;  // the candidate tables hold the owned queries only
    int shard_exchanges = 0;
    int64_t shard_aln_pairs = 0;  // pairs THIS rank aligned in sharded alignment rounds since ioc_set_shard
    DevBuf b_shard_stage;
};

int ioc_fail(ioc_ctx* c, int code, const std::string& msg);

// Entries one device pass takes (the all-pairs candidate tables grow with the square of the entries).  ioc_index_build refuses
// more; ioc_cluster_merge runs a larger right batch in chunks, ioc_cluster_consensus in windows of at most this many entries.
constexpr int32_t IOC_PASS_ENTRIES = 131072;
// ... and what the two drivers cut at: IOC_MERGE_CHUNK (entries, 1 .. IOC_PASS_ENTRIES) when set, else IOC_PASS_ENTRIES
int32_t ioc_pass_entries();
// ioc_capi.cpp: the export of the current resolve (ioc_index_export) ready ON THE DEVICE (ioc_ctx::exp_dev), whatever
// IOC_EXPORT_HOST_ORDER says
int ioc_export_on_device(ioc_ctx* c);

// a HIP call of a function that returns an ioc status: on failure "<call text>: <hipGetErrorString>" and IOC_ERR_HIP
#define IOC_CHK(c, call)                                                                           \
    do {                                                                                           \
        hipError_t e__ = (call);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return ioc_fail((c), IOC_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)

// a call that returns an ioc status: anything but IOC_OK is returned at once (the callee has set the message)
#define IOC_TRY(call)                  \
    do {                               \
        int r__ = (call);              \
        if (r__ != IOC_OK) return r__; \
    } while (0)

// `b` holds at least `bytes` bytes afterwards (0 bytes: 16).  A block that has to grow is freed behind a synchronisation of
// c->stream and allocated anew at bytes + bytes / 8 + 256, poisoned (IOC_POISON); its old contents are gone.  Out of memory:
// IOC_ERR_CAPACITY, with the size in the message.
int ioc_reserve(ioc_ctx* c, DevBuf& b, size_t bytes);
// the scoped temporary: a fresh block of exactly `bytes` bytes (0: 16) in an empty DevBuf, which frees it at the end of its scope
int ioc_alloc(ioc_ctx* c, DevBuf& b, size_t bytes);
// sharded score + resolve (ioc_set_shard): one all-reduce through the caller's hook / a host array of words summed over ranks
int ioc_shard_exchange(ioc_ctx* c, void* d_buf, int64_t count, int kind);
int ioc_shard_sum_host(ioc_ctx* c, int32_t* words, int64_t count);
// waits until the background upload of the query arrays has reached `stage` (see ioc_ctx::up_stage); 2 also ends the thread
int ioc_wait_uploads(ioc_ctx* c, int stage);

// ioc_query_candidates for many queries at once (one launch per chunk, one synchronisation): per query the same
// lists — target, strand (+1 / -1), Size, first hitting Index, cached totalMapped (0xFFFFFFFF: not evaluated) —
// in ascending (strand +1 first, target) order.  Internal: used by the hitOrder replay of the sahlin driver.
struct IocCandTable {
    int q = 0;
    std::vector<int32_t> tg;
    std::vector<int8_t> st;
    std::vector<uint32_t> sz, fi, tm;
};
int ioc_query_candidates_many(ioc_ctx* c, const std::vector<int>& qs, std::vector<IocCandTable>& out);
// ioc_capi.cpp: ioc_get_decisions + ioc_get_ties (tie_count and tie_keys, both or neither) + ioc_get_cuts (cut; null: left out)
// behind one wait for the stream: what run_pipeline reads after every resolve
__attribute__((visibility("hidden"))) int ioc_get_resolved(ioc_ctx* c, int32_t* target, int8_t* strand, uint8_t* flags, uint32_t* tie_count,
                                                           uint32_t* tie_keys, int32_t* cut);

// events of a call's launches (the aligner: three per slice — the forward pass, the traceback, the end), destroyed on every way
// out, the IOC_CHK returns included
struct __attribute__((visibility("hidden"))) EventSet {
    std::vector<hipEvent_t> v;
    ~EventSet()
    {
        for (auto& e : v)
            if (e) (void)hipEventDestroy(e);
    }
};

// the aligner's sequence pool (ioc_align_set_pool): the length of sequence `id`, and the one check that a pair's two lie in it
static inline int64_t ioc_seq_len(const ioc_ctx* c, int32_t id) { return c->aln_offs[size_t(id) + 1] - c->aln_offs[size_t(id)]; }
static inline int ioc_pair_in_pool(ioc_ctx* c, const ioc_aln_pair& a)
{
    const int64_t n_seqs = c->aln_offs.empty() ? 0 : int64_t(c->aln_offs.size()) - 1;
    if (a.query < 0 || a.query >= n_seqs || a.ref < 0 || a.ref >= n_seqs)
        return ioc_fail(c, IOC_ERR_ARG, "alignment pair refers to a sequence outside the pool");
    return IOC_OK;
}

// ioc_align_gpu.hip: ioc_align_pairs with the walks' operation bytes handed to `sink` (ioc_align_sink.h; null: no walk emits) —
// what the emitting entry points of ioc_align_sinks.cpp run
struct AlnSink;
__attribute__((visibility("hidden"))) int ioc_align_pairs_sink(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match,
                                                               int32_t mismatch, int32_t gap_extend, int32_t* out_score, int64_t* out_windows,
                                                               double* out_ratio, const AlnSink* sink);

// ioc_ops_stats.hip: the statistics (ioc_host_ops_stats) of the operation strings an emitting slice of the aligner left on the
// device — pair ord[x]'s string is buf[end[pid] - len[pid] .. end[pid]), its record out[x]; a pair with len == 0, len > room or
// len > end is skipped
hipError_t iock_ops_stats(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room,
                          const uint32_t* ord, uint32_t cnt, ioc_aln_stats* out);

// ioc_ops_pileup.hip: the same strings piled onto their references (ioc_host_ops_pileup) — pair pid adds into the records of
// `cols` from row_base[pid] on (negative: skipped), its query bases read at pool + q_off[pid]; the same pairs are skipped
hipError_t iock_ops_pileup(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room,
                           const uint32_t* ord, uint32_t cnt, const int64_t* row_base, const uint32_t* q_off, const uint8_t* pool,
                           uint64_t pool_bytes, ioc_pileup_col* cols, uint64_t n_rows);

// ... and what they insert into `ins` as well (ioc_host_ops_pileup_ins): the variant of ioc_align_pairs_polish
hipError_t iock_ops_pileup_ins(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room,
                               const uint32_t* ord, uint32_t cnt, const int64_t* row_base, const uint32_t* q_off, const uint8_t* pool,
                               uint64_t pool_bytes, ioc_pileup_col* cols, ioc_pileup_ins* ins, uint64_t n_rows);

// ... and the weights of the same events into wcols / wins (ioc_host_ops_pileup_weighted): the variant of
// ioc_align_pairs_polish_weighted; q_len[pid]: the pair's query length, quals: one quality byte per byte of the pool
hipError_t iock_ops_pileup_weighted(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room,
                                    const uint32_t* ord, uint32_t cnt, const int64_t* row_base, const uint32_t* q_off, const uint32_t* q_len,
                                    const uint8_t* pool, const uint8_t* quals, uint64_t pool_bytes, ioc_pileup_col* cols,
                                    ioc_pileup_col* wcols, ioc_pileup_ins* wins, uint64_t n_rows);

// ioc_pile_call.hip: the consensus call (ioc_host_pileup_call) of many references from device tables (a segment: IocPileSeg,
// ioc_sink_plan.h)
hipError_t iock_pile_call(hipStream_t st, const IocPileSeg* segs, uint32_t n_segs, const ioc_pileup_col* cols, const ioc_pileup_ins* ins,
                          uint64_t n_rows, const uint8_t* frames, uint64_t frame_bytes, int32_t min_depth, int64_t* seg_len,
                          ioc_polish_stats* stats, int64_t* out_off, uint8_t* out_seq, uint8_t* out_qual, uint64_t out_bytes);

// ... by weight (ioc_host_pileup_call_weighted): cols gates, wcols / wins decide
hipError_t iock_pile_call_weighted(hipStream_t st, const IocPileSeg* segs, uint32_t n_segs, const ioc_pileup_col* cols, const ioc_pileup_col* wcols,
                                   const ioc_pileup_ins* wins, uint64_t n_rows, const uint8_t* frames, uint64_t frame_bytes, int32_t min_depth,
                                   int64_t* seg_len, ioc_polish_stats* stats, int64_t* out_off, uint8_t* out_seq, uint8_t* out_qual,
                                   uint64_t out_bytes);

// ... and the scan alone: out_off[0 .. n] (device) = the exclusive scan of len[0 .. n) (k_pile_scan, for the stages that count per item)
hipError_t iock_pile_scan(hipStream_t st, const int64_t* len, uint32_t n, int64_t* out_off);

// ioc_pile_sites.hip: the projection of the same strings into byte planes of the pairs' own (ioc_host_ops_project) — pair pid's
// base plane from base_planes + plane[pid] on, its ins plane from ins_planes + plane[pid] on (plane_bytes bytes each, set to
// IOC_ALLELE_NONE / 0 by the caller); launched beside iock_ops_pileup*, the same pairs are skipped
hipError_t iock_ops_project(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room,
                            const uint32_t* ord, uint32_t cnt, const int64_t* row_base, const uint32_t* q_off, const uint64_t* plane,
                            const uint8_t* pool, uint64_t pool_bytes, uint8_t* base_planes, uint8_t* ins_planes, uint64_t plane_bytes);
// ... the sites of many segments from a device table (ioc_host_pileup_sites per segment; of IocPileSeg row0 and rlen are read) ...
hipError_t iock_pile_sites(hipStream_t st, const IocPileSeg* segs, uint32_t n_segs, const ioc_pileup_col* cols, uint64_t n_rows, int32_t min_depth,
                           int32_t min_alt, int32_t min_pct, int32_t max_sites, int64_t* n_found, int64_t* seg_len, int64_t* site_off,
                           ioc_pile_site* out, uint64_t sites_cap);
// ... and every pair's alleles at the kept sites of its segment, from its planes (ioc_host_site_alleles)
hipError_t iock_site_alleles(hipStream_t st, uint32_t n_pairs, const int32_t* seg_of_pair, const IocPileSeg* segs, uint32_t n_segs,
                             const uint64_t* plane, const uint8_t* base_planes, const uint8_t* ins_planes, uint64_t plane_bytes,
                             const ioc_pile_site* sites, const int64_t* site_off, const int64_t* allele_off, uint8_t* alleles,
                             uint64_t alleles_cap);

// ioc_plane_pile.hip: what the same strings insert, into six byte planes of the pairs' own (ioc_host_ops_project_ins) — slot j of
// pair pid from slot_planes + j * plane_bytes + plane[pid] on (set to 0 by the caller); launched beside iock_ops_project
hipError_t iock_ops_project_ins(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room,
                                const uint32_t* ord, uint32_t cnt, const int64_t* row_base, const uint32_t* q_off, const uint64_t* plane,
                                const uint8_t* pool, uint64_t pool_bytes, uint8_t* slot_planes, uint64_t plane_bytes);
// ... and the tables of the two groups of every segment added up from the planes (ioc_host_planes_pile per member): everything is
// a device pointer; group-segment 2 g + h takes the pairs members[mem_off[g] .. mem_off[g + 1]) whose group byte is h
struct IocPlaneWork;  // (ioc_plane_pile.h: 64 rows of a group-segment)
hipError_t iock_plane_pile(hipStream_t st, const IocPlaneWork* work, uint32_t n_work, const IocPileSeg* gsegs, const uint32_t* mem_off,
                           const uint32_t* members, uint32_t n_pairs, const uint8_t* group, const uint64_t* plane, const uint8_t* base_planes,
                           const uint8_t* slot_planes, uint64_t plane_bytes, ioc_pileup_col* gcols, ioc_pileup_ins* gins, uint64_t n_rows);

// ioc_group_pile.hip: the tables of any number of groups of every segment added up from the same planes: everything is a device
// pointer; group-segment x (n_gsegs of them, in segment order) takes the pairs gmembers[gmem_off[x] .. gmem_off[x + 1]), its own
// list in ascending order (group_member_lists, ioc_sink_plan.h), n_members in all
struct IocGroupWork;  // (ioc_group_pile.h: 64 rows of a group-segment)
hipError_t iock_group_pile(hipStream_t st, const IocGroupWork* work, uint32_t n_work, const IocPileSeg* gsegs, uint32_t n_gsegs, const uint32_t* gmem_off,
                           const uint32_t* gmembers, uint32_t n_members, uint32_t n_pairs, const uint64_t* plane, const uint8_t* base_planes,
                           const uint8_t* slot_planes, uint64_t plane_bytes, ioc_pileup_col* gcols, ioc_pileup_ins* gins, uint64_t n_rows);

// ioc_group_pile_weighted.hip: the weight of every vote of the same strings into seven byte planes of the pairs' own
// (ioc_host_ops_project_weights) — [wbase plane][wslot-0 planes] .. [wslot-5 planes], plane_bytes each, pair pid's bytes from
// plane[pid] on of every one; quals: the pool's quality bytes (pool_bytes of them), q_len[pid]: the pair's query length —, and
// the three tables of any number of groups of every segment added up from the planes and the weight planes
// (ioc_host_planes_pile, ioc_host_planes_pile_weighted): the arguments of iock_group_pile, with gwcols / gwins beside gcols
hipError_t iock_ops_project_weights(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room, const uint32_t* ord,
                                    uint32_t cnt, const int64_t* row_base, const uint32_t* q_off, const uint32_t* q_len, const uint64_t* plane,
                                    const uint8_t* quals, uint64_t pool_bytes, uint8_t* weight_planes, uint64_t plane_bytes);
hipError_t iock_group_pile_weighted(hipStream_t st, const IocGroupWork* work, uint32_t n_work, const IocPileSeg* gsegs, uint32_t n_gsegs, const uint32_t* gmem_off,
                                    const uint32_t* gmembers, uint32_t n_members, uint32_t n_pairs, const uint64_t* plane, const uint8_t* base_planes,
                                    const uint8_t* slot_planes, const uint8_t* weight_planes, uint64_t plane_bytes, ioc_pileup_col* gcols,
                                    ioc_pileup_col* gwcols, ioc_pileup_ins* gwins, uint64_t n_rows);

// ioc_read_correct.hip: every pair's read corrected against the tables of its segment (ioc_host_read_correct per pair).  Everything
// is a device pointer: pair i belongs to segment seg_of_pair[i] and has its rows from byte plane[i] on of the base plane and of the
// six slot planes (plane_bytes each, one behind the other); pair_len / stats: n_pairs words of scratch and the records.  The count
// pass and the scan first; the write pass once out_seq / out_qual hold out_off[n_pairs] bytes.
struct IocReadCorrectDev {
    const IocPileSeg* segs;
    uint32_t n_segs, n_pairs;
    const int32_t* seg_of_pair;
    const uint64_t* plane;
    const ioc_pileup_col* cols;
    const ioc_pileup_ins* ins;
    uint64_t n_rows;
    const uint8_t* frames;
    uint64_t frame_bytes;
    const uint8_t *base_planes, *slot_planes;
    uint64_t plane_bytes;
    int64_t* pair_len;
    ioc_correct_stats* stats;
};
hipError_t iock_read_correct_count(hipStream_t st, const IocReadCorrectDev& v, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_run,
                                   int64_t* out_off);
hipError_t iock_read_correct_emit(hipStream_t st, const IocReadCorrectDev& v, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_run,
                                  const int64_t* out_off, uint8_t* out_seq, uint8_t* out_qual, uint64_t out_bytes);

// ioc_iso_correct.hip: every pair's read corrected against the tables of its own isoform, long insertions carried through
// (ioc_host_read_correct_long per pair).  Everything is a device pointer.  The tables are those of n_tables group-segments (gsegs:
// their rows, and the frame of their segment), the first n_group_tables a group's and the rest a whole segment's; pair i is held
// against group-segment table[i], has its rows from byte plane[i] on of the base plane, the six slot planes and the length plane
// (plane_bytes each) and from word plane[i] on of the position plane, and its read q_len[i] bytes from q_off[i] on of the pool.
// pair_len / stats: n_pairs words of scratch and the records.  The count pass and the scan first; the write pass once out_seq /
// out_qual hold out_off[n_pairs] bytes.
struct IocIsoCorrectDev {
    const IocPileSeg* gsegs;
    uint32_t n_tables, n_group_tables, n_pairs;
    const uint32_t* table;
    const uint64_t* plane;
    const ioc_pileup_col* cols;
    const ioc_pileup_ins* ins;
    uint64_t n_rows;
    const uint8_t* frames;
    uint64_t frame_bytes;
    const uint8_t *base_planes, *slot_planes, *ilen_planes;
    const uint32_t* qpos_planes;
    uint64_t plane_bytes;
    const uint8_t* pool;
    uint64_t pool_bytes;
    const uint64_t* q_off;
    const uint32_t* q_len;
    int64_t* pair_len;
    ioc_iso_correct_stats* stats;
};
hipError_t iock_iso_correct_count(hipStream_t st, const IocIsoCorrectDev& v, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_run,
                                  int64_t* out_off);
hipError_t iock_iso_correct_emit(hipStream_t st, const IocIsoCorrectDev& v, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_run,
                                 const int64_t* out_off, uint8_t* out_seq, uint8_t* out_qual, uint64_t out_bytes);

// ioc_read_blocks.hip: the exon blocks of many segments and every read's isoform (ioc_host_planes_blocks per segment).  Everything
// is a device pointer.  Pair i belongs to segment seg_of_pair[i], has its rows from byte plane[i] on of the base planes and its
// words — ceil((rlen + 1) / 64) of each bit plane (cov, del, gap: n_pair_words words each) — from word pair_word[i] on.  Segment g:
// the pairs members[mem_off[g] .. mem_off[g + 1]) in ascending order as its reads, its words of `var` from seg_word[g] on
// (n_seg_words in all; word_seg says whose each is), its rows of `rows` from segs[g].row0 on and its min(max_blocks, rlen) block
// slots from block_base[g] on (n_block_slots in all).  mask / flags: a word and a byte of scratch per pair.  reads and seg_out are
// set to 0 by the caller.
struct IocReadBlocksDev {
    const IocPileSeg* segs;
    uint32_t n_segs, n_pairs;
    const int32_t* seg_of_pair;
    const uint64_t* plane;
    const uint8_t* base_planes;
    uint64_t plane_bytes;
    const uint32_t *mem_off, *members;
    const uint64_t *pair_word, *seg_word;
    const int32_t* word_seg;
    const int64_t* block_base;
    uint64_t n_pair_words, n_seg_words, n_rows, n_block_slots;
    unsigned long long *cov, *del, *gap, *var, *mask;
    uint8_t* flags;
    ioc_block_row* rows;
    ioc_pile_block* blocks;
    ioc_read_blocks* reads;
    ioc_blocks_seg* seg_out;
};
hipError_t iock_read_blocks(hipStream_t st, const IocReadBlocksDev& v, int32_t min_gap, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                            int32_t min_block, int32_t max_blocks);

// ioc_read_inserts.hip: how many bases the same strings insert in front of every row, into one byte plane of the pairs' own
// (ioc_host_ops_project_ilen) — pair pid's from ilen_planes + plane[pid] on (set to 0 by the caller); launched beside iock_ops_project —
// and the insertion sites of many segments with every read's combined isoform (ioc_host_planes_inserts per segment).  Everything is
// a device pointer, laid out as for IocReadBlocksDev: the words of the bit planes span and near per pair, those of var per segment,
// min(max_sites, max(rlen - 1, 0)) site slots of segment g from site_base[g] on (n_site_slots in all; slot_seg says whose each is).
// pre_key / pre_mask: pair i's block word and its mask at word i * stride (NULL: 0), pre_full per segment (NULL: 0).  sites, reads
// and seg_out are set to 0 by the caller.
hipError_t iock_ops_project_ilen(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room, const uint32_t* ord,
                                 uint32_t cnt, const int64_t* row_base, const uint64_t* plane, uint8_t* ilen_planes, uint64_t plane_bytes);
struct IocReadInsertsDev {
    const IocPileSeg* segs;
    uint32_t n_segs, n_pairs;
    const int32_t* seg_of_pair;
    const uint64_t* plane;
    const uint8_t *base_planes, *ilen_planes;
    uint64_t plane_bytes;
    const uint32_t *mem_off, *members;
    const uint64_t *pair_word, *seg_word;
    const int32_t* word_seg;
    const int64_t* site_base;
    const int32_t* slot_seg;
    uint64_t n_pair_words, n_seg_words, n_rows, n_site_slots;
    const unsigned long long *pre_key, *pre_mask, *pre_full;
    uint32_t pre_key_stride, pre_mask_stride;
    unsigned long long *span, *near, *var, *mask;
    uint8_t* flags;
    uint16_t* wmax;  // scratch: a carrier's largest windowed sum at kept site k of its segment, at wmax[pair * wmax_stride + k]; n_wmax entries
    uint32_t wmax_stride;
    uint64_t n_wmax;
    ioc_insert_row* rows;
    ioc_pile_insert* sites;
    ioc_read_inserts* reads;
    ioc_inserts_seg* seg_out;
};
enum { IOC_READ_INSERTS_KERNELS = 8 };  // (each: IOC_READ_INSERTS_KERNELS + 1 events, or NULL)
hipError_t iock_read_inserts(hipStream_t st, const IocReadInsertsDev& v, int32_t min_ins, int32_t slack, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                             int32_t max_sites, hipEvent_t* each);

// ioc_insert_windows.hip: where every row of the same strings lies in the read, into one plane of 32-bit words of the pairs' own
// (ioc_host_ops_project_qpos) — pair pid's from word plane[pid] on of qpos_planes, plane_rows words in all (set to 0 by the caller);
// launched beside iock_ops_project — and the windows of the carriers at every kept insertion site (ioc_host_insert_windows per
// segment).  Everything is a device pointer.  Segment g has the sites site_off[g] .. site_off[g + 1] of `sites` (n_sites in all;
// site_seg says whose each is) and the pairs members[mem_off[g] .. mem_off[g + 1]); pair i has its read's length in qlen[i], its key
// in keys[i] and the entry of site k of its segment at slots[i * stride + k], n_slots entries in all.
hipError_t iock_ops_project_qpos(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room, const uint32_t* ord,
                                 uint32_t cnt, const int64_t* row_base, const uint64_t* plane, uint32_t* qpos_planes, uint64_t plane_rows);
struct IocWinSlot;
struct IocWinItem;
struct IocWinDev {
    const IocPileSeg* segs;
    uint32_t n_segs, n_pairs;
    const int32_t* seg_of_pair;
    const uint64_t* plane;
    const uint8_t* base_planes;
    const uint32_t* qpos_planes;
    uint64_t plane_rows;
    const uint32_t* qlen;
    const uint32_t *mem_off, *members;
    const ioc_pile_insert* sites;
    const int64_t* site_off;
    const int32_t* site_seg;
    uint32_t n_sites;
    const unsigned long long* keys;
    IocWinSlot* slots;
    uint32_t stride;
    uint64_t n_slots;
    ioc_insert_window* win;
};
// k_win_bounds and k_win_template over the view, in a row on `st`; `each` (3 events, or NULL) as for iock_read_inserts
hipError_t iock_win_bounds_template(hipStream_t st, const IocWinDev& v, int32_t slack, int32_t max_win, hipEvent_t* each);
// k_win_align over items[0 .. n_items): both strings in `pool`, the voters' planes (plane_bytes each: the base plane set to
// IOC_ALLELE_NONE, the six slot planes one behind the other set to 0 by the caller) and the direction words (n_dir_words of them
// from `dir` on, from which an item's offsets count).  phase: 0 both halves, 1 the fill alone, 2 the walk alone (over the words a
// fill left), for the measurement.
hipError_t iock_win_align(hipStream_t st, const IocWinItem* items, uint32_t n_items, const uint8_t* pool, uint64_t pool_bytes, uint8_t* base_planes,
                          uint8_t* slot_planes, uint64_t plane_bytes, uint32_t* dir, uint64_t n_dir_words, int32_t match, int32_t mismatch, int32_t gap,
                          int phase);

// ioc_window_variants.hip: two exons at one junction (ioc_host_insert_window_variants per segment) behind the window kernels.
// Everything is a device pointer.  `w` is the window stage's view as k_win_bounds and k_win_template left it; an entry is a (pair,
// site) place of its table, w.n_slots of them.  Round r (0: against template A, 1: against template B) leaves entry e's flag at
// flag[r * n_slots + e] (WINVAR_*, ioc_window_variants.h; set to 0 by the caller) and its agreement at agree[r * n_slots + e] (set
// to INT32_MIN by the caller); var: a record per site; variant: a byte per entry.
struct IocWinVarDev {
    IocWinDev w;
    uint8_t* flag;
    int32_t* agree;
    ioc_window_variant* var;
    uint8_t* variant;
};
struct WinVarRule;
// k_win_agree over the items of a round that k_win_align has run over: item x's entry is at[x]
hipError_t iock_win_agree(hipStream_t st, const IocWinItem* items, const uint64_t* at, uint32_t n_items, const uint8_t* pool, uint64_t pool_bytes,
                          const uint8_t* base_planes, uint64_t plane_bytes, int32_t* agree, uint8_t* flag, uint64_t n_entries, int32_t min_agree);
// k_win_template_far: n_far and template B of every site where round B runs, into var
hipError_t iock_win_template_far(hipStream_t st, const IocWinVarDev& v, const WinVarRule& rule);
// k_win_decide, k_win_rekey and the isoform count over key2 / mask2, in a row on `st`.  `k` is the view the key functions of
// ioc_read_stage.h read: n_segs, n_pairs, seg_of_pair, mem_off, members, pre_*, reads (key: key2, set to 0 by the caller), mask, flags;
// seg_out: a record per segment.  `each` (IOC_WIN_VARIANTS_KERNELS + 1 events, or NULL) as for iock_read_inserts.
enum { IOC_WIN_VARIANTS_KERNELS = 5 };
hipError_t iock_win_decide_rekey(hipStream_t st, const IocWinVarDev& v, const WinVarRule& rule, const IocReadInsertsDev& k, ioc_variants_seg* seg_out,
                                 hipEvent_t* each);

// ioc_iso_splice.hip: the full-length sequence of every isoform (ioc_host_isoform_splice per group-segment).  Everything is a device
// pointer.  Group-segment x (n_gsegs of them) is gsegs[x], belongs to segment gseg_seg[x] and carries keys[x]; segment g has the
// window records site_off[g] .. site_off[g + 1] of `win` (n_sites in all), site k's called bytes at win_off[k] .. win_off[k + 1] of
// wseq / wqual (win_bytes each).  Group-segment x's site records begin at splice[splice_off[x]] (n_splice in all), its plan at
// plan[x * IOC_SPLICE_PLAN_MAX] and holds plan_n[x] intervals.
struct IocSpliceIv;  // (ioc_iso_splice.h: the rows [lo, hi) and the window that replaces them)
struct IocSpliceDev {
    const IocPileSeg* gsegs;
    uint32_t n_gsegs;
    const int32_t* gseg_seg;
    const unsigned long long* keys;
    const ioc_insert_window* win;
    const long long *site_off, *win_off;
    uint64_t n_sites;
    const uint8_t *wseq, *wqual;
    uint64_t win_bytes;
    const long long* splice_off;
    ioc_splice_site* splice;
    uint64_t n_splice;
    ioc_splice_stats* sstats;
    IocSpliceIv* plan;
    uint32_t* plan_n;
    const ioc_window_variant* var;  // NULL, or the splice by variant: a record per site, keys are key2, and win_off / wseq / wqual /
                                    // win_bytes describe the variant stage's slots (2 n_sites + 1 offsets, slot 2 k + h of site k)
};
hipError_t iock_splice_plan(hipStream_t st, const IocSpliceDev& v);
// k_splice_call: the count pass (emit false: seg_len and stats, a word and a record per group-segment) or the write pass (emit true:
// the bytes from out_off[x] on, out_bytes of room each, and `at` of the DONE sites); iock_pile_scan goes between them
hipError_t iock_splice_call(hipStream_t st, const IocSpliceDev& v, bool emit, const ioc_pileup_col* cols, const ioc_pileup_ins* ins, uint64_t n_rows,
                            const uint8_t* frames, uint64_t frame_bytes, int32_t min_depth, int64_t* seg_len, ioc_polish_stats* stats, const int64_t* out_off,
                            uint8_t* out_seq, uint8_t* out_qual, uint64_t out_bytes);

// ioc_read_ends.hip: the alternative ends of many segments (ioc_host_reads_ends per segment).  Everything is a device pointer.
// Pair i belongs to segment seg_of_pair[i], has the extent extents[i] and pre_group[i * pre_stride] (pre_group NULL: 0).  Segment
// g: the pairs members[mem_off[g] .. mem_off[g + 1]) in ascending order as its reads, its rows of `hist` (and of `rows`, which may
// be NULL) from segs[g].row0 on, its ceil((rlen + 1) / 64) words of either bit plane from seg_word[g] on (n_seg_words in all;
// word_seg says whose each is), its min(max_sites, rlen + 1) start slots from site_base[2 g] on and as many stop slots from
// site_base[2 g + 1] on (n_site_slots in all; slot_unit says which 2 g + kind each belongs to) and its min(max_variants, reads)
// variant slots from var_base[g] on (n_var_slots in all).  hist (starts, stops a row), n_part (a word per segment), sites,
// variants and seg_out are set to 0 by the caller; key, same and flags are a word, a word and a byte of scratch per pair.
struct IocReadEndsDev {
    const IocPileSeg* segs;
    uint32_t n_segs, n_pairs;
    const int32_t* seg_of_pair;
    const ioc_read_extent* extents;
    const int32_t* pre_group;
    uint32_t pre_stride;
    const uint32_t *mem_off, *members;
    const uint64_t* seg_word;
    const int32_t* word_seg;
    const int64_t *site_base, *var_base;
    const int32_t* slot_unit;
    uint64_t n_seg_words, n_rows, n_site_slots, n_var_slots;
    uint2* hist;
    uint32_t* n_part;
    unsigned long long *bits_start, *bits_stop, *key;
    uint32_t* same;
    uint8_t* flags;
    ioc_end_row* rows;
    ioc_end_site* sites;
    ioc_end_variant* variants;
    ioc_read_ends* reads;
    ioc_ends_seg* seg_out;
};
enum { IOC_READ_ENDS_KERNELS = 8 };  // (each: IOC_READ_ENDS_KERNELS + 1 events, or NULL)
hipError_t iock_read_ends(hipStream_t st, const IocReadEndsDev& v, int32_t slack, int32_t min_over, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                          int32_t max_sites, int32_t max_variants, hipEvent_t* each);

// ioc_site_split.hip: the split of many segments' reads by their linked sites (ioc_host_alleles_split per segment).  Everything
// is a device pointer.  Segment g: the sites site_off[g] .. site_off[g + 1], the pairs members[mem_off[g] .. mem_off[g + 1]) in
// ascending order as its reads, word_off[g + 1] - word_off[g] = ceil(reads / 64) words a plane and site, its planes from word
// bit_off[g] on (words x sites of them each); tile_seg: the segment of every word of the call, seg_of_site that of every site.
struct IocSplitDev {
    uint32_t n_segs, n_pairs, n_tiles;
    uint64_t n_sites, allele_bytes, plane_words, max_seg_sites;
    const ioc_pile_site* sites;
    const long long* site_off;    // [n_segs + 1]
    const uint8_t* alleles;       // pair i's bytes from allele_off[i] on, one per site of its segment
    const long long* allele_off;  // [n_pairs + 1]
    const int32_t* seg_of_pair;
    const uint32_t *mem_off, *members, *word_off;  // [n_segs + 1], [n_pairs], [n_segs + 1]
    const long long* bit_off;                      // [n_segs + 1]
    const int32_t *tile_seg, *seg_of_site;         // [n_tiles], [n_sites]
    int2* marks;                                   // [n_sites] (minor, major)
    unsigned long long *bits_minor, *bits_major;   // [plane_words] each
    unsigned long long *g1, *g0;                   // [n_tiles] each
    long long* link;                               // [n_sites]
    int8_t* phase;                                 // [n_sites]
    int32_t* seed;                                 // [n_segs]
    uint8_t* group;                                // [n_pairs]
    int32_t* vote;                                 // [n_pairs]
    ioc_split_seg* rec;                            // [n_segs]
};
enum class IocSplitStep { marks, bits, link, seed, phase0, vote, group_bits, rephase, record };
hipError_t iock_site_split(hipStream_t st, const IocSplitDev& v, IocSplitStep step, int32_t min_link, int32_t min_margin);

// ioc_capi.cpp: queries whose minimizer arrays are already in HBM (ioc_batch_view::minimizers_on_device)
extern "C" int ioc_queries_upload_devmins(ioc_ctx* c, int32_t n, const int64_t* off_fwd, const int64_t* off_rev, const uint32_t* d_min_val,
                                          const uint32_t* d_min_pos, int64_t total, const uint32_t* hpc_len, const uint8_t* err_cell,
                                          const uint32_t* min_total);

// f(0) .. f(count - 1) on the host's cores (independent items only).  The workers are a pool that lives with the process
// (ioc_host.cpp): the consensus path comes here ~1000 times per batch, and starting 16 threads per call cost 0.4 s of it.
// A region entered while another one runs (another context on another thread, or a nested call) starts threads of its own.
void ioc_pool_run(size_t count, size_t nthreads, const std::function<void(size_t)>& f);
template <typename F>
static inline void ioc_parallel_for(size_t count, F f, size_t serial_below = 4)
{
    const size_t hw = std::thread::hardware_concurrency();
    const size_t nt = count < serial_below ? 1 : std::min<size_t>(count, std::max<size_t>(1, std::min<size_t>(16, hw)));
    if (nt <= 1) {
        for (size_t x = 0; x < count; ++x) f(x);
        return;
    }
    ioc_pool_run(count, nt, std::function<void(size_t)>(std::ref(f)));
}

#endif