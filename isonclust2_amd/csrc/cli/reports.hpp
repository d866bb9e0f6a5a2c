// The read reports of `dump` (--read-stats, --pileup, --polish, --sites, --split, --split-polish, --correct, --isoforms, --isoforms-polish, --isoforms-polish-weighted, --isoforms-inserts, --isoforms-ends, --isoforms-correct): every read of clusters.tsv
// aligned against its cluster's representative on the GPU, in groups of whole clusters.  report_plan.cpp cuts the groups and
// formats records (host only, checked by tools/cli_reports_check.cpp); reports.cpp aligns a group and writes its share of the files.
#ifndef ISONCLUST2_CLI_REPORTS_HPP
#define ISONCLUST2_CLI_REPORTS_HPP
#include <cstdint>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "cer.hpp"
#include "isonclust2_hip.h"

struct SitesOpt {
    bool on = false;
    int min_depth = 3, min_alt = 3, min_pct = 25, max_sites = 4096;
};
struct SplitOpt {
    bool on = false;
    int min_link = 3, min_margin = 1, rounds = 2;
    int polish_min_depth = 0;  // --split-polish: > 0, the depth below which a group's call keeps the representative's base
};
struct CorrectOpt {  // --correct: the thresholds of ioc_host_read_correct
    bool on = false;
    int min_depth = 3, min_alt = 3, min_pct = 25, max_run = 10;
};
struct IsoformsOpt {  // --isoforms: the thresholds of ioc_host_planes_blocks
    bool on = false;
    int min_gap = 20, min_depth = 3, min_alt = 3, min_pct = 25, min_block = 10, max_blocks = 32;
    int polish_min_depth = 0;  // --isoforms-polish: > 0, the depth below which an isoform's call keeps the representative's base, and ...
    int polish_max = 16;       // ... how many isoforms of a cluster are called
    bool polish_weighted = false;  // --isoforms-polish-weighted: every isoform is called by weight (ioc_align_pairs_blocks_polish_weighted)
    bool inserts = false;                            // --isoforms-inserts: the insertion sites as well (ioc_align_pairs_blocks_inserts), and ...
    int min_ins = 20, ins_slack = 8, ins_max = 32;   // ... the thresholds of ioc_host_planes_inserts the block search does not share
    bool inserts_seq = false;                        // --isoforms-inserts-seq: the consensus of the carriers' windows at every kept site as well
    int ins_max_win = IOC_WIN_MAX;                   // (ioc_align_pairs_blocks_inserts_seq), and the longest window that votes
    bool variants = false;                           // --isoforms-inserts-variants: two exons at one junction told apart as well
    int variants_min_agree = IOC_WINVAR_MIN_AGREE;   // (ioc_align_pairs_blocks_inserts_variants), and the agreement a voter is near a template at
    bool full = false;                               // --isoforms-full: every combined isoform's full-length sequence as well
    int full_max = 16;                               // (ioc_align_pairs_isoforms_full), and how many isoforms of a cluster are called
    bool full_variants = false;                      // --isoforms-full-variants: with the variants, the full-length sequence of every isoform counted
                                                     // again, each exon's own variant spliced in (ioc_align_pairs_isoforms_full_variants); full_max applies
    bool ends = false;                               // --isoforms-ends: the alternative ends as well (ioc_align_pairs_blocks_ends), and the
    bool correct = false;                            // --isoforms-correct: every read corrected against the tables of its own isoform as well
                                                     // (ioc_align_pairs_blocks_correct), under the thresholds of --correct-*
    int ends_slack = 10, ends_min_over = 20, ends_min_pct = 10, ends_max = 32, ends_max_variants = 64;  // thresholds of ioc_host_reads_ends the block search does not share
};
struct ReportOpts {
    bool stats = false;        // --read-stats
    bool pileup = false;       // --pileup
    int polish_min_depth = 0;  // --polish: > 0, the depth below which the call keeps the representative's base
    bool polish_weighted = false;
    SitesOpt sites;
    SplitOpt split;
    CorrectOpt correct;
    IsoformsOpt isoforms;
    bool polish() const { return polish_min_depth > 0; }
    bool group_polish() const { return split.on && split.polish_min_depth > 0; }
    bool iso_polish() const { return isoforms.on && isoforms.polish_min_depth > 0; }
    bool segs() const { return polish() || sites.on || split.on || correct.on || isoforms.on; }  // the calls that take the clusters as segments
    bool groups() const { return pileup || segs(); }                // something is written per group
    bool any() const { return stats || groups(); }
};

// a row of clusters.tsv: the read's id, sequence and quality lines where they lie in the sorted FASTQ's mapping
struct ReadStatRow {
    unsigned cls;
    int strand;
    const char* id;
    size_t id_len;
    const char* seq;
    size_t seq_len;
    const char* qual;
    size_t qual_len;
};

// the rows whose cluster has a record in cluster_cons.fq, in the order of clusters.tsv; row y of every per-read table is kept[y]
struct ReportRows {
    const std::vector<ReadStatRow>& all;
    std::vector<size_t> kept;
    std::vector<std::vector<size_t>> rows_of;  // per cluster: its rows y
    const ReadStatRow& row(size_t y) const { return all[kept[y]]; }
};
ReportRows keep_report_rows(const cer::Batch& b, const std::vector<ReadStatRow>& rows);

// everything one group of clusters sends to the device
struct ReportGroup {
    std::string pool, quals;  // the sequences side by side, and their quality lines in the same order
    std::vector<int64_t> offs, qoffs;
    std::vector<ioc_aln_pair> pairs;      // (e is set from the quality lines when the group is aligned)
    std::vector<size_t> pair_row;         // per pair: its row y
    std::vector<int32_t> pair_q, pair_rep_q;  // per pair: the quality lines of its read and of its representative (indices into qoffs)
    // the group's clusters in cluster order with the first of their rows in the group's table (-1: a cluster without a row of
    // clusters.tsv, all zeros) and their segment (-1 likewise); per pair its cluster's first row
    std::vector<std::pair<size_t, int64_t>> group_cls;
    std::vector<int32_t> group_seg;
    std::vector<int64_t> row_base;
    int64_t group_rows = 0;
    // one segment per cluster with rows, in the order of group_cls
    std::vector<ioc_polish_seg> segs;
    std::vector<int32_t> seg_of_pair, seg_reads;

    // the 256 MB rule: a cluster that needs `need` more bytes of pool opens the next group, unless this one is empty
    bool would_overflow(size_t need, size_t pool_max) const { return !pairs.empty() && pool.size() + need > pool_max; }
    void add_rowless_cluster(size_t ci);
    void add_cluster(const cer::Batch& b, size_t ci, const ReportRows& rows, const ReportOpts& opts);
    void clear();
};

constexpr size_t REPORT_POOL_MAX = size_t(256) << 20;
// Walks the clusters in order and calls emit(group) at every cut and at the end (then possibly with no pair at all).  A cluster
// is never divided; one without rows goes to the group that is open when it is met.
void plan_report_groups(const cer::Batch& b, const ReportRows& rows, const ReportOpts& opts, const std::function<void(ReportGroup&)>& emit,
                        size_t pool_max = REPORT_POOL_MAX);

// what the consensus calls may return at most, for all segments of a group (polish) or for both sides of them (groups = 2)
int64_t polish_capacity(const ReportGroup& g, int groups = 1);
// the sites the segments can have at most, and the allele bytes of all pairs at that
struct SiteCapacity {
    int64_t sites = 0, alleles = 0;
};
SiteCapacity site_capacity(const ReportGroup& g, int max_sites);

// what the correction of every read of a group may return at most: every pair's segment's bound
int64_t correct_capacity(const ReportGroup& g);
// ... and the correction by isoform, which carries long insertions through: that and every pair's read
int64_t iso_correct_capacity(const ReportGroup& g);

// the blocks a block search may keep at most, for all segments of a group: min(max_blocks, the representative's length) each
int64_t blocks_capacity(const ReportGroup& g, int max_blocks);
// what the consensus of the isoforms may return at most, for all segments of a group: a segment has at most as many isoforms as
// reads, so min(max_iso, its reads) of them (isoforms), each at most the consensus bound of its representative (bytes)
struct IsoCapacity {
    int64_t isoforms = 0, bytes = 0;
};
IsoCapacity iso_polish_capacity(const ReportGroup& g, int max_iso);
// ... and of ioc_align_pairs_isoforms_full and ioc_align_pairs_isoforms_full_variants (one slot a site is taken): an isoform holds at
// most its call's bound and a window of 7 max_win + 6 bytes a site
IsoCapacity iso_full_capacity(const ReportGroup& g, int max_iso, int max_sites, int max_win);
// the insertion sites a search may keep at most, for all segments of a group: min(max_sites, the junctions of the representative) each
int64_t inserts_capacity(const ReportGroup& g, int max_sites);
// A signature of insertion sites: one character per kept site from the key's two bits each — '=' lack (as the representative), '+'
// carry, '.' none —, "*" where the cluster has no site.
std::string inserts_signature(uint64_t key, int32_t n_sites);
// the rows of cluster_inserts.tsv of one cluster: "# cluster <id>: kept <n> of <found> sites" where the list was cut, then
// "<id> <first> <end> <carry> <lack> <none> <len_min> <len_max>" per kept site
std::string cluster_inserts_rows(size_t cluster, const ioc_inserts_seg& z, const ioc_pile_insert* sites);
// the columns of read_inserts.tsv behind the cluster and the read: "<signature> <combined isoform or .> <direct|assigned|rare|ambiguous>"
std::string read_insert_columns(const ioc_read_inserts& r, int32_t n_sites);
// ... of read_insert_variants.tsv: the signature with the variants told apart ('=' lack, 'A' / 'B' carry, '.' not across or unknown), and the columns behind it
std::string variants_signature(uint64_t key2, int32_t n_sites);
std::string read_variant_columns(const ioc_read_variants& r, int32_t n_sites);
// ... of a record of cluster_isoforms_full_variants.fq: " ins<b>/<A|B>@<at>+<len>" for every DONE site of an isoform, the letter being the
// state of key2 there — the record of cluster_insert_variants.fq that stands at base `at`
std::string full_variants_tail(uint64_t key2, const ioc_splice_site* sites, int64_t n_sites);
// the end sites (start and stop sites together) and the variants a search for ends may keep at most, for all segments of a group:
// 2 min(max_sites, the representative's length + 1) and min(max_variants, its reads) each
struct EndsCapacity {
    int64_t sites = 0, variants = 0;
};
EndsCapacity ends_capacity(const ReportGroup& g, int max_sites, int max_variants);
// the rows of cluster_ends.tsv of one cluster: "# cluster <id>: kept <n> of <found> start sites" (stop sites likewise) where a list
// was cut, then "<id> <start|stop> <index> <first> <end> <peak row> <peak reads> <reads> <over>" per kept site, the start sites first
std::string cluster_ends_rows(size_t cluster, const ioc_ends_seg& z, const ioc_end_site* starts, const ioc_end_site* stops);
// the rows of cluster_end_variants.tsv of one cluster: "# cluster <id>: kept <n> of <found> variants" where the list was cut, then
// "<id> <variant> <isoform> <start site> <stop site> <reads>" per kept variant
std::string cluster_end_variants_rows(size_t cluster, const ioc_ends_seg& z, const ioc_end_variant* variants);
// the columns of read_ends.tsv behind the read and the cluster: "<first row> <end row> <head> <tail> <start site or .> <stop site or .>
// <variant or .>"
std::string read_end_columns(const ioc_read_extent& e, const ioc_read_ends& r);
// A signature: one character per kept block from the key's two bits each — '=' keep, '-' skip, '~' part, '.' none —, "*" where the
// cluster has no block.
std::string blocks_signature(uint64_t key, int32_t n_blocks);
// the rows of cluster_blocks.tsv of one cluster: "# cluster <id>: kept <n> of <found> blocks" where the list was cut, then
// "<id> <block> <first> <end> <keep> <skip> <part> <none>" per kept block
std::string cluster_blocks_rows(size_t cluster, const ioc_blocks_seg& z, const ioc_pile_block* blocks);
// the rows of cluster_isoforms.tsv of one cluster, "<id> <isoform> <signature> <direct> <assigned>" per isoform, from the records
// of its reads (any order)
std::string cluster_isoforms_rows(size_t cluster, const ioc_blocks_seg& z, const std::vector<ioc_read_blocks>& reads);
// The records of cluster_isoforms.fq of one cluster: nothing for a cluster without a block; else one per called isoform h = 0 ..
// n_called - 1, "@cluster_<id>/iso<h> key=<signature as in cluster_isoforms.tsv> reads=<direct + assigned> subs= dels= ins= low=",
// the isoform's bytes seq / qual at [off[h], off[h + 1]) and its record stats[h]
std::string cluster_isoform_records(size_t cluster, const ioc_blocks_seg& z, const std::vector<ioc_read_blocks>& reads, int64_t n_called, const int64_t* off,
                                    const ioc_polish_stats* stats, const char* seq, const char* qual);
// the columns of read_isoforms.tsv behind the cluster and the read: "<isoform or .> <direct|assigned|rare|ambiguous> <signature>
// <first> <end> <gaps> <gap rows>"
std::string read_isoform_columns(const ioc_read_blocks& r, int32_t n_blocks);

char allele_char(int32_t kind, int32_t a);
// "@<name> reads= subs= dels= ins= low=<tail>", the sequence, "+", the qualities
std::string polish_record(const std::string& name, int32_t reads, const ioc_polish_stats& z, const char* tail, const char* seq, const char* qual, size_t len);
// A record of corrected_reads.fq: "@<id> cluster=<c> subs= fills= removes= ins_add= ins_drop= low= guarded=", then the read's own
// first lead_i bases with their own qualities, the corrected aligned part (cseq / cqual, clen bytes) and its last trail_i bases
// likewise, "+", the qualities.  read / qual: the read as it was aligned (as cluster_fastq/<id>.fq has it), read_len bases; a
// quality line of another length is cut or filled up with '!'.  An alignment whose longest insertion exceeds IOC_PILE_INS_SLOTS:
// the read as it is, " uncorrected=long_insertion" and counters of 0 (the planes hold six inserted bases a run: the correction
// would cut it).
std::string corrected_record(const char* id, size_t id_len, unsigned cls, const char* read, size_t read_len, const char* qual, size_t qual_len,
                             const ioc_aln_stats& a, const ioc_correct_stats& z, const char* cseq, const char* cqual, size_t clen);

// A record of corrected_reads_isoforms.fq: corrected_record's layout with " isoform=<h or -> table=<isoform|cluster> long_runs=
// long_bases=" behind its counters; a long insertion is carried through, so no read is left as it is for one.  An unresolved pair
// (IOC_ISOC_UNRESOLVED): the read as it is, " uncorrected=unresolved_insertion" and counters of 0.
std::string iso_corrected_record(const char* id, size_t id_len, unsigned cls, const char* read, size_t read_len, const char* qual, size_t qual_len,
                                 const ioc_aln_stats& a, const ioc_iso_correct_stats& z, int32_t isoform, const char* cseq, const char* cqual, size_t clen);

void write_read_reports(const cer::Batch& b, const std::string& outdir, const std::vector<ReadStatRow>& rows, const ReportOpts& opts);

#endif
