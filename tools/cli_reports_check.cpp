// cli_reports_check.cpp — how `dump` cuts its clusters into groups for the read reports (isonclust2_amd/csrc/cli/report_plan.cpp),
// on a batch built in memory: a cluster whose representative has a negative score (its rows do not count), a cluster without
// rows, a cluster whose representative is on strand -1 with reads of both strands, and three further clusters.
//
//  1. With the default cap there is one group; its pool (with the reverse complements), its quality lines (reversed with their
//     reads), both offset tables, every pair's query, reference and rc flag, row_base, seg_of_pair, seg_reads, group_cls and
//     group_seg are compared with values written out by hand, and so are the capacity sums of the consensus and site calls.
//  2. With the cap lowered to every value from the smallest cluster's need to the total, the cuts are exactly where a plain loop
//     over the needs puts them (pool + need > cap with a non-empty pool): no cluster is divided, a cluster without rows goes to
//     the group that is open when it is met, and the groups' pairs one after the other are the pairs of the one-group plan.
//  3. polish_record and allele_char on one hand-made input each; corrected_record with both clipped ends attached, with a short
//     quality line, with clips that exceed the read, and with an alignment whose insertion is too long to correct; the rows of
//     --isoforms: a signature of every state and of no block, a cut list's '#' line, the isoforms counted from the reads' records, the records of
//     --isoforms-polish and what they may take.
//
// Host code only (the planner does not touch the library, so neither common.cpp nor the library is linked); meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc/cli \
//       -o /tmp/cli_reports_check tools/cli_reports_check.cpp isonclust2_amd/csrc/cli/report_plan.cpp isonclust2_amd/csrc/cli/cer.cpp \
//       && /tmp/cli_reports_check
//
// Exit status 0 and "ok" when everything agrees.
#include <cstdio>
#include <string>
#include <tuple>
#include <vector>

#include "reports.hpp"

using namespace cer;
using std::string;

namespace {

int faults = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            ++faults;                                                  \
        }                                                              \
    } while (0)

std::shared_ptr<Cluster> cluster_of(const char* seq, const char* qual, double score, int strand)
{
    auto cl = std::make_shared<Cluster>();
    auto rep = std::make_shared<ProcSeq>();
    rep->RawSeq.reset(new Seq{"rep", seq, qual, score, 0.01});
    rep->MatchStrand = strand;
    cl->push_back(rep);
    return cl;
}

struct Read {
    unsigned cls;
    int strand;
    string id, seq, qual;
};

// a pair as the strings it stands for: its row, the query and the reference as the pool has them, the rc flag
typedef std::tuple<size_t, string, string, int32_t> PairText;
std::vector<PairText> pair_texts(const ReportGroup& g)
{
    std::vector<PairText> out;
    auto piece = [&](int32_t s) { return g.pool.substr(size_t(g.offs[size_t(s)]), size_t(g.offs[size_t(s) + 1] - g.offs[size_t(s)])); };
    for (size_t x = 0; x < g.pairs.size(); ++x) out.emplace_back(g.pair_row[x], piece(g.pairs[x].query), piece(g.pairs[x].ref), g.pairs[x].ref_revcomp);
    return out;
}

template <class T>
bool same(const std::vector<T>& got, std::initializer_list<T> want)
{
    return got == std::vector<T>(want);
}

}  // namespace

int main()
{
    Batch b;
    b.Cls = {cluster_of("AAAA", "HHHH", -1.0, 1),      cluster_of("ACGTAC", "IIIIII", 9.0, 1), cluster_of("TTTT", "MMMM", 8.0, 1),
             cluster_of("TTGCA", "JJJJJ", 7.0, -1),    cluster_of("CCCC", "KKK", 6.0, 1),      cluster_of("GGGGGGG", "LLLLLLL", 5.0, 1)};
    // the rows of clusters.tsv, in the order of the sorted FASTQ: clusters interleaved, one row of the unusable cluster 0 and one
    // of a cluster the batch does not have
    const std::vector<Read> reads = {{3, 1, "r3a", "TGCAA", "abcde"}, {0, 1, "r0", "AAA", "hhh"},    {1, 1, "r1a", "ACGTA", "ABCDE"}, {5, -1, "r5", "GGGG", "opqr"},
                                     {1, -1, "r1b", "GGTAC", "12345"}, {4, 1, "r4", "CCC", "lmn"},    {3, -1, "r3b", "AACN", "wxyz"},  {99, 1, "r9", "ACGT", "IIII"}};
    std::vector<ReadStatRow> all;
    for (const Read& r : reads) all.push_back(ReadStatRow{r.cls, r.strand, r.id.data(), r.id.size(), r.seq.data(), r.seq.size(), r.qual.data(), r.qual.size()});
    const ReportRows rows = keep_report_rows(b, all);
    EXPECT(same<size_t>(rows.kept, {0, 2, 3, 4, 5, 6}));
    EXPECT(rows.rows_of[0].empty() && rows.rows_of[2].empty());
    EXPECT(same<size_t>(rows.rows_of[1], {1, 3}) && same<size_t>(rows.rows_of[3], {0, 5}) && same<size_t>(rows.rows_of[4], {4}) && same<size_t>(rows.rows_of[5], {2}));

    ReportOpts opts;
    opts.stats = opts.pileup = opts.sites.on = opts.split.on = true;
    opts.polish_min_depth = opts.split.polish_min_depth = 3;

    // ---- 1. one group, against values written out by hand ----
    std::vector<ReportGroup> one;
    plan_report_groups(b, rows, opts, [&](ReportGroup& g) { one.push_back(g); });
    EXPECT(one.size() == 1);
    const ReportGroup& g = one[0];
    //              c1: rep   r1a    rc(r1b)   c3: rep  r3a    rc(r3b)  c4: rep r4   c5: rep     rc(r5)
    EXPECT(g.pool == "ACGTAC" "ACGTA" "GTACC"     "TTGCA" "TGCAA" "NGTT"    "CCCC" "CCC"   "GGGGGGG" "CCCC");
    EXPECT(g.quals == "IIIIII" "ABCDE" "54321"    "JJJJJ" "abcde" "zyxw"    "KKK" "lmn"    "LLLLLLL" "rqpo");
    EXPECT(same<int64_t>(g.offs, {0, 6, 11, 16, 21, 26, 30, 34, 37, 44, 48}));
    EXPECT(same<int64_t>(g.qoffs, {0, 6, 11, 16, 21, 26, 30, 33, 36, 43, 47}));
    const int32_t want_pairs[6][3] = {{1, 0, 0}, {2, 0, 0}, {4, 3, 1}, {5, 3, 1}, {7, 6, 0}, {9, 8, 0}};
    EXPECT(g.pairs.size() == 6);
    for (size_t x = 0; x < g.pairs.size() && x < 6; ++x)
        EXPECT(g.pairs[x].query == want_pairs[x][0] && g.pairs[x].ref == want_pairs[x][1] && g.pairs[x].ref_revcomp == want_pairs[x][2] && g.pairs[x].reserved == 0 &&
               g.pairs[x].e == 0.0);
    EXPECT(same<size_t>(g.pair_row, {1, 3, 0, 5, 4, 2}));
    EXPECT(same<int32_t>(g.pair_q, {1, 2, 4, 5, 7, 9}) && same<int32_t>(g.pair_rep_q, {0, 0, 3, 3, 6, 8}));
    EXPECT(same<int64_t>(g.row_base, {0, 0, 7, 7, 13, 18}) && g.group_rows == 26);
    EXPECT(same<int32_t>(g.seg_of_pair, {0, 0, 1, 1, 2, 3}) && same<int32_t>(g.seg_reads, {2, 2, 1, 1}));
    EXPECT((g.group_cls == std::vector<std::pair<size_t, int64_t>>{{1, 0}, {2, -1}, {3, 7}, {4, 13}, {5, 18}}));
    EXPECT(same<int32_t>(g.group_seg, {0, -1, 1, 2, 3}));
    const int32_t want_segs[4][2] = {{0, 0}, {3, 1}, {6, 0}, {8, 0}};
    EXPECT(g.segs.size() == 4);
    for (size_t s = 0; s < g.segs.size() && s < 4; ++s) EXPECT(g.segs[s].ref == want_segs[s][0] && g.segs[s].ref_revcomp == want_segs[s][1]);
    // rlen + IOC_PILE_INS_SLOTS * (rlen + 1) for 6, 5, 4, 7 bases: 48 + 41 + 34 + 55
    EXPECT(polish_capacity(g) == 178 && polish_capacity(g, 2) == 356);
    // min(10, 2 * rlen + 1) = 10, 10, 9, 10 sites; times 2, 2, 1, 1 reads
    EXPECT(site_capacity(g, 10).sites == 39 && site_capacity(g, 10).alleles == 59);
    // min(max_iso, reads) = 2, 2, 1, 1 isoforms at 16 and 1 each at 1; times the bounds above
    EXPECT(iso_polish_capacity(g, 16).isoforms == 6 && iso_polish_capacity(g, 16).bytes == 2 * 48 + 2 * 41 + 34 + 55);
    EXPECT(iso_polish_capacity(g, 1).isoforms == 4 && iso_polish_capacity(g, 1).bytes == 178);
    // the correction by isoform: every pair's segment's bound and its own read beside it
    int64_t reads_bytes = 0;
    for (const ioc_aln_pair& pr : g.pairs) reads_bytes += g.offs[size_t(pr.query) + 1] - g.offs[size_t(pr.query)];
    EXPECT(reads_bytes > 0 && iso_correct_capacity(g) == correct_capacity(g) + reads_bytes);
    // without a per-group file nothing but the pool, the pairs and their maps is kept
    {
        ReportOpts stats_only;
        stats_only.stats = true;
        std::vector<ReportGroup> plain;
        plan_report_groups(b, rows, stats_only, [&](ReportGroup& x) { plain.push_back(x); });
        EXPECT(plain.size() == 1 && plain[0].pool == g.pool && plain[0].pair_row == g.pair_row && plain[0].group_cls.empty() && plain[0].segs.empty() &&
               plain[0].row_base.empty() && plain[0].group_seg.empty());
    }

    // ---- 2. every cap from the smallest need to the total ----
    const std::vector<std::pair<size_t, size_t>> need = {{1, 16}, {3, 14}, {4, 7}, {5, 11}};  // cluster, rep + reads
    const std::vector<PairText> all_pairs = pair_texts(g);
    for (size_t cap = 7; cap <= 48; ++cap) {
        // a plain loop over the needs: which clusters each group must hold, the one without rows (2) where it is met
        std::vector<std::vector<size_t>> want(1);
        size_t fill = 0;
        for (const auto& nd : need) {
            if (nd.first == 3) want.back().push_back(2);
            if (fill > 0 && fill + nd.second > cap) want.emplace_back(), fill = 0;
            want.back().push_back(nd.first);
            fill += nd.second;
        }
        std::vector<std::vector<size_t>> got;
        std::vector<PairText> got_pairs;
        plan_report_groups(b, rows, opts, [&](ReportGroup& x) {
            got.emplace_back();
            for (const auto& gc : x.group_cls) got.back().push_back(gc.first);
            for (const PairText& p : pair_texts(x)) got_pairs.push_back(p);
            size_t reads_in = 0;
            for (int32_t n : x.seg_reads) reads_in += size_t(n);
            EXPECT(reads_in == x.pairs.size() && x.group_cls.size() == x.group_seg.size() && x.offs.size() == x.qoffs.size());  // whole clusters only
            EXPECT(x.segs.size() <= 1 || x.pool.size() <= cap);  // (a single cluster may exceed the cap: it cannot be divided)
        }, cap);
        EXPECT(got == want);
        EXPECT(got_pairs == all_pairs);
    }

    // ---- 3. the record format and the allele characters ----
    ioc_polish_stats z{};
    z.n_sub = 1, z.n_del = 2, z.n_ins = 3, z.n_low = 4;
    EXPECT(polish_record("cluster_7/1", 3, z, " weighted=1", "ACGTAC", "IIII!!", 4) == "@cluster_7/1 reads=3 subs=1 dels=2 ins=3 low=4 weighted=1\nACGT\n+\nIIII\n");
    string chars;
    for (int32_t a = -1; a <= 6; ++a) chars += allele_char(0, a);
    for (int32_t a = -1; a <= 2; ++a) chars += allele_char(IOC_SITE_INS, a);
    EXPECT(chars == "?ACGTN-?" "?.+?");

    // a read of 10 bases whose alignment leaves 2 free in front and 3 behind: its 5 aligned bases became "ACGTTT"
    ioc_aln_stats a{};
    a.lead_i = 2, a.trail_i = 3, a.longest_ins = IOC_PILE_INS_SLOTS;
    ioc_correct_stats k{};
    k.out_len = 6, k.n_sub = 1, k.n_fill = 2, k.n_remove = 3, k.n_ins_add = 4, k.n_ins_drop = 5, k.n_low = 6, k.n_guarded = 7;
    const char* const head = "@r1 cluster=4 subs=1 fills=2 removes=3 ins_add=4 ins_drop=5 low=6 guarded=7\n";
    EXPECT(corrected_record("r1 x", 2, 4, "ggCCCCCttt", 10, "0123456789", 10, a, k, "ACGTTT", "IIIII!", 6) == string(head) + "ggACGTTTttt\n+\n01IIIII!789\n");
    EXPECT(corrected_record("r1", 2, 4, "ggCCCCCttt", 10, "0123", 4, a, k, "ACGTTT", "IIIII!", 6) == string(head) + "ggACGTTTttt\n+\n01IIIII!!!!\n");
    a.lead_i = 8, a.trail_i = 5;  // (clips that do not fit the read: the trailing one gives way)
    EXPECT(corrected_record("r1", 2, 4, "ggCCCCCttt", 10, "0123456789", 10, a, k, "", "", 0) == string(head) + "ggCCCCCttt\n+\n0123456789\n");
    a.lead_i = 2, a.trail_i = 3, a.longest_ins = IOC_PILE_INS_SLOTS + 1;
    EXPECT(corrected_record("r1", 2, 4, "ggCCCCCttt", 10, "0123456789", 10, a, k, "ACGTTT", "IIIII!", 6) ==
           "@r1 cluster=4 subs=0 fills=0 removes=0 ins_add=0 ins_drop=0 low=0 guarded=0 uncorrected=long_insertion\nggCCCCCttt\n+\n0123456789\n");

    // the record of the correction by isoform: corrected_record's layout with four more fields; a long insertion is no reason to
    // leave the read as it is, an unresolved pair is (the library hands back counters of 0 for it)
    ioc_iso_correct_stats zc{6, 1, 2, 3, 4, 5, 6, 7, 3, 1, 40, 0};
    const char* const ihead = "@r1 cluster=4 subs=1 fills=2 removes=3 ins_add=4 ins_drop=5 low=6 guarded=7 isoform=1 table=isoform long_runs=1 long_bases=40\n";
    EXPECT(iso_corrected_record("r1 x", 2, 4, "ggCCCCCttt", 10, "0123456789", 10, a, zc, 1, "ACGTTT", "IIIII!", 6) == string(ihead) + "ggACGTTTttt\n+\n01IIIII!789\n");
    EXPECT(iso_corrected_record("r1", 2, 4, "ggCCCCCttt", 10, "0123", 4, a, zc, 1, "ACGTTT", "IIIII!", 6) == string(ihead) + "ggACGTTTttt\n+\n01IIIII!!!!\n");
    zc.table = -1 - 2;
    EXPECT(iso_corrected_record("r1", 2, 4, "ggCCCCCttt", 10, "0123456789", 10, a, zc, -1, "ACGTTT", "IIIII!", 6).find(" isoform=- table=cluster long_runs=1 ") != string::npos);
    a.lead_i = 8, a.trail_i = 5;  // (clips that do not fit the read: the trailing one gives way)
    const string clipped = iso_corrected_record("r1", 2, 4, "ggCCCCCttt", 10, "0123456789", 10, a, zc, -1, "", "", 0), whole = "\nggCCCCCttt\n+\n0123456789\n";
    EXPECT(clipped.size() > whole.size() && clipped.substr(clipped.size() - whole.size()) == whole);
    a.lead_i = 2, a.trail_i = 3;
    ioc_iso_correct_stats zu{};
    zu.table = 0, zu.flags = IOC_ISOC_UNRESOLVED;
    EXPECT(iso_corrected_record("r1", 2, 4, "ggCCCCCttt", 10, "0123", 4, a, zu, 0, "", "", 0) ==
           "@r1 cluster=4 subs=0 fills=0 removes=0 ins_add=0 ins_drop=0 low=0 guarded=0 isoform=0 table=isoform long_runs=0 long_bases=0 uncorrected=unresolved_insertion\n"
           "ggCCCCCttt\n+\n0123!!!!!!\n");

    // three kept blocks of four found; the states keep, skip, part at blocks 0 .. 2 make the key 0 + (1 << 2) + (2 << 4)
    EXPECT(blocks_signature(0x24, 3) == "=-~" && blocks_signature(0x3, 1) == "." && blocks_signature(7, 0) == "*" && blocks_signature(~0ull, 32) == string(32, '.'));
    const ioc_blocks_seg zs{3, 4, 2, 5, 3, 1, 0, 1};
    const ioc_pile_block kept[3] = {{10, 50, 3, 2, 0, 0, {0, 0}}, {100, 220, 2, 2, 1, 0, {0, 0}}, {300, 310, 1, 2, 1, 1, {0, 0}}};
    EXPECT(cluster_blocks_rows(9, zs, kept) == "# cluster 9: kept 3 of 4 blocks\n9\t0\t10\t50\t3\t2\t0\t0\n9\t1\t100\t220\t2\t2\t1\t0\n9\t2\t300\t310\t1\t2\t1\t1\n");
    EXPECT(cluster_blocks_rows(9, ioc_blocks_seg{0, 0, 1, 5, 5, 0, 0, 0}, nullptr).empty());
    const std::vector<ioc_read_blocks> recs = {{0x24, 1, IOC_ISO_DIRECT, 0, 400, 1, 40}, {0x0, 0, IOC_ISO_DIRECT, 0, 400, 0, 0}, {0x34, 1, IOC_ISO_ASSIGNED, 0, 290, 1, 40},
                                               {0x24, 1, IOC_ISO_DIRECT, 2, 399, 1, 41}, {0x15, -1, IOC_ISO_RARE, 0, 400, 3, 170}};
    EXPECT(cluster_isoforms_rows(9, zs, recs) == "9\t0\t===\t1\t0\n9\t1\t=-~\t2\t1\n");
    EXPECT(read_isoform_columns(recs[2], 3) == "1\tassigned\t=-.\t0\t290\t1\t40" && read_isoform_columns(recs[4], 3) == ".\trare\t---\t0\t400\t3\t170");
    // the records of cluster_isoforms.fq: both isoforms, the first alone (--isoforms-polish-max 1), and none for a cluster without a block
    const int64_t ioff[3] = {4, 8, 10};
    ioc_polish_stats zi[2] = {};
    zi[1].n_del = 2, zi[1].n_low = 1;
    const string both = "@cluster_9/iso0 key==== reads=1 subs=0 dels=0 ins=0 low=0\nACGT\n+\nIIII\n@cluster_9/iso1 key==-~ reads=3 subs=0 dels=2 ins=0 low=1\nTT\n+\n!J\n";
    EXPECT(cluster_isoform_records(9, zs, recs, 2, ioff, zi, "....ACGTTT", "....IIII!J") == both);
    EXPECT(cluster_isoform_records(9, zs, recs, 1, ioff, zi, "....ACGTTT", "....IIII!J") == both.substr(0, both.find("@cluster_9/iso1")));
    EXPECT(cluster_isoform_records(9, ioc_blocks_seg{0, 0, 1, 5, 5, 0, 0, 0}, recs, 1, ioff, zi, "....ACGTTT", "....IIII!J").empty());
    ioc_read_blocks amb{};
    amb.group = -1, amb.how = IOC_ISO_AMBIGUOUS;
    EXPECT(read_isoform_columns(amb, 0) == ".\tambiguous\t*\t0\t0\t0\t0" && read_isoform_columns(recs[1], 3) == "0\tdirect\t===\t0\t400\t0\t0");

    if (faults) {
        fprintf(stderr, "%d checks failed\n", faults);
        return 1;
    }
    printf("ok\n");
    return 0;
}
