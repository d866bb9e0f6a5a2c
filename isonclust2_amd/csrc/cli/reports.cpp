// dump --read-stats: <outdir>/read_stats.tsv, one row per row of clusters.tsv whose cluster has a record in cluster_cons.fq.  The
// read as cluster_fastq/<id>.fq has it (reverse-complemented when its strand is -1) is aligned against the representative as
// cluster_cons.fq has it, e = CalcErrorRate of the two quality lines as those files have them, k the batch's k-mer size, scores
// 2 / -2 / extend 1 as the cluster drivers use — so the files `dump` writes determine the report.  The alignments are reduced to
// their statistics on the device (ioc_align_pairs_stats), in groups of whole clusters whose sequence pool stays under 256 MB.
//
// dump --pileup: <outdir>/cluster_pileup.tsv from the same pairs in the same groups, piled on the device onto their cluster's
// representative (ioc_align_pairs_pileup): for every cluster with a record in cluster_cons.fq, in cluster order, one row per
// position of the representative as that file has it — how many reads cover the base, what they say there, how many have an
// insertion in front of it — and a last row (RepBase '-') for the insertions behind the last base.  With both options a group
// is aligned once: the pileup call returns the statistics of the same alignments.
//
// dump --polish: <outdir>/cluster_polished.fq from the same pairs, groups and frames — one record per record of cluster_cons.fq, in
// its order and frame: the majority call over the cluster's reads (ioc_align_pairs_polish: both pileup tables and the call on the
// device, only the sequences come back), header "@cluster_<id> reads=<pairs> subs= dels= ins= low=".  A cluster without a row of
// clusters.tsv keeps its representative, with '!' qualities.  Beside the other options a group is still aligned once: the
// polish call returns the statistics and the first table as well.
//
// dump --polish --polish-weighted: the same records, order and frames, called by weight (ioc_align_pairs_polish_weighted): every
// read votes with the base qualities of its line as cluster_fastq/<id>.fq has it (reversed with the read when its strand is
// -1), the pool's qualities being the lines e is computed from already.  The header gains a last field " weighted=1".
//
// dump --sites: <outdir>/cluster_sites.tsv and <outdir>/read_alleles.tsv from the same pairs, groups and frames
// (ioc_align_pairs_alleles: the table, every read's projection, the sites and the alleles on the device; one byte per read and
// site comes back).  cluster_sites.tsv: for every cluster in cluster order one row per variable site of its representative —
// position, kind (base | ins: an insertion in front of the position), depth, and the two alleles with their counts, written
// A C G T N - at a base site, '.' (absent) and '+' (present) at an insertion site; a cluster cut at --sites-max gets a line
// "# cluster X: kept K of F sites".  read_alleles.tsv: one row per row read_stats.tsv has, the read's allele at every kept site
// of its cluster as one character, '?' where the read does not cover the site, "*" for a cluster without sites.  Beside
// --read-stats and --pileup a group is still aligned once: the call returns the statistics and the table as well.  With
// --polish a group is aligned a second time, for the second table.
//
// dump --split: <outdir>/cluster_split.tsv and <outdir>/read_split.tsv (ioc_align_pairs_split: the call of --sites with the reads
// of every cluster split in two by its linked sites where the alleles lie; the thresholds of the site search are the --sites-*
// ones, whether --sites is given or not).  cluster_split.tsv: one row per cluster in cluster order — how many sites it kept, how
// many of them ended up linked, the seed site's position and kind ("." for a cluster without a split), its reads and how many
// of them are in group 0, in group 1 and in neither.  read_split.tsv: one row per row read_stats.tsv has — the read's group
// (0 | 1 | .) and its vote.  Whether a split is real is the reader's judgement of those counts.  Beside --sites, --read-stats and
// --pileup a group is still aligned once.
//
// dump --split --split-polish: <outdir>/cluster_split_polished.fq (ioc_align_pairs_split_polish: the call of --split with the
// consensus of both groups of every cluster called on the device from the reads' planes, no read aligned a second time).  For
// every cluster that has a split (a seed site), in cluster order, one record per group that has reads, group 0 before group 1,
// named after the cluster's record in cluster_cons.fq with "/0" or "/1" appended: "@cluster_<id>/<group> reads=<the group's reads>
// subs= dels= ins= low=", in the frame of that record; positions covered by fewer than --split-polish-min-depth reads of the
// group keep the representative's base with quality '!'.  The other report files are what they are without the option.
//
// dump --correct: <outdir>/corrected_reads.fq (ioc_align_pairs_correct: the alignment and both tables of --polish with every read
// projected beside them, and every read corrected against its cluster's pileup where all of that lies; a call of its own, which
// takes the statistics and the first table when no call before it has).  One record per row read_stats.tsv has, in that order: the
// read as cluster_fastq/<id>.fq has it with its aligned part corrected, the ends the alignment leaves free as they are (corrected_record,
// report_plan.cpp); a read whose alignment inserts more than six bases in a row is written as it is and marked.  The other report
// files are what they are without the option.
//
// dump --isoforms: <outdir>/cluster_blocks.tsv, cluster_isoforms.tsv and read_isoforms.tsv (ioc_align_pairs_blocks: the alignment, the
// table of counts and every read's base plane of --sites, and the block search over the planes where they lie; a call of its own,
// which takes the statistics and the first table when no call before it has).  cluster_blocks.tsv: the stretches of a cluster's
// representative that some of its reads skip, with how many reads keep, skip, half-skip or do not reach each; cluster_isoforms.tsv:
// the signatures that enough reads carry; read_isoforms.tsv: one row per row read_stats.tsv has, in that order (report_plan.cpp
// formats all three).  The other report files are what they are without the option.
//
// dump --isoforms --isoforms-polish: <outdir>/cluster_isoforms.fq (ioc_align_pairs_blocks_polish: the call of --isoforms with the
// consensus of every isoform called on the device from the reads' planes, no read aligned a second time).  For every cluster
// with at least one block, in cluster order, one record per called isoform in ascending order — the first
// --isoforms-polish-max of them —, named after the cluster's record in cluster_cons.fq with "/iso<h>" appended:
// "@cluster_<id>/iso<h> key=<signature as in cluster_isoforms.tsv> reads=<its direct and assigned reads> subs= dels= ins= low=", in
// the frame of that record; positions covered by fewer than --isoforms-polish-min-depth reads of the isoform keep the
// representative's base with quality '!'.  The other report files are what they are without the option.
//
// dump --isoforms --isoforms-correct: <outdir>/corrected_reads_isoforms.fq (ioc_align_pairs_blocks_correct: the call of --isoforms with
// the slot, length and position planes projected beside it and every read corrected against the tables of its own isoform — its
// cluster's where its isoform has fewer than --correct-min-depth reads or it has none —, a long insertion carried through as the
// read has it): one record per row of clusters.tsv, in that order (iso_corrected_record, report_plan.cpp).
// dump --isoforms --isoforms-polish --isoforms-polish-weighted: the same records of cluster_isoforms.fq, names and order, every
// isoform called by weight (ioc_align_pairs_blocks_polish_weighted: the weight of every vote kept beside the reads' planes, still
// no read aligned a second time): every read votes with the base qualities of its line as --polish-weighted has them.  Where
// an isoform has 5 to 12 reads this is what keeps three low-quality reads from outvoting two good ones.  The other report files
// are what they are without the option.
//
// dump --isoforms --isoforms-inserts: <outdir>/cluster_inserts.tsv and read_inserts.tsv (ioc_align_pairs_blocks_inserts: the call of
// --isoforms with every read's length plane kept beside its base plane and the search for insertion sites behind the block search,
// no read aligned a second time): cluster_inserts.tsv: the places where some reads of a cluster carry an exon its representative
// lacks, with how many reads carry it, lack it or do not reach across and the carriers' shortest and longest insertion;
// read_inserts.tsv: one row per row read_stats.tsv has, in that order, with the read's signature at the sites and its isoform over
// blocks and sites together.  The three files of --isoforms and the other report files are what they are without the option.
//
// dump --isoforms --isoforms-ends: <outdir>/cluster_ends.tsv, cluster_end_variants.tsv and read_ends.tsv (ioc_align_pairs_blocks_ends: the
// call of --isoforms with the search for ends behind the block search, no read aligned a second time): cluster_ends.tsv: where the
// reads of a cluster start and stop on its representative, with the row most of them use, how many reads use the site and how many
// of those go on beyond the representative there; cluster_end_variants.tsv: the (isoform, start site, stop site) triples that enough
// reads carry; read_ends.tsv: one row per row read_stats.tsv has, in that order, with the rows the read covers, the bases it has in
// front of and behind its alignment, its sites and its variant.  The three files of --isoforms are what they are without the option.
#include "reports.hpp"

#include <cstdio>
#include <fstream>
#include <memory>

#include "common.hpp"

using namespace cer;
using std::string;

namespace {

// the sequences and call statistics of a polish call, segment after segment
struct PolishedSet {
    string seq, qual;
    std::vector<int64_t> off;
    std::vector<ioc_polish_stats> stats;
    void reset(int64_t cap, size_t n)
    {
        seq.assign(size_t(cap), '\0'), qual.assign(size_t(cap), '\0');
        off.assign(n + 1, 0), stats.assign(n, ioc_polish_stats{});
    }
};

// what comes back for one group
struct GroupResult {
    std::vector<int32_t> score;  // per pair ...
    std::vector<int64_t> windows;
    std::vector<ioc_aln_stats> stats;
    std::vector<uint8_t> alleles;  // (--sites) pair x's alleles at [allele_off[x], allele_off[x + 1])
    std::vector<int64_t> allele_off;
    std::vector<uint8_t> group;  // (--split)
    std::vector<int32_t> vote;
    std::vector<ioc_pileup_col> cols;  // (--pileup) the group's table, group_rows rows
    std::vector<ioc_pile_site> sites;  // (--sites, --split) segment g's sites at [site_off[g], site_off[g + 1]), site_found[g] before the cut
    std::vector<int64_t> site_off, site_found;
    std::vector<ioc_split_seg> split_seg;
    PolishedSet polished;        // (--polish) per segment
    PolishedSet group_polished;  // (--split-polish) per segment and side: 2 * g + h
    string cseq, cqual;          // (--correct) pair x's corrected bytes at [coff[x], coff[x + 1]), its record and the statistics of its alignment
    std::vector<int64_t> coff;
    std::vector<ioc_correct_stats> cstats;
    std::vector<ioc_aln_stats> caln;
    string icseq, icqual;        // (--isoforms-correct) the same of the correction by isoform
    std::vector<int64_t> icoff;
    std::vector<ioc_iso_correct_stats> icstats;
    std::vector<ioc_aln_stats> icaln;
    std::vector<ioc_pile_block> blocks;  // (--isoforms) segment g's kept blocks at [block_off[g], block_off[g + 1]), its record, and pair x's
    std::vector<int64_t> block_off;
    std::vector<ioc_blocks_seg> blocks_seg;
    std::vector<ioc_read_blocks> read_blocks;
    PolishedSet iso_polished;       // (--isoforms-polish) per called isoform: segment g's at [iso_off[g], iso_off[g + 1])
    std::vector<int64_t> iso_off;
    std::vector<ioc_pile_insert> inserts;  // (--isoforms-inserts) segment g's kept sites at [insert_off[g], insert_off[g + 1]), its record, and pair x's
    std::vector<int64_t> insert_off;
    std::vector<ioc_inserts_seg> inserts_seg;
    std::vector<ioc_read_inserts> read_inserts;
    std::vector<ioc_end_site> end_sites;  // (--isoforms-ends) segment g's start sites at [end_off[2 g], end_off[2 g + 1]), its stop sites behind them, its
    std::vector<int64_t> end_off, var_off;  // variants at [var_off[g], var_off[g + 1]), its record, and pair x's extent and record
    std::vector<ioc_end_variant> end_variants;
    std::vector<ioc_ends_seg> ends_seg;
    std::vector<ioc_read_extent> extents;
    std::vector<ioc_read_ends> read_ends;
    std::vector<ioc_insert_window> ins_windows;  // (--isoforms-inserts-seq) per kept site, in the order of `inserts`: its record, and its consensus at
    std::vector<int64_t> win_off;            // [win_off[s], win_off[s + 1]) of wseq / wqual
    std::vector<ioc_polish_stats> win_stats;
    string wseq, wqual;
    // (--isoforms-inserts-variants) per kept site its record and its two slots, slot 2 s + h at [vslot_off[2 s + h], vslot_off[2 s + h + 1]) of vseq /
    // vqual; per pair its variant bytes (IOC_INSERTS_MAX each) and its record; per segment its record
    std::vector<ioc_window_variant> win_variants;
    std::vector<int64_t> vslot_off;
    std::vector<ioc_polish_stats> var_stats;
    string vseq, vqual;
    std::vector<uint8_t> variant;
    std::vector<ioc_read_variants> read_variants;
    std::vector<ioc_variants_seg> variants_seg;
    // (--isoforms-full) per called combined isoform, segment g's at [full_off[g], full_off[g + 1]): its bytes at [fseq_off[x], fseq_off[x + 1]) of
    // fseq / fqual (room for the bound, written up to fseq_off's last entry), its records, and its site records from fsplice_off[x] on
    std::unique_ptr<char[]> fseq, fqual;
    std::vector<int64_t> full_off, fseq_off, fsplice_off;
    std::vector<ioc_polish_stats> fstats;
    std::vector<ioc_splice_site> fsplice;
};

// a row of the three per-read tables
struct RowResult {
    int32_t score = 0;
    int64_t windows = 0;
    ioc_aln_stats st{};
    size_t rep_len = 0;
    string alleles;                  // (--sites) one character per kept site of the read's cluster
    uint8_t group = IOC_SPLIT_NONE;  // (--split) the read's side, and ...
    int32_t vote = 0;                // ... its vote
    // (--correct) the read's record of corrected_reads.fq.  The file follows clusters.tsv, whose rows are in the order of the sorted
    // FASTQ and so interleave the clusters, while the groups come cluster by cluster: the records wait here until the last group
    // is done, the whole corrected read set in host memory (the other per-read tables keep a few words a row)
    string corrected;
    string iso_corrected;            // (--isoforms-correct) the read's record of corrected_reads_isoforms.fq, kept likewise
    ioc_read_blocks iso{};           // (--isoforms) the read's record, and how many blocks its cluster kept
    int32_t iso_blocks = 0;
    ioc_read_inserts ins{};          // (--isoforms-inserts) the read's record, and how many sites its cluster kept
    int32_t ins_sites = 0;
    ioc_read_variants var{0, -1, 0};  // (--isoforms-inserts-variants) the read's record and its variant at every kept site
    string variants;
    ioc_read_extent extent{};        // (--isoforms-ends) the read's extent and its record
    ioc_read_ends ends{-1, -1, -1, 0};
};

// The one place that chooses a library call.  --sites and / or --split come first; --polish, --correct and --isoforms are calls of their own,
// each of which takes the statistics and the first table only when no call before it produced them; otherwise the pileup;
// otherwise the statistics.
void align_group(ioc_ctx* c, int k, const ReportOpts& o, ReportGroup& g, GroupResult& r)
{
    const size_t nq = g.qoffs.size() - 1, np = g.pairs.size(), ns = g.segs.size();
    std::vector<double> qs(nq), qe(nq);
    check(c, ioc_qual_scores(c, int32_t(nq), g.qoffs.data(), reinterpret_cast<const uint8_t*>(g.quals.data()), k, qs.data(), qe.data()), "quality scores");
    for (size_t x = 0; x < np; ++x) g.pairs[x].e = qe[size_t(g.pair_q[x])] + qe[size_t(g.pair_rep_q[x])];
    check(c, ioc_align_set_pool(c, int32_t(g.offs.size() - 1), g.pool.data(), g.offs.data()), "sequence pool");
    r.score.assign(np, 0), r.windows.assign(np, 0), r.stats.assign(o.stats ? np : 0, ioc_aln_stats{});
    const int32_t n = int32_t(np), n_segs = int32_t(ns);
    const ioc_aln_pair* const pairs = g.pairs.data();
    int32_t* const sc = r.score.data();
    int64_t* const win = r.windows.data();
    ioc_aln_stats* const st = o.stats ? r.stats.data() : nullptr;
    const SitesOpt& so = o.sites;
    const SplitOpt& sp = o.split;
    bool have_first = false;  // the statistics and the first table are in r already
    if (so.on || sp.on) {
        const SiteCapacity cap = site_capacity(g, so.max_sites);
        r.sites.assign(size_t(cap.sites), ioc_pile_site{}), r.site_off.assign(ns + 1, 0), r.site_found.assign(ns, 0);
        r.alleles.assign(so.on ? size_t(cap.alleles) + 1 : size_t(1), 0), r.allele_off.assign(np + 1, 0);
        if (o.pileup) r.cols.assign(size_t(g.group_rows), ioc_pileup_col{});
        ioc_pileup_col* const cols = o.pileup ? r.cols.data() : nullptr;
        uint8_t* const alleles = so.on ? r.alleles.data() : nullptr;
        const int64_t a_cap = so.on ? cap.alleles : 0;
        if (sp.on) {
            r.group.assign(np, 0), r.vote.assign(np, 0), r.split_seg.assign(ns, ioc_split_seg{});
            if (o.group_polish()) {
                PolishedSet& gp = r.group_polished;
                const int64_t gcap = polish_capacity(g, 2);
                gp.reset(gcap, 2 * ns);
                check(c, ioc_align_pairs_split_polish(c, n, pairs, k, 2, -2, 1, sc, win, nullptr, st, n_segs, g.segs.data(), g.seg_of_pair.data(), so.min_depth,
                                                      so.min_alt, so.min_pct, so.max_sites, r.sites.data(), cap.sites, r.site_off.data(), r.site_found.data(),
                                                      alleles, a_cap, r.allele_off.data(), cols, sp.min_link, sp.min_margin, sp.rounds, nullptr, nullptr,
                                                      r.group.data(), r.vote.data(), r.split_seg.data(), sp.polish_min_depth, &gp.seq[0], &gp.qual[0], gcap,
                                                      gp.off.data(), gp.stats.data(), nullptr, nullptr),
                      "split by linked sites with the groups' consensus");
            } else {
                check(c, ioc_align_pairs_split(c, n, pairs, k, 2, -2, 1, sc, win, nullptr, st, n_segs, g.segs.data(), g.seg_of_pair.data(), so.min_depth,
                                               so.min_alt, so.min_pct, so.max_sites, r.sites.data(), cap.sites, r.site_off.data(), r.site_found.data(), alleles,
                                               a_cap, r.allele_off.data(), cols, sp.min_link, sp.min_margin, sp.rounds, nullptr, nullptr, r.group.data(),
                                               r.vote.data(), r.split_seg.data()),
                      "split by linked sites");
            }
        } else {
            check(c, ioc_align_pairs_alleles(c, n, pairs, k, 2, -2, 1, sc, win, nullptr, st, n_segs, g.segs.data(), g.seg_of_pair.data(), so.min_depth, so.min_alt,
                                             so.min_pct, so.max_sites, r.sites.data(), cap.sites, r.site_off.data(), r.site_found.data(), r.alleles.data(),
                                             cap.alleles, r.allele_off.data(), cols),
                  "variable sites");
        }
        have_first = true;
    }
    if (o.polish()) {
        PolishedSet& pol = r.polished;
        const int64_t cap = polish_capacity(g);
        pol.reset(cap, ns);
        if (o.pileup && !have_first) r.cols.assign(size_t(g.group_rows), ioc_pileup_col{});
        ioc_aln_stats* const st_out = have_first ? nullptr : st;
        ioc_pileup_col* const cols_out = o.pileup && !have_first ? r.cols.data() : nullptr;
        if (o.polish_weighted) {
            // (the quality lines lie in `quals` in the order and at the lengths of the sequences in `pool`)
            if (g.qoffs != g.offs) die("--polish-weighted: a quality line is not as long as its sequence!");
            check(c, ioc_align_set_pool_qual(c, g.quals.data(), int64_t(g.quals.size())), "pool qualities");
            check(c, ioc_align_pairs_polish_weighted(c, n, pairs, k, 2, -2, 1, sc, win, nullptr, st_out, n_segs, g.segs.data(), g.seg_of_pair.data(),
                                                     o.polish_min_depth, &pol.seq[0], &pol.qual[0], cap, pol.off.data(), pol.stats.data(), cols_out, nullptr,
                                                     nullptr),
                  "weighted polished consensus");
        } else {
            check(c, ioc_align_pairs_polish(c, n, pairs, k, 2, -2, 1, sc, win, nullptr, st_out, n_segs, g.segs.data(), g.seg_of_pair.data(), o.polish_min_depth,
                                            &pol.seq[0], &pol.qual[0], cap, pol.off.data(), pol.stats.data(), cols_out, nullptr),
                  "polished consensus");
        }
        have_first = true;
    }
    if (o.correct.on) {
        const CorrectOpt& co = o.correct;
        const int64_t cap = correct_capacity(g);
        r.cseq.assign(size_t(cap), '\0'), r.cqual.assign(size_t(cap), '\0');
        r.coff.assign(np + 1, 0), r.cstats.assign(np, ioc_correct_stats{}), r.caln.assign(np, ioc_aln_stats{});
        if (o.pileup && !have_first) r.cols.assign(size_t(g.group_rows), ioc_pileup_col{});
        check(c, ioc_align_pairs_correct(c, n, pairs, k, 2, -2, 1, sc, win, nullptr, r.caln.data(), n_segs, g.segs.data(), g.seg_of_pair.data(), co.min_depth,
                                         co.min_alt, co.min_pct, co.max_run, &r.cseq[0], &r.cqual[0], cap, r.coff.data(), r.cstats.data(),
                                         o.pileup && !have_first ? r.cols.data() : nullptr, nullptr),
              "read correction");
        if (o.stats && !have_first) r.stats = r.caln;
        have_first = true;
    }
    if (o.isoforms.on) {
        const IsoformsOpt& io = o.isoforms;
        const int64_t cap = blocks_capacity(g, io.max_blocks);
        r.blocks.assign(size_t(std::max<int64_t>(cap, 1)), ioc_pile_block{}), r.block_off.assign(ns + 1, 0), r.blocks_seg.assign(ns, ioc_blocks_seg{});
        r.read_blocks.assign(np, ioc_read_blocks{});
        // (a corrected record needs the free ends of its alignment: the statistics an earlier call of the group left — --correct's, or
        // those of --read-stats — serve where there are any, and the reduction does not run again for the same pairs)
        const std::vector<ioc_aln_stats>* const earlier = !io.correct ? nullptr : r.caln.size() == np ? &r.caln : have_first && r.stats.size() == np ? &r.stats : nullptr;
        std::vector<ioc_aln_stats> aln((o.stats && !have_first) || (io.correct && !earlier) ? np : 0);
        if (o.pileup && !have_first) r.cols.assign(size_t(g.group_rows), ioc_pileup_col{});
        // every call of the block family begins with the same arguments, the context's to the table's: `more` is what its later stages take
        const auto blocks_call = [&](auto entry, const char* what, auto... more) {
            check(c, entry(c, n, pairs, k, 2, -2, 1, sc, win, nullptr, aln.empty() ? nullptr : aln.data(), n_segs, g.segs.data(), g.seg_of_pair.data(), io.min_gap,
                           io.min_depth, io.min_alt, io.min_pct, io.min_block, io.max_blocks, nullptr, r.blocks.data(), cap, r.block_off.data(), r.read_blocks.data(),
                           r.blocks_seg.data(), o.pileup && !have_first ? r.cols.data() : nullptr, more...),
                  what);
        };
        if (o.iso_polish()) {
            PolishedSet& ip = r.iso_polished;
            const IsoCapacity icap = iso_polish_capacity(g, io.polish_max);
            ip.reset(icap.bytes, size_t(icap.isoforms));
            r.iso_off.assign(ns + 1, 0);
            if (io.polish_weighted) {
                // (the quality lines lie in `quals` in the order and at the lengths of the sequences in `pool`)
                if (g.qoffs != g.offs) die("--isoforms-polish-weighted: a quality line is not as long as its sequence!");
                check(c, ioc_align_set_pool_qual(c, g.quals.data(), int64_t(g.quals.size())), "pool qualities");
            }
            blocks_call(io.polish_weighted ? ioc_align_pairs_blocks_polish_weighted : ioc_align_pairs_blocks_polish,
                        io.polish_weighted ? "exon blocks with the isoforms' weighted consensus" : "exon blocks with the isoforms' consensus", io.polish_max,
                        io.polish_min_depth, &ip.seq[0], &ip.qual[0], icap.bytes, ip.off.data(), ip.stats.data(), icap.isoforms, r.iso_off.data());
        } else if (io.inserts) {
            const int64_t icap = inserts_capacity(g, io.ins_max);
            r.inserts.assign(size_t(std::max<int64_t>(icap, 1)), ioc_pile_insert{}), r.insert_off.assign(ns + 1, 0), r.inserts_seg.assign(ns, ioc_inserts_seg{});
            r.read_inserts.assign(np, ioc_read_inserts{});
            const auto inserts_call = [&](auto entry, const char* what, auto... more) {
                blocks_call(entry, what, io.min_ins, io.ins_slack, io.ins_max, nullptr, r.inserts.data(), icap, r.insert_off.data(), r.read_inserts.data(),
                            r.inserts_seg.data(), more...);
            };
            if (io.inserts_seq) {
                // (the scoring of the windows: the aligner's match and mismatch, a gap that costs what a mismatch does; the call at depth 3)
                const int64_t wcap = icap * (7 * int64_t(io.ins_max_win) + 6);
                r.ins_windows.assign(size_t(std::max<int64_t>(icap, 1)), ioc_insert_window{}), r.win_off.assign(size_t(icap) + 1, 0);
                r.win_stats.assign(size_t(std::max<int64_t>(icap, 1)), ioc_polish_stats{});
                r.wseq.assign(size_t(std::max<int64_t>(wcap, 1)), '\0'), r.wqual.assign(size_t(std::max<int64_t>(wcap, 1)), '\0');
                const bool variants = io.variants && !io.full, full = io.full || (variants && io.full_variants);
                if (variants) {
                    r.win_variants.assign(size_t(std::max<int64_t>(icap, 1)), ioc_window_variant{}), r.vslot_off.assign(2 * size_t(icap) + 1, 0);
                    r.var_stats.assign(size_t(std::max<int64_t>(2 * icap, 1)), ioc_polish_stats{});
                    r.vseq.assign(size_t(std::max<int64_t>(2 * wcap, 1)), '\0'), r.vqual.assign(size_t(std::max<int64_t>(2 * wcap, 1)), '\0');
                    r.variant.assign(np * size_t(IOC_INSERTS_MAX), 0), r.read_variants.assign(np, ioc_read_variants{}), r.variants_seg.assign(ns, ioc_variants_seg{});
                }
                // (the full-length room is the bound, which is generous: a window's 7 max_win + 6 bytes a site an isoform — by variant one
                // slot a site is taken; the pages the call does not write are never touched)
                const IsoCapacity fcap = full ? iso_full_capacity(g, io.full_max, io.ins_max, io.ins_max_win) : IsoCapacity{};
                if (full) {
                    r.fseq.reset(new char[size_t(std::max<int64_t>(fcap.bytes, 1))]), r.fqual.reset(new char[size_t(std::max<int64_t>(fcap.bytes, 1))]);
                    r.full_off.assign(ns + 1, 0), r.fseq_off.assign(size_t(fcap.isoforms) + 1, 0), r.fsplice_off.assign(size_t(fcap.isoforms) + 1, 0);
                    r.fstats.assign(size_t(std::max<int64_t>(fcap.isoforms, 1)), ioc_polish_stats{});
                    r.fsplice.assign(size_t(std::max<int64_t>(fcap.isoforms * io.ins_max, 1)), ioc_splice_site{});
                }
                // the window stage's arguments behind the insert stage's, the variant stage's behind those, the isoforms' last
                const auto windows_call = [&](auto entry, const char* what, auto... more) {
                    inserts_call(entry, what, io.ins_max_win, 2, -2, 2, 3, r.ins_windows.data(), &r.wseq[0], &r.wqual[0], wcap, r.win_off.data(), r.win_stats.data(), more...);
                };
                const auto variants_call = [&](auto entry, const char* what, auto... more) {
                    windows_call(entry, what, io.variants_min_agree, r.win_variants.data(), &r.vseq[0], &r.vqual[0], 2 * wcap, r.vslot_off.data(), r.var_stats.data(),
                                 r.variant.data(), nullptr, r.read_variants.data(), r.variants_seg.data(), more...);
                };
                const auto full_call = [&](const auto& call, auto entry, const char* what) {
                    call(entry, what, io.full_max, r.fseq.get(), r.fqual.get(), fcap.bytes, r.fseq_off.data(), r.fstats.data(), nullptr, r.fsplice.data(),
                         int64_t(r.fsplice.size()), r.fsplice_off.data(), fcap.isoforms, r.full_off.data());
                };
                if (variants && full)
                    full_call(variants_call, ioc_align_pairs_isoforms_full_variants,
                              "exon blocks with the insertion sites, their sequences, their variants and the isoforms' full-length sequences by variant");
                else if (full)
                    full_call(windows_call, ioc_align_pairs_isoforms_full, "exon blocks with the insertion sites, their sequences and the isoforms' full-length sequences");
                else if (variants)
                    variants_call(ioc_align_pairs_blocks_inserts_variants, "exon blocks with the insertion sites, their sequences and their variants");
                else
                    windows_call(ioc_align_pairs_blocks_inserts_seq, "exon blocks with the insertion sites and their sequences");
            } else
                inserts_call(ioc_align_pairs_blocks_inserts, "exon blocks with the insertion sites");
        } else if (io.ends) {
            const EndsCapacity ecap = ends_capacity(g, io.ends_max, io.ends_max_variants);
            r.end_sites.assign(size_t(std::max<int64_t>(ecap.sites, 1)), ioc_end_site{}), r.end_off.assign(2 * ns + 1, 0), r.var_off.assign(ns + 1, 0);
            r.end_variants.assign(size_t(std::max<int64_t>(ecap.variants, 1)), ioc_end_variant{}), r.ends_seg.assign(ns, ioc_ends_seg{});
            r.extents.assign(np, ioc_read_extent{}), r.read_ends.assign(np, ioc_read_ends{});
            blocks_call(ioc_align_pairs_blocks_ends, "exon blocks with the alternative ends", io.ends_slack, io.ends_min_over, io.ends_min_pct, io.ends_max,
                        io.ends_max_variants, r.extents.data(), nullptr, r.end_sites.data(), ecap.sites, r.end_off.data(), r.end_variants.data(), ecap.variants,
                        r.var_off.data(), r.read_ends.data(), r.ends_seg.data());
        } else if (io.correct) {
            const CorrectOpt& co = o.correct;
            const int64_t ccap = iso_correct_capacity(g);
            r.icseq.assign(size_t(std::max<int64_t>(ccap, 1)), '\0'), r.icqual.assign(size_t(std::max<int64_t>(ccap, 1)), '\0');
            r.icoff.assign(np + 1, 0), r.icstats.assign(np, ioc_iso_correct_stats{});
            blocks_call(ioc_align_pairs_blocks_correct, "exon blocks with every read corrected against its isoform", co.min_depth, co.min_alt, co.min_pct, co.max_run,
                        &r.icseq[0], &r.icqual[0], ccap, r.icoff.data(), r.icstats.data());
            r.icaln = earlier ? *earlier : aln;
        } else {
            blocks_call(ioc_align_pairs_blocks, "exon blocks");
        }
        if (o.stats && !have_first) r.stats = aln;
        have_first = true;
    }
    if (have_first) return;
    if (o.pileup) {
        r.cols.assign(size_t(g.group_rows), ioc_pileup_col{});
        check(c, ioc_align_pairs_pileup(c, n, pairs, k, 2, -2, 1, sc, win, nullptr, st, g.row_base.data(), g.group_rows, r.cols.data()), "alignment pileup");
    } else {
        check(c, ioc_align_pairs_stats(c, n, pairs, k, 2, -2, 1, sc, win, nullptr, r.stats.data()), "alignment statistics");
    }
}

// a group's results into the rows of the per-read tables
void scatter_to_rows(const ReportOpts& o, const ReportRows& rows, const ReportGroup& g, const GroupResult& r, std::vector<RowResult>& res)
{
    for (size_t x = 0; x < g.pairs.size(); ++x) {
        RowResult& row = res[g.pair_row[x]];
        row.rep_len = size_t(g.offs[size_t(g.pairs[x].ref) + 1] - g.offs[size_t(g.pairs[x].ref)]);
        if (o.stats) row.score = r.score[x], row.windows = r.windows[x], row.st = r.stats[x];
        if (o.split.on) row.group = r.group[x], row.vote = r.vote[x];
        if (o.sites.on) {
            const int64_t s0 = r.site_off[size_t(g.seg_of_pair[x])];
            for (int64_t a = r.allele_off[x]; a < r.allele_off[x + 1]; ++a)
                row.alleles += allele_char(r.sites[size_t(s0 + a - r.allele_off[x])].kind, r.alleles[size_t(a)]);
            if (row.alleles.empty()) row.alleles = "*";
        }
        if (o.isoforms.on) row.iso = r.read_blocks[x], row.iso_blocks = r.blocks_seg[size_t(g.seg_of_pair[x])].n_blocks;
        if (o.isoforms.on && o.isoforms.inserts) row.ins = r.read_inserts[x], row.ins_sites = r.inserts_seg[size_t(g.seg_of_pair[x])].n_sites;
        if (o.isoforms.on && o.isoforms.inserts && o.isoforms.variants) {
            row.var = r.read_variants[x];
            row.variants.clear();
            for (int32_t b = 0; b < row.ins_sites && b < IOC_INSERTS_MAX; ++b) row.variants += ".ABo"[r.variant[x * size_t(IOC_INSERTS_MAX) + size_t(b)] & 3u];
        }
        if (o.isoforms.on && o.isoforms.ends) row.extent = r.extents[x], row.ends = r.read_ends[x];
        if (o.isoforms.on && o.isoforms.correct) {
            const ReadStatRow& rd = rows.row(g.pair_row[x]);
            const size_t q0 = size_t(g.offs[size_t(g.pairs[x].query)]), l0 = size_t(g.qoffs[size_t(g.pair_q[x])]), l1 = size_t(g.qoffs[size_t(g.pair_q[x]) + 1]);
            row.iso_corrected = iso_corrected_record(rd.id, rd.id_len, rd.cls, g.pool.data() + q0, rd.seq_len, g.quals.data() + l0, l1 - l0, r.icaln[x], r.icstats[x],
                                                     r.read_blocks[x].group, r.icseq.data() + r.icoff[x], r.icqual.data() + r.icoff[x],
                                                     size_t(r.icoff[x + 1] - r.icoff[x]));
        }
        if (o.correct.on) {
            const ReadStatRow& rd = rows.row(g.pair_row[x]);
            const size_t q0 = size_t(g.offs[size_t(g.pairs[x].query)]), l0 = size_t(g.qoffs[size_t(g.pair_q[x])]), l1 = size_t(g.qoffs[size_t(g.pair_q[x]) + 1]);
            row.corrected = corrected_record(rd.id, rd.id_len, rd.cls, g.pool.data() + q0, rd.seq_len, g.quals.data() + l0, l1 - l0, r.caln[x], r.cstats[x],
                                             r.cseq.data() + r.coff[x], r.cqual.data() + r.coff[x], size_t(r.coff[x + 1] - r.coff[x]));
        }
    }
}

// a cluster's representative as cluster_cons.fq has it
string frame_of(const Batch& b, size_t ci)
{
    const auto& rep = b.Cls[ci]->at(0);
    return rep->MatchStrand == -1 ? revcomp(rep->RawSeq->seq.str()) : rep->RawSeq->seq.str();
}

const char* site_kind(const ioc_pile_site& t) { return t.kind == IOC_SITE_INS ? "ins" : "base"; }

void write_pileup(std::ofstream& out, const Batch& b, const ReportGroup& g, const GroupResult& r)
{
    string text;
    for (const auto& gc : g.group_cls) {
        const string frame = frame_of(b, gc.first);
        text.clear();
        for (size_t p = 0; p <= frame.size(); ++p) {
            const ioc_pileup_col z = gc.second < 0 ? ioc_pileup_col{} : r.cols[size_t(gc.second) + p];
            text += std::to_string(gc.first) + '\t' + std::to_string(p) + '\t' + (p < frame.size() ? frame[p] : '-') + '\t' +
                    std::to_string(uint64_t(z.a) + z.c + z.g + z.t + z.other + z.del) + '\t' + std::to_string(z.a) + '\t' + std::to_string(z.c) + '\t' +
                    std::to_string(z.g) + '\t' + std::to_string(z.t) + '\t' + std::to_string(z.other) + '\t' + std::to_string(z.del) + '\t' +
                    std::to_string(z.ins_runs) + '\t' + std::to_string(z.ins_bases) + '\n';
        }
        out.write(text.data(), std::streamsize(text.size()));
    }
}

void write_polish(std::ofstream& out, const Batch& b, const ReportGroup& g, const GroupResult& r, bool weighted)
{
    const PolishedSet& pol = r.polished;
    const char* const tail = weighted ? " weighted=1" : "";
    for (size_t x = 0; x < g.group_cls.size(); ++x) {
        const int32_t s = g.group_seg[x];
        const string name = "cluster_" + std::to_string(g.group_cls[x].first);
        string text;
        if (s < 0) {  // a cluster without a row: its representative, nothing called
            const string seq = frame_of(b, g.group_cls[x].first), qual(seq.size(), '!');
            ioc_polish_stats z{};
            z.n_low = int32_t(seq.size());
            text = polish_record(name, 0, z, tail, seq.data(), qual.data(), seq.size());
        } else {
            const size_t at = size_t(pol.off[size_t(s)]), len = size_t(pol.off[size_t(s) + 1]) - at;
            text = polish_record(name, g.seg_reads[size_t(s)], pol.stats[size_t(s)], tail, pol.seq.data() + at, pol.qual.data() + at, len);
        }
        out.write(text.data(), std::streamsize(text.size()));
    }
}

void write_sites(std::ofstream& out, const ReportGroup& g, const GroupResult& r)
{
    string text;
    for (size_t x = 0; x < g.group_cls.size(); ++x) {
        const int32_t s = g.group_seg[x];
        if (s < 0) continue;
        text.clear();
        const string id = std::to_string(g.group_cls[x].first);
        const int64_t s0 = r.site_off[size_t(s)], s1 = r.site_off[size_t(s) + 1];
        if (r.site_found[size_t(s)] > s1 - s0) text += "# cluster " + id + ": kept " + std::to_string(s1 - s0) + " of " + std::to_string(r.site_found[size_t(s)]) + " sites\n";
        for (int64_t at = s0; at < s1; ++at) {
            const ioc_pile_site& t = r.sites[size_t(at)];
            text += id + '\t' + std::to_string(t.row) + '\t' + site_kind(t) + '\t' + std::to_string(t.depth) + '\t' + allele_char(t.kind, t.major) + '\t' +
                    std::to_string(t.n_major) + '\t' + allele_char(t.kind, t.minor) + '\t' + std::to_string(t.n_minor) + '\n';
        }
        out.write(text.data(), std::streamsize(text.size()));
    }
}

void write_split(std::ofstream& out, const ReportGroup& g, const GroupResult& r)
{
    string text;
    for (size_t x = 0; x < g.group_cls.size(); ++x) {
        const int32_t s = g.group_seg[x];
        const ioc_split_seg z = s < 0 ? ioc_split_seg{-1, 0, 0, 0, 0, 0, 0} : r.split_seg[size_t(s)];
        const int64_t s0 = s < 0 ? 0 : r.site_off[size_t(s)], n_sites = s < 0 ? 0 : r.site_off[size_t(s) + 1] - s0;
        text = std::to_string(g.group_cls[x].first) + '\t' + std::to_string(n_sites) + '\t' + std::to_string(z.n_linked) + '\t';
        if (z.seed >= 0 && z.seed < n_sites) {
            const ioc_pile_site& t = r.sites[size_t(s0 + z.seed)];
            text += std::to_string(t.row) + '\t' + site_kind(t);
        } else {
            text += ".\t.";
        }
        text += '\t' + std::to_string(z.n_reads) + '\t' + std::to_string(z.n_group0) + '\t' + std::to_string(z.n_group1) + '\t' + std::to_string(z.n_none) + '\n';
        out.write(text.data(), std::streamsize(text.size()));
    }
}

void write_group_polish(std::ofstream& out, const ReportGroup& g, const GroupResult& r)
{
    const PolishedSet& gp = r.group_polished;
    for (size_t x = 0; x < g.group_cls.size(); ++x) {
        const int32_t s = g.group_seg[x];
        if (s < 0 || r.split_seg[size_t(s)].seed < 0) continue;
        for (size_t h = 0; h < 2; ++h) {
            const int32_t reads = h ? r.split_seg[size_t(s)].n_group1 : r.split_seg[size_t(s)].n_group0;
            if (reads <= 0) continue;
            const size_t gs = 2 * size_t(s) + h, at = size_t(gp.off[gs]), len = size_t(gp.off[gs + 1] - gp.off[gs]);
            const string text = polish_record("cluster_" + std::to_string(g.group_cls[x].first) + '/' + std::to_string(h), reads, gp.stats[gs], "",
                                              gp.seq.data() + at, gp.qual.data() + at, len);
            out.write(text.data(), std::streamsize(text.size()));
        }
    }
}

void write_blocks(std::ofstream& blocks, std::ofstream& isoforms, std::ofstream* iso_fq, const ReportGroup& g, const GroupResult& r)
{
    std::vector<std::vector<ioc_read_blocks>> mine(g.segs.size());
    for (size_t x = 0; x < g.pairs.size(); ++x) mine[size_t(g.seg_of_pair[x])].push_back(r.read_blocks[x]);
    for (size_t x = 0; x < g.group_cls.size(); ++x) {
        const int32_t s = g.group_seg[x];
        if (s < 0) continue;
        const string rows = cluster_blocks_rows(g.group_cls[x].first, r.blocks_seg[size_t(s)], r.blocks.data() + r.block_off[size_t(s)]);
        const string iso = cluster_isoforms_rows(g.group_cls[x].first, r.blocks_seg[size_t(s)], mine[size_t(s)]);
        blocks.write(rows.data(), std::streamsize(rows.size()));
        isoforms.write(iso.data(), std::streamsize(iso.size()));
        if (!iso_fq) continue;
        const PolishedSet& ip = r.iso_polished;
        const int64_t i0 = r.iso_off[size_t(s)], i1 = r.iso_off[size_t(s) + 1];
        const string fq = cluster_isoform_records(g.group_cls[x].first, r.blocks_seg[size_t(s)], mine[size_t(s)], i1 - i0, ip.off.data() + i0, ip.stats.data() + i0,
                                                  ip.seq.data(), ip.qual.data());
        iso_fq->write(fq.data(), std::streamsize(fq.size()));
    }
}

void write_inserts(std::ofstream& out, const ReportGroup& g, const GroupResult& r)
{
    for (size_t x = 0; x < g.group_cls.size(); ++x) {
        const int32_t s = g.group_seg[x];
        if (s < 0) continue;
        const string rows = cluster_inserts_rows(g.group_cls[x].first, r.inserts_seg[size_t(s)], r.inserts.data() + r.insert_off[size_t(s)]);
        out.write(rows.data(), std::streamsize(rows.size()));
    }
}

void write_ends(std::ofstream& ends, std::ofstream& variants, const ReportGroup& g, const GroupResult& r)
{
    for (size_t x = 0; x < g.group_cls.size(); ++x) {
        const int32_t s = g.group_seg[x];
        if (s < 0) continue;
        const ioc_ends_seg& z = r.ends_seg[size_t(s)];
        const string rows = cluster_ends_rows(g.group_cls[x].first, z, r.end_sites.data() + r.end_off[2 * size_t(s)], r.end_sites.data() + r.end_off[2 * size_t(s) + 1]);
        const string vars = cluster_end_variants_rows(g.group_cls[x].first, z, r.end_variants.data() + r.var_off[size_t(s)]);
        ends.write(rows.data(), std::streamsize(rows.size()));
        variants.write(vars.data(), std::streamsize(vars.size()));
    }
}

// cluster_inserts.fq: a record per called site, "@cluster_<id>/ins<b> rows=<lo>-<hi> voters=<n> template=<read>" — the consensus of
// what the voters hold between rows lo and hi of the representative, to stand in place of those rows
void write_insert_windows(std::ofstream& out, const ReportRows& rows, const ReportGroup& g, const GroupResult& r)
{
    for (size_t x = 0; x < g.group_cls.size(); ++x) {
        const int32_t s = g.group_seg[x];
        if (s < 0) continue;
        for (int64_t a = r.insert_off[size_t(s)]; a < r.insert_off[size_t(s) + 1]; ++a) {
            const ioc_insert_window& w = r.ins_windows[size_t(a)];
            const int64_t b0 = r.win_off[size_t(a)], b1 = r.win_off[size_t(a) + 1];
            if (w.tlen <= 0 || b1 <= b0 || w.template_pair < 0 || size_t(w.template_pair) >= g.pair_row.size()) continue;
            const ReadStatRow& rd = rows.row(g.pair_row[size_t(w.template_pair)]);
            out << "@cluster_" << g.group_cls[x].first << "/ins" << a - r.insert_off[size_t(s)] << " rows=" << w.lo << '-' << w.hi << " voters=" << w.n_voters
                << " template=" << string(rd.id, rd.id_len) << '\n';
            out.write(r.wseq.data() + b0, std::streamsize(b1 - b0));
            out << "\n+\n";
            out.write(r.wqual.data() + b0, std::streamsize(b1 - b0));
            out << '\n';
        }
    }
}

// cluster_insert_variants.fq: a record per called variant of a site, "@cluster_<id>/ins<b>/<A|B> rows=<lo>-<hi> voters=<n> template=<read>
// split=<0|1>" — variant A is the one of the site's template, and the only one where the site does not split
void write_insert_variants(std::ofstream& out, const ReportRows& rows, const ReportGroup& g, const GroupResult& r)
{
    for (size_t x = 0; x < g.group_cls.size(); ++x) {
        const int32_t s = g.group_seg[x];
        if (s < 0) continue;
        for (int64_t a = r.insert_off[size_t(s)]; a < r.insert_off[size_t(s) + 1]; ++a) {
            const ioc_insert_window& w = r.ins_windows[size_t(a)];
            const ioc_window_variant& v = r.win_variants[size_t(a)];
            for (int h = 0; h < 2; ++h) {
                const int64_t b0 = r.vslot_off[2 * size_t(a) + size_t(h)], b1 = r.vslot_off[2 * size_t(a) + size_t(h) + 1];
                const int32_t pair = h ? v.template_pair_b : w.template_pair;
                if (b1 <= b0 || pair < 0 || size_t(pair) >= g.pair_row.size()) continue;
                const ReadStatRow& rd = rows.row(g.pair_row[size_t(pair)]);
                out << "@cluster_" << g.group_cls[x].first << "/ins" << a - r.insert_off[size_t(s)] << '/' << "AB"[h] << " rows=" << w.lo << '-' << w.hi
                    << " voters=" << (h ? v.n_b : v.n_a) << " template=" << string(rd.id, rd.id_len) << " split=" << v.split << '\n';
                out.write(r.vseq.data() + b0, std::streamsize(b1 - b0));
                out << "\n+\n";
                out.write(r.vqual.data() + b0, std::streamsize(b1 - b0));
                out << '\n';
            }
        }
    }
}

// cluster_isoforms_full.fq: a record per called combined isoform of every cluster that has a block or a site
void write_isoforms_full(std::ofstream& out, const ReportGroup& g, const GroupResult& r)
{
    for (size_t x = 0; x < g.group_cls.size(); ++x) {
        const int32_t s = g.group_seg[x];
        if (s < 0 || (r.blocks_seg[size_t(s)].n_blocks < 1 && r.inserts_seg[size_t(s)].n_sites < 1)) continue;
        const int64_t i0 = r.full_off[size_t(s)], n = r.full_off[size_t(s) + 1] - i0;
        std::vector<uint64_t> bkey(size_t(n), 0), ikey(size_t(n), 0);
        std::vector<int32_t> mine(size_t(n), 0);
        for (size_t p = 0; p < g.pairs.size(); ++p) {
            const ioc_read_inserts& ri = r.read_inserts[p];
            if (g.seg_of_pair[p] != s || ri.group < 0 || ri.group >= n) continue;
            if (ri.how == IOC_ISO_DIRECT) bkey[size_t(ri.group)] = r.read_blocks[p].key, ikey[size_t(ri.group)] = ri.key;
            if (ri.how == IOC_ISO_DIRECT || ri.how == IOC_ISO_ASSIGNED) ++mine[size_t(ri.group)];
        }
        for (int64_t h = 0; h < n; ++h) {
            const size_t at = size_t(r.fseq_off[size_t(i0 + h)]), len = size_t(r.fseq_off[size_t(i0 + h) + 1]) - at;
            string tail;
            for (int64_t b = r.fsplice_off[size_t(i0 + h)]; b < r.fsplice_off[size_t(i0 + h) + 1]; ++b)
                if (r.fsplice[size_t(b)].state == IOC_SPLICE_DONE)
                    tail += " ins" + std::to_string(b - r.fsplice_off[size_t(i0 + h)]) + '@' + std::to_string(r.fsplice[size_t(b)].at) + '+' + std::to_string(r.fsplice[size_t(b)].len);
            const string text = polish_record("cluster_" + std::to_string(g.group_cls[x].first) + "/iso" + std::to_string(h) + " key=" +
                                                  blocks_signature(bkey[size_t(h)], r.blocks_seg[size_t(s)].n_blocks) + '/' +
                                                  inserts_signature(ikey[size_t(h)], r.inserts_seg[size_t(s)].n_sites),
                                              mine[size_t(h)], r.fstats[size_t(i0 + h)], tail.c_str(), r.fseq.get() + at, r.fqual.get() + at, len);
            out.write(text.data(), std::streamsize(text.size()));
        }
    }
}

// cluster_isoforms_full_variants.fq: a record per called isoform as the variant stage counted them again, of every cluster that has a
// block or a site — cluster_isoforms_full.fq's records, the sites half of key= in the variant file's letters and every spliced site
// with the variant whose record of cluster_insert_variants.fq stands there
void write_isoforms_full_variants(std::ofstream& out, const ReportGroup& g, const GroupResult& r)
{
    for (size_t x = 0; x < g.group_cls.size(); ++x) {
        const int32_t s = g.group_seg[x];
        if (s < 0 || (r.blocks_seg[size_t(s)].n_blocks < 1 && r.inserts_seg[size_t(s)].n_sites < 1)) continue;
        const int64_t i0 = r.full_off[size_t(s)], n = r.full_off[size_t(s) + 1] - i0;
        std::vector<uint64_t> bkey(size_t(n), 0), key2(size_t(n), 0);
        std::vector<uint8_t> has(size_t(n), 0);
        std::vector<int32_t> mine(size_t(n), 0);
        for (size_t p = 0; p < g.pairs.size(); ++p) {
            const ioc_read_variants& rv = r.read_variants[p];
            if (g.seg_of_pair[p] != s || rv.group < 0 || rv.group >= n) continue;
            if (rv.how == IOC_ISO_DIRECT && !has[size_t(rv.group)]) bkey[size_t(rv.group)] = r.read_blocks[p].key, key2[size_t(rv.group)] = rv.key2, has[size_t(rv.group)] = 1;
            if (rv.how == IOC_ISO_DIRECT || rv.how == IOC_ISO_ASSIGNED) ++mine[size_t(rv.group)];
        }
        for (int64_t h = 0; h < n; ++h) {
            const size_t at = size_t(r.fseq_off[size_t(i0 + h)]), len = size_t(r.fseq_off[size_t(i0 + h) + 1]) - at;
            const int64_t b0 = r.fsplice_off[size_t(i0 + h)];
            const string tail = full_variants_tail(key2[size_t(h)], r.fsplice.data() + b0, r.fsplice_off[size_t(i0 + h) + 1] - b0);
            const string text = polish_record("cluster_" + std::to_string(g.group_cls[x].first) + "/iso" + std::to_string(h) + " key=" +
                                                  blocks_signature(bkey[size_t(h)], r.blocks_seg[size_t(s)].n_blocks) + '/' +
                                                  variants_signature(key2[size_t(h)], r.inserts_seg[size_t(s)].n_sites),
                                              mine[size_t(h)], r.fstats[size_t(i0 + h)], tail.c_str(), r.fseq.get() + at, r.fqual.get() + at, len);
            out.write(text.data(), std::streamsize(text.size()));
        }
    }
}

// the files that grow group by group
struct GroupFiles {
    std::ofstream pileup, polish, sites, split, group_polish, blocks, isoforms, iso_fq, inserts, inserts_fq, variants_fq, full_fq, full_variants_fq, ends, end_variants;
    GroupFiles(const string& outdir, const ReportOpts& o)
    {
        if (o.pileup) {
            create_file(outdir + "/cluster_pileup.tsv", pileup);
            pileup << "ClusterId\tPos\tRepBase\tDepth\tA\tC\tG\tT\tN\tDel\tInsReads\tInsBases\n";
        }
        if (o.polish()) create_file(outdir + "/cluster_polished.fq", polish);
        if (o.sites.on) {
            create_file(outdir + "/cluster_sites.tsv", sites);
            sites << "ClusterId\tPos\tKind\tDepth\tMajor\tNMajor\tMinor\tNMinor\n";
        }
        if (o.split.on) {
            create_file(outdir + "/cluster_split.tsv", split);
            split << "ClusterId\tNSites\tNLinked\tSeedPos\tSeedKind\tNReads\tNGroup0\tNGroup1\tNNone\n";
        }
        if (o.group_polish()) create_file(outdir + "/cluster_split_polished.fq", group_polish);
        if (o.isoforms.on) {
            create_file(outdir + "/cluster_blocks.tsv", blocks);
            blocks << "ClusterId\tBlock\tFirst\tEnd\tKeep\tSkip\tPart\tNone\n";
            create_file(outdir + "/cluster_isoforms.tsv", isoforms);
            isoforms << "ClusterId\tIsoform\tSignature\tDirect\tAssigned\n";
        }
        if (o.iso_polish()) create_file(outdir + "/cluster_isoforms.fq", iso_fq);
        if (o.isoforms.on && o.isoforms.inserts) {
            create_file(outdir + "/cluster_inserts.tsv", inserts);
            inserts << "ClusterId\tFirst\tEnd\tCarry\tLack\tNone\tLenMin\tLenMax\n";
            if (o.isoforms.inserts_seq) create_file(outdir + "/cluster_inserts.fq", inserts_fq);
            if (o.isoforms.inserts_seq && o.isoforms.full) create_file(outdir + "/cluster_isoforms_full.fq", full_fq);
            if (o.isoforms.inserts_seq && o.isoforms.variants) create_file(outdir + "/cluster_insert_variants.fq", variants_fq);
            if (o.isoforms.inserts_seq && o.isoforms.variants && o.isoforms.full_variants) create_file(outdir + "/cluster_isoforms_full_variants.fq", full_variants_fq);
        }
        if (o.isoforms.on && o.isoforms.ends) {
            create_file(outdir + "/cluster_ends.tsv", ends);
            ends << "ClusterId\tKind\tIndex\tFirst\tEnd\tPeakRow\tPeakReads\tReads\tOver\n";
            create_file(outdir + "/cluster_end_variants.tsv", end_variants);
            end_variants << "ClusterId\tVariant\tIsoform\tStartSite\tStopSite\tReads\n";
        }
    }
    void write(const Batch& b, const ReportOpts& o, const ReportRows& rows, const ReportGroup& g, const GroupResult& r)
    {
        if (o.pileup) write_pileup(pileup, b, g, r);
        if (o.polish()) write_polish(polish, b, g, r, o.polish_weighted);
        if (o.sites.on && !g.segs.empty()) write_sites(sites, g, r);
        if (o.split.on) write_split(split, g, r);
        if (o.group_polish() && !g.segs.empty()) write_group_polish(group_polish, g, r);
        if (o.isoforms.on && !g.segs.empty()) write_blocks(blocks, isoforms, o.iso_polish() ? &iso_fq : nullptr, g, r);
        if (o.isoforms.on && o.isoforms.inserts && !g.segs.empty()) write_inserts(inserts, g, r);
        if (o.isoforms.on && o.isoforms.ends && !g.segs.empty() && !g.pairs.empty()) write_ends(ends, end_variants, g, r);
        if (o.isoforms.on && o.isoforms.inserts && o.isoforms.inserts_seq && !g.segs.empty() && !g.pairs.empty()) write_insert_windows(inserts_fq, rows, g, r);
        if (o.isoforms.on && o.isoforms.inserts && o.isoforms.inserts_seq && o.isoforms.full && !g.segs.empty() && !g.pairs.empty()) write_isoforms_full(full_fq, g, r);
        if (o.isoforms.on && o.isoforms.inserts && o.isoforms.inserts_seq && o.isoforms.variants && !g.segs.empty() && !g.pairs.empty()) write_insert_variants(variants_fq, rows, g, r);
        if (o.isoforms.on && o.isoforms.inserts && o.isoforms.inserts_seq && o.isoforms.variants && o.isoforms.full_variants && !g.segs.empty() && !g.pairs.empty())
            write_isoforms_full_variants(full_variants_fq, g, r);
    }
};

// the three per-read tables, from the flat per-row results
void write_read_alleles(const string& outdir, const ReportRows& rows, const std::vector<RowResult>& res)
{
    std::ofstream out;
    create_file(outdir + "/read_alleles.tsv", out);
    out << "Read\tClusterId\tAlleles\n";
    for (size_t y = 0; y < rows.kept.size(); ++y) {
        const ReadStatRow& r = rows.row(y);
        out.write(r.id, std::streamsize(r.id_len));
        out << '\t' << r.cls << '\t' << res[y].alleles << '\n';
    }
}

void write_read_split(const string& outdir, const ReportRows& rows, const std::vector<RowResult>& res)
{
    std::ofstream out;
    create_file(outdir + "/read_split.tsv", out);
    out << "Read\tClusterId\tGroup\tVote\n";
    for (size_t y = 0; y < rows.kept.size(); ++y) {
        const ReadStatRow& r = rows.row(y);
        out.write(r.id, std::streamsize(r.id_len));
        out << '\t' << r.cls << '\t' << (res[y].group == 0 ? "0" : res[y].group == 1 ? "1" : ".") << '\t' << res[y].vote << '\n';
    }
}

void write_read_isoforms(const string& outdir, const ReportRows& rows, const std::vector<RowResult>& res)
{
    std::ofstream out;
    create_file(outdir + "/read_isoforms.tsv", out);
    out << "ClusterId\tRead\tIsoform\tHow\tSignature\tFirst\tEnd\tGaps\tGapRows\n";
    for (size_t y = 0; y < rows.kept.size(); ++y) {
        const ReadStatRow& r = rows.row(y);
        out << r.cls << '\t';
        out.write(r.id, std::streamsize(r.id_len));
        out << '\t' << read_isoform_columns(res[y].iso, res[y].iso_blocks) << '\n';
    }
}

void write_read_inserts(const string& outdir, const ReportRows& rows, const std::vector<RowResult>& res)
{
    std::ofstream out;
    create_file(outdir + "/read_inserts.tsv", out);
    out << "ClusterId\tRead\tInserts\tIsoform\tHow\n";
    for (size_t y = 0; y < rows.kept.size(); ++y) {
        const ReadStatRow& r = rows.row(y);
        out << r.cls << '\t';
        out.write(r.id, std::streamsize(r.id_len));
        out << '\t' << read_insert_columns(res[y].ins, res[y].ins_sites) << '\n';
    }
}

// read_insert_variants.tsv: one row per row read_inserts.tsv has, in that order
void write_read_insert_variants(const string& outdir, const ReportRows& rows, const std::vector<RowResult>& res)
{
    std::ofstream out;
    create_file(outdir + "/read_insert_variants.tsv", out);
    out << "ClusterId\tRead\tVariants\tInserts\tIsoform\tHow\n";
    for (size_t y = 0; y < rows.kept.size(); ++y) {
        const ReadStatRow& r = rows.row(y);
        out << r.cls << '\t';
        out.write(r.id, std::streamsize(r.id_len));
        out << '\t' << (res[y].variants.empty() ? string("*") : res[y].variants) << '\t' << read_variant_columns(res[y].var, res[y].ins_sites) << '\n';
    }
}

void write_read_ends(const string& outdir, const ReportRows& rows, const std::vector<RowResult>& res)
{
    std::ofstream out;
    create_file(outdir + "/read_ends.tsv", out);
    out << "Read\tClusterId\tFirstRow\tEndRow\tHead\tTail\tStartSite\tStopSite\tVariant\n";
    for (size_t y = 0; y < rows.kept.size(); ++y) {
        const ReadStatRow& r = rows.row(y);
        out.write(r.id, std::streamsize(r.id_len));
        out << '\t' << r.cls << '\t' << read_end_columns(res[y].extent, res[y].ends) << '\n';
    }
}

void write_corrected_reads(const string& outdir, const std::vector<RowResult>& res)
{
    std::ofstream out;
    create_file(outdir + "/corrected_reads.fq", out);
    for (const RowResult& r : res) out.write(r.corrected.data(), std::streamsize(r.corrected.size()));
}

// corrected_reads_isoforms.fq: one record per row of clusters.tsv, in that order
void write_iso_corrected_reads(const string& outdir, const std::vector<RowResult>& res)
{
    std::ofstream out;
    create_file(outdir + "/corrected_reads_isoforms.fq", out);
    for (const RowResult& r : res) out.write(r.iso_corrected.data(), std::streamsize(r.iso_corrected.size()));
}

void write_read_stats(const string& outdir, const ReportRows& rows, const std::vector<RowResult>& res)
{
    std::ofstream out;
    create_file(outdir + "/read_stats.tsv", out);
    out << "ClusterId\tStrand\tRead\tReadLen\tRepLen\tScore\tWindows\tColumns\tMatches\tMismatches\tIns\tDel\tInsRuns\tDelRuns\tLongestIns\tLongestDel\t"
           "ReadStart\tReadEnd\tRepStart\tRepEnd\tIdentity\n";
    for (size_t y = 0; y < rows.kept.size(); ++y) {
        const ReadStatRow& r = rows.row(y);
        const RowResult& a = res[y];
        const ioc_aln_stats& s = a.st;
        char ident[32];
        snprintf(ident, sizeof ident, "%.6f", s.columns > 0 ? double(s.matches) / double(s.columns) : 0.0);
        out << r.cls << '\t' << r.strand << '\t';
        out.write(r.id, std::streamsize(r.id_len));
        out << '\t' << r.seq_len << '\t' << a.rep_len << '\t' << a.score << '\t' << a.windows << '\t' << s.columns << '\t' << s.matches << '\t' << s.mismatches
            << '\t' << s.ins << '\t' << s.del << '\t' << s.ins_runs << '\t' << s.del_runs << '\t' << s.longest_ins << '\t' << s.longest_del << '\t' << s.lead_i
            << '\t' << int64_t(r.seq_len) - s.trail_i << '\t' << s.lead_d << '\t' << int64_t(a.rep_len) - s.trail_d << '\t' << ident << '\n';
    }
}

}  // namespace

void write_read_reports(const Batch& b, const string& outdir, const std::vector<ReadStatRow>& all_rows, const ReportOpts& opts)
{
    const int k = b.SortArgs.KmerSize;
    const ReportRows rows = keep_report_rows(b, all_rows);
    std::vector<RowResult> res(rows.kept.size());
    ioc_ctx* c = rows.kept.empty() ? nullptr : make_ctx();
    GroupFiles files(outdir, opts);
    GroupResult result;
    plan_report_groups(b, rows, opts, [&](ReportGroup& g) {
        if (!g.pairs.empty()) {
            align_group(c, k, opts, g, result);
            scatter_to_rows(opts, rows, g, result, res);
        }
        if (opts.groups()) files.write(b, opts, rows, g, result);
    });
    if (c) ioc_ctx_destroy(c);
    if (opts.sites.on) write_read_alleles(outdir, rows, res);
    if (opts.split.on) write_read_split(outdir, rows, res);
    if (opts.stats) write_read_stats(outdir, rows, res);
    if (opts.correct.on) write_corrected_reads(outdir, res);
    if (opts.isoforms.on && opts.isoforms.correct) write_iso_corrected_reads(outdir, res);
    if (opts.isoforms.on) write_read_isoforms(outdir, rows, res);
    if (opts.isoforms.on && opts.isoforms.inserts) write_read_inserts(outdir, rows, res);
    if (opts.isoforms.on && opts.isoforms.inserts && opts.isoforms.variants) write_read_insert_variants(outdir, rows, res);
    if (opts.isoforms.on && opts.isoforms.ends) write_read_ends(outdir, rows, res);
}
