// dump  (src/main.cpp:204-236, 430-453; src/output.cpp:151-275); the read reports beyond the reference's files: reports.cpp
#include <getopt.h>

#include <atomic>
#include <cerrno>
#include <climits>
#include <cstring>
#include <iostream>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "reports.hpp"

using namespace cer;
using std::cerr;
using std::endl;
using std::string;

namespace {

struct DumpOptions {
    string outdir, index, batch;
    // --read-stats: read_stats.tsv, every read aligned against its cluster's representative (on the GPU)
    // --pileup: cluster_pileup.tsv, the same alignments piled onto the representative position by position
    // --polish: cluster_polished.fq, every representative called anew from both pileup tables of its reads
    // --polish-min-depth: positions covered by fewer reads keep the representative's base
    // --polish-weighted: the call of --polish with every read's vote weighted by its base quality
    // --sites: cluster_sites.tsv and read_alleles.tsv, where the reads of a cluster disagree and which read says what there
    // --split: cluster_split.tsv and read_split.tsv, the reads of a cluster in two groups by its linked sites
    // --split-polish: cluster_split_polished.fq, the consensus of each group of every cluster that has a split
    // --split-polish-min-depth: positions covered by fewer reads of the group keep the representative's base
    // --correct: corrected_reads.fq, every read corrected against the pileup of its cluster; --correct-*: its thresholds
    // --isoforms: cluster_blocks.tsv, cluster_isoforms.tsv, read_isoforms.tsv, the exon blocks of a cluster and every read's isoform; --isoforms-*
    // --isoforms-polish: cluster_isoforms.fq, the consensus of every isoform of every cluster that has a block
    // --isoforms-polish-min-depth / --isoforms-polish-max: positions covered by fewer reads of the isoform keep the representative's base / the isoforms called per cluster
    // --isoforms-polish-weighted: every isoform is called by weight, every read voting with its base qualities
    // --isoforms-inserts: cluster_inserts.tsv, read_inserts.tsv, the exons a cluster's reads carry and its representative lacks, and isoforms over blocks and sites
    // --isoforms-correct: corrected_reads_isoforms.fq, every read corrected against the tables of its own isoform, long insertions carried through
    // --isoforms-ends: cluster_ends.tsv, cluster_end_variants.tsv, read_ends.tsv, where the reads of a cluster start and stop on its representative, and the variants
    ReportOpts reports;
};

// a whole number of [lo, hi], or the end of the run
int number(const char* name, const char* text, long lo, long hi)
{
    char* end = nullptr;
    errno = 0;
    const long v = strtol(text, &end, 10);
    if (errno != 0 || end == text || *end != '\0' || v < lo || v > hi)
        die(string(name) + " must be a whole number" + (hi < INT32_MAX ? " from " + std::to_string(lo) + " to " + std::to_string(hi) : " of at least " + std::to_string(lo)) + "!");
    return int(v);
}

void print_dump_help()
{
    cerr << "isONclust2-hip dump -i sorted_reads_idx.cer -o outdir [--read-stats] [--pileup] [--polish [--polish-min-depth N] [--polish-weighted]]" << endl
         << "                    [--sites [--sites-min-depth N] [--sites-min-alt N] [--sites-min-pct P] [--sites-max N]]" << endl
         << "                    [--split [--split-min-link N] [--split-min-margin N] [--split-rounds N]" << endl
         << "                     [--split-polish [--split-polish-min-depth N]]]" << endl
         << "                    [--correct [--correct-min-depth N] [--correct-min-alt N] [--correct-min-pct P] [--correct-max-run N]]" << endl
         << "                    [--isoforms [--isoforms-min-gap N] [--isoforms-min-depth N] [--isoforms-min-alt N] [--isoforms-min-pct P]" << endl
         << "                     [--isoforms-min-block N] [--isoforms-max N]" << endl
         << "                     [--isoforms-polish [--isoforms-polish-min-depth N] [--isoforms-polish-max N] [--isoforms-polish-weighted]]" << endl
         << "                     [--isoforms-inserts [--isoforms-min-ins N] [--isoforms-ins-slack N] [--isoforms-ins-max N]" << endl
         << "                     [--isoforms-inserts-seq [--isoforms-inserts-max-win N] [--isoforms-full [--isoforms-full-max N]]" << endl
         << "                      [--isoforms-inserts-variants [--isoforms-inserts-variants-min-agree N] [--isoforms-full-variants]]]]" << endl
         << "                     [--isoforms-ends [--isoforms-ends-slack N] [--isoforms-ends-min-over N] [--isoforms-ends-min-pct P]" << endl
         << "                     [--isoforms-ends-max N] [--isoforms-ends-max-variants N]]" << endl
         << "                     [--isoforms-correct]] final.cer" << endl
         << "  --read-stats   also write outdir/read_stats.tsv: every read of clusters.tsv aligned against its cluster's representative" << endl
         << "                 as cluster_cons.fq has it (GPU): score, windows, identity, gaps and where the alignment begins and ends" << endl
         << "  --pileup       also write outdir/cluster_pileup.tsv: per position of every representative of cluster_cons.fq, how many reads of" << endl
         << "                 its cluster cover it, the bases they have there, deletions, and insertions in front of it (GPU)" << endl
         << "  --polish       also write outdir/cluster_polished.fq: one record per record of cluster_cons.fq, the majority call over the" << endl
         << "                 cluster's reads aligned against it — substitutions, deletions and insertions of up to 6 bases (GPU);" << endl
         << "                 header: reads, and how many positions were substituted, deleted, inserted or left as they were" << endl
         << "  --polish-min-depth N   positions covered by fewer than N reads keep the representative's base, quality '!' (default 3)" << endl
         << "  --polish-weighted      with --polish: every read votes with its base qualities (Phred, 1 .. 93) instead of 1, so that" << endl
         << "                 a few confident reads outvote many doubtful ones; min-depth still counts reads; header: weighted=1" << endl
         << "  --sites        also write outdir/cluster_sites.tsv, the positions of every representative where a second allele has real" << endl
         << "                 support among the cluster's reads (a base, a deletion, an insertion in front of the position), and" << endl
         << "                 outdir/read_alleles.tsv, every read's allele at each of its cluster's sites, one character per site (GPU);" << endl
         << "                 with --read-stats / --pileup the reads are still aligned once, with --polish a second time" << endl
         << "  --sites-min-depth N    only positions covered by at least N reads can be sites (default 3)" << endl
         << "  --sites-min-alt N      the second allele needs at least N reads (default 3) ..." << endl
         << "  --sites-min-pct P      ... and at least P percent of the depth, 1 .. 50 (default 25)" << endl
         << "  --sites-max N          keep the first N sites of a cluster (default 4096); a cluster with more gets a '#' line" << endl
         << "  --split        also write outdir/cluster_split.tsv, per cluster how many of its sites (found under the --sites-* thresholds) vary" << endl
         << "                 together and how many reads stand on either side of that pattern, and outdir/read_split.tsv, every read's" << endl
         << "                 group (0 | 1 | .) and vote (GPU); whether a cluster is one thing or two is the reader's judgement of the counts" << endl
         << "  --split-min-link N     two sites are linked when their reads agree or disagree by at least N (default 3)" << endl
         << "  --split-min-margin N   a read joins a group when its vote is at least N on that side (default 1)" << endl
         << "  --split-rounds N       refinement rounds, 0 .. 64, which carry the split along a representative no read spans (default 2)" << endl
         << "  --split-polish         with --split: also write outdir/cluster_split_polished.fq, for every cluster that has a split the" << endl
         << "                 consensus of each group that has reads (records <cluster>/0 and <cluster>/1), called from the alignments" << endl
         << "                 of --split: no read is aligned again" << endl
         << "  --split-polish-min-depth N   positions covered by fewer than N reads of the group keep the representative's base (default 3)" << endl
         << "  --correct      also write outdir/corrected_reads.fq: every read of clusters.tsv with the part that aligns against its cluster's" << endl
         << "                 representative corrected by the cluster's reads (GPU): a base, a deletion or an inserted base that enough reads" << endl
         << "                 share is kept (a cluster holds a gene: haplotypes and isoforms keep what is theirs), anything else becomes what" << endl
         << "                 most reads say; the unaligned ends stay as they are; qualities: 40 x the share of the cluster's reads that" << endl
         << "                 support the base, '!' where too few reads cover it; header: cluster, and how many positions were substituted," << endl
         << "                 filled, removed, inserted, dropped, left for low depth, or held back by --correct-max-run.  A read whose" << endl
         << "                 alignment inserts more than 6 bases in a row is written as it is, with uncorrected=long_insertion." << endl
         << "                 The correction is a call of its own: beside --polish, --sites or --split the reads are aligned once more" << endl
         << "                 for it (beside --read-stats and --pileup alone they are aligned once)" << endl
         << "  --correct-min-depth N  positions covered by fewer than N reads are left as the read has them (default 3)" << endl
         << "  --correct-min-alt N    what a read says is kept when at least N reads say it (default 3) ..." << endl
         << "  --correct-min-pct P    ... and at least P percent of the depth, 1 .. 50 (default 25)" << endl
         << "  --correct-max-run N    a run of more than N deleted positions in a row is not filled in, and one of more than N bases is not" << endl
         << "                 removed, 0 .. 64 (default 10: a choice — sequencing indels are short, a missing exon is not — that was not" << endl
         << "                 measured on real data)" << endl
         << "  --isoforms     also write outdir/cluster_blocks.tsv, cluster_isoforms.tsv and read_isoforms.tsv (GPU): the stretches of a cluster's" << endl
         << "                 representative that some of its reads skip (exon blocks: first, end, and how many reads keep, skip, partly skip" << endl
         << "                 or do not reach each; a '#' line where a cluster's list was cut), the signatures that enough complete reads carry" << endl
         << "                 (one character per block: '=' keep, '-' skip, '~' part) with their reads, and per read its isoform (or '.')," << endl
         << "                 whether it carries the signature itself (direct), fits exactly one (assigned), carries one too few reads share" << endl
         << "                 (rare) or fits none or several (ambiguous), its own signature ('.' where it does not reach across a block), the" << endl
         << "                 representative's positions it covers and its long gaps.  An exon the representative lacks is not found.  The" << endl
         << "                 report is a call of its own: beside --polish, --sites, --split or --correct the reads are aligned once more for it" << endl
         << "  --isoforms-min-gap N    a run of at least N deleted positions in a row is a long gap (default 20: a choice that was not" << endl
         << "                 measured on real data)" << endl
         << "  --isoforms-min-depth N  positions covered by fewer than N reads are not variable (default 3)" << endl
         << "  --isoforms-min-alt N    a position is variable when at least N reads have a long gap there and N have none, and a signature" << endl
         << "                 is an isoform when at least N complete reads carry it (default 3) ..." << endl
         << "  --isoforms-min-pct P    ... and at least P percent of the depth either way, 1 .. 50 (default 25)" << endl
         << "  --isoforms-min-block N  a run of at least N variable positions is a block (default 10: a choice that was not measured on" << endl
         << "                 real data)" << endl
         << "  --isoforms-max N        keep the first N blocks of a cluster, 1 .. 32 (default 32)" << endl
         << "  --isoforms-polish       with --isoforms: also write outdir/cluster_isoforms.fq, for every cluster that has a block the consensus" << endl
         << "                 of each of its isoforms (records <cluster>/iso<n>, with the isoform's signature as key=), called from the" << endl
         << "                 alignments of --isoforms over the isoform's direct and assigned reads: no read is aligned again.  An isoform" << endl
         << "                 keeps the representative's coordinates: a skipped block is a deletion, an exon the representative lacks is" << endl
         << "                 not found.  Whether an isoform is real is the reader's judgement of the counts" << endl
         << "  --isoforms-polish-min-depth N   positions covered by fewer than N reads of the isoform keep the representative's base (default 3)" << endl
         << "  --isoforms-polish-max N         call the first N isoforms of a cluster (default 16: a choice — it bounds what a cluster may" << endl
         << "                 write before its isoforms are known — that was not measured on real data)" << endl
         << "  --isoforms-polish-weighted      with --isoforms-polish: call every isoform by weight — every read votes with the base qualities of" << endl
         << "                 its line (Phred, 1 .. 93), a deletion with the smaller of its neighbours'; the depth gates stay counts of reads." << endl
         << "                 The same records of cluster_isoforms.fq, names and order; still no read is aligned again" << endl
         << "  --isoforms-inserts      with --isoforms: also write outdir/cluster_inserts.tsv and read_inserts.tsv, from the same alignments: the" << endl
         << "                 places where some reads carry an exon the representative lacks (insertion sites: the first junction and one" << endl
         << "                 past the last, how many reads carry an insertion there, lack it or do not reach across, and the shortest and" << endl
         << "                 longest insertion of the carriers; a '#' line where a cluster's list was cut), and per read its signature at the" << endl
         << "                 sites ('=' lack, '+' carry, '.' not across), its isoform counted over blocks AND sites together (or '.') and how" << endl
         << "                 it got it, as in read_isoforms.tsv.  The three files of --isoforms stay what they are.  The sequence of an" << endl
         << "                 inserted exon: --isoforms-inserts-seq.  Not offered together with --isoforms-polish: the isoforms' consensus" << endl
         << "                 is called over the blocks alone" << endl
         << "  --isoforms-inserts-seq  with --isoforms-inserts: also write outdir/cluster_inserts.fq, from the same alignments: per site that has a" << endl
         << "                 voter a record \"cluster_<id>/ins<b> rows=<lo>-<hi> voters=<n> template=<read>\", the consensus of what the carriers" << endl
         << "                 hold between rows lo and hi of the representative (the site widened by --isoforms-ins-slack, in the orientation the" << endl
         << "                 reads were aligned in), to stand in place of those rows.  All carriers of a site vote together" << endl
         << "  --isoforms-inserts-max-win N  a carrier votes where its stretch between the two rows has at most N bases, 1 .. 512 (default 512)" << endl
         << "  --isoforms-inserts-variants  with --isoforms-inserts-seq: also write outdir/cluster_insert_variants.fq and read_insert_variants.tsv, from the" << endl
         << "                 same alignments: where the voters of a site hold two different exons (mutually exclusive exons) they are split in two," << endl
         << "                 and per called variant there is a record \"cluster_<id>/ins<b>/<A|B> rows=<lo>-<hi> voters=<n> template=<read> split=<0|1>\"," << endl
         << "                 variant A being the one of the site's template; per read its variant at every site ('A', 'B', 'o' a voter near neither," << endl
         << "                 '.' no voter), its signature with the variants told apart ('=' lack, 'A' / 'B' carry, '.' not across or unknown) and its" << endl
         << "                 isoform counted again over blocks and sites.  The files that exist stay what they are.  Not offered together with" << endl
         << "                 --isoforms-full: the splice reads one window a site (--isoforms-full-variants splices each variant's own)" << endl
         << "  --isoforms-inserts-variants-min-agree N  a voter is near a template where matches minus mismatches minus gaps of its alignment reach N" << endl
         << "                 percent of the longer of the two, 1 .. 100 (default 45: a choice made on simulated windows at 8 % errors, not measured on" << endl
         << "                 real data; exons under about 40 bases and reads beyond about 10 % errors are outside what it separates)" << endl
         << "  --isoforms-full         with --isoforms-inserts-seq: also write outdir/cluster_isoforms_full.fq, from the same alignments: for every cluster" << endl
         << "                 that has a block or a site, a record per isoform counted over blocks and sites together, \"cluster_<id>/iso<h>" << endl
         << "                 key=<blocks>/<sites> reads=<n> subs= dels= ins= low= [ins<b>@<at>+<len> ..]\": the consensus of the isoform's reads in the" << endl
         << "                 representative's frame with, for every site the isoform carries, the site's record of cluster_inserts.fq in place of" << endl
         << "                 the rows it stands for (len bases from base at on) - the isoform's full-length sequence" << endl
         << "  --isoforms-full-max N   call the first N isoforms of a cluster (default 16)" << endl
         << "  --isoforms-full-variants  with --isoforms-inserts-variants: also write outdir/cluster_isoforms_full_variants.fq, from the same alignments:" << endl
         << "                 the records of cluster_isoforms_full.fq for the isoforms counted again over the variants, the sites half of key= in the" << endl
         << "                 letters of read_insert_variants.tsv ('=', 'A', 'B', '.'), and every site the isoform carries as ins<b>/<A|B>@<at>+<len>:" << endl
         << "                 the record of cluster_insert_variants.fq that stands there - two exons at one junction, each in its own transcript." << endl
         << "                 --isoforms-full-max applies.  Not offered together with --isoforms-full: one fused call a run" << endl
         << "  --isoforms-min-ins N    a read carries an insertion at a junction where the bases it inserts within --isoforms-ins-slack junctions" << endl
         << "                 sum to at least N, 1 .. 255 (default 20: a choice that was not measured on real data)" << endl
         << "  --isoforms-ins-slack N  ... the junctions on either side that count, 0 .. 32 (default 8: at 8 % errors the aligner breaks a 40-base" << endl
         << "                 exon into two runs a few positions apart; a choice that was not measured on real data)" << endl
         << "  --isoforms-ins-max N    keep the first N insertion sites of a cluster, 1 .. 32 (default 32)" << endl
         << "  --isoforms-ends         with --isoforms: also write outdir/cluster_ends.tsv, cluster_end_variants.tsv and read_ends.tsv, from the same" << endl
         << "                 alignments: where the reads of a cluster start and stop on its representative (start and stop sites: the first row" << endl
         << "                 and one past the last, the row most reads use and how many, the reads of the site and how many of them go on beyond" << endl
         << "                 the representative there; a '#' line where a list was cut), the (isoform, start site, stop site) triples that at" << endl
         << "                 least --isoforms-min-alt reads carry (variants), and per read the rows it covers, the bases it has in front of and" << endl
         << "                 behind its alignment, its start site, its stop site and its variant (or '.').  A start site at row 0 whose reads" << endl
         << "                 mostly go on says the representative is the short one.  Two ends closer than about twice the slack are one site." << endl
         << "                 The three files of --isoforms stay what they are.  Not offered together with --isoforms-inserts or" << endl
         << "                 --isoforms-polish: one fused call a run" << endl
         << "  --isoforms-ends-slack N         reads that start (stop) within N rows of each other share a site, 0 .. 32 (default 10: a choice that" << endl
         << "                 was not measured on real data)" << endl
         << "  --isoforms-ends-min-over N      a read goes on beyond the representative where it has at least N unaligned bases there (default 20)" << endl
         << "  --isoforms-ends-min-pct P       a site needs at least P percent of the cluster's reads, 1 .. 100 (default 10), and --isoforms-min-alt reads" << endl
         << "  --isoforms-ends-max N           keep the first N start sites and the first N stop sites of a cluster, 1 .. 32 (default 32)" << endl
         << "  --isoforms-ends-max-variants N  keep the first N variants of a cluster (default 64)" << endl
         << "  --isoforms-correct      with --isoforms: also write outdir/corrected_reads_isoforms.fq, from the same alignments: every read of" << endl
         << "                 clusters.tsv corrected as --correct corrects it, but against the reads of its own isoform (read_isoforms.tsv) where" << endl
         << "                 that has at least --correct-min-depth reads, else against its whole cluster; an insertion of more than 6 bases in a" << endl
         << "                 row — an exon the representative lacks — is carried through as the read has it, at quality '!', while the rest of" << endl
         << "                 the read is corrected.  The header has --correct's counters and isoform=<h or ->, table=<isoform|cluster>," << endl
         << "                 long_runs= and long_bases=; a read whose insertion cannot be placed is written as it is, with" << endl
         << "                 uncorrected=unresolved_insertion.  The thresholds are --correct-*'s; --correct itself is not needed and stays" << endl
         << "                 what it is.  Not offered together with --isoforms-inserts, --isoforms-ends or --isoforms-polish: one fused" << endl
         << "                 call a run" << endl;
}

DumpOptions parse_dump_options(int argc, char** argv)
{
    static const struct option lo[] = {{"verbose", no_argument, 0, 'v'}, {"debug", no_argument, 0, 'd'}, {"help", no_argument, 0, 'h'},
                                       {"outdir", required_argument, 0, 'o'}, {"index", required_argument, 0, 'i'},
                                       {"read-stats", no_argument, 0, 1000}, {"pileup", no_argument, 0, 1001},
                                       {"polish", no_argument, 0, 1002}, {"polish-min-depth", required_argument, 0, 1003},
                                       {"polish-weighted", no_argument, 0, 1004}, {"sites", no_argument, 0, 1005},
                                       {"sites-min-depth", required_argument, 0, 1006}, {"sites-min-alt", required_argument, 0, 1007},
                                       {"sites-min-pct", required_argument, 0, 1008}, {"sites-max", required_argument, 0, 1009},
                                       {"split", no_argument, 0, 1010}, {"split-min-link", required_argument, 0, 1011},
                                       {"split-min-margin", required_argument, 0, 1012}, {"split-rounds", required_argument, 0, 1013},
                                       {"split-polish", no_argument, 0, 1014}, {"split-polish-min-depth", required_argument, 0, 1015},
                                       {"correct", no_argument, 0, 1016}, {"correct-min-depth", required_argument, 0, 1017},
                                       {"correct-min-alt", required_argument, 0, 1018}, {"correct-min-pct", required_argument, 0, 1019},
                                       {"correct-max-run", required_argument, 0, 1020},
                                       {"isoforms", no_argument, 0, 1021}, {"isoforms-min-gap", required_argument, 0, 1022},
                                       {"isoforms-min-depth", required_argument, 0, 1023}, {"isoforms-min-alt", required_argument, 0, 1024},
                                       {"isoforms-min-pct", required_argument, 0, 1025}, {"isoforms-min-block", required_argument, 0, 1026},
                                       {"isoforms-max", required_argument, 0, 1027}, {"isoforms-polish", no_argument, 0, 1028},
                                       {"isoforms-polish-min-depth", required_argument, 0, 1029}, {"isoforms-polish-max", required_argument, 0, 1030},
                                       {"isoforms-polish-weighted", no_argument, 0, 1031}, {"isoforms-inserts", no_argument, 0, 1032},
                                       {"isoforms-min-ins", required_argument, 0, 1033}, {"isoforms-ins-slack", required_argument, 0, 1034},
                                       {"isoforms-ins-max", required_argument, 0, 1035}, {"isoforms-inserts-seq", no_argument, 0, 1036},
                                       {"isoforms-inserts-max-win", required_argument, 0, 1037}, {"isoforms-full", no_argument, 0, 1038},
                                       {"isoforms-full-max", required_argument, 0, 1039}, {"isoforms-ends", no_argument, 0, 1040},
                                       {"isoforms-ends-slack", required_argument, 0, 1041}, {"isoforms-ends-min-over", required_argument, 0, 1042},
                                       {"isoforms-ends-min-pct", required_argument, 0, 1043}, {"isoforms-ends-max", required_argument, 0, 1044},
                                       {"isoforms-ends-max-variants", required_argument, 0, 1045}, {"isoforms-inserts-variants", no_argument, 0, 1046},
                                       {"isoforms-inserts-variants-min-agree", required_argument, 0, 1047},
                                       {"isoforms-full-variants", no_argument, 0, 1048}, {"isoforms-correct", no_argument, 0, 1049}, {0, 0, 0, 0}};
    DumpOptions d;
    ReportOpts& r = d.reports;
    bool polish = false, split_polish = false, iso_polish = false;
    int polish_min_depth = 3, split_polish_min_depth = 3, iso_polish_min_depth = 3;
    int o;
    while ((o = getopt_long(argc, argv, "dhvo:i:", lo, nullptr)) != -1) {
        switch (o) {
            case 'o': d.outdir = optarg; break;
            case 'i': d.index = optarg; break;
            case 'v': VERBOSE = true; break;
            case 1000: r.stats = true; break;
            case 1001: r.pileup = true; break;
            case 1002: polish = true; break;
            case 1003: polish_min_depth = atoi(optarg); break;
            case 1004: r.polish_weighted = true; break;
            case 1005: r.sites.on = true; break;
            case 1006: r.sites.min_depth = number("--sites-min-depth", optarg, 1, INT32_MAX); break;
            case 1007: r.sites.min_alt = number("--sites-min-alt", optarg, 1, INT32_MAX); break;
            case 1008: r.sites.min_pct = number("--sites-min-pct", optarg, 1, 50); break;
            case 1009: r.sites.max_sites = number("--sites-max", optarg, 1, INT32_MAX); break;
            case 1010: r.split.on = true; break;
            case 1011: r.split.min_link = number("--split-min-link", optarg, 1, INT32_MAX); break;
            case 1012: r.split.min_margin = number("--split-min-margin", optarg, 1, INT32_MAX); break;
            case 1013: r.split.rounds = number("--split-rounds", optarg, 0, 64); break;
            case 1014: split_polish = true; break;
            case 1015: split_polish_min_depth = number("--split-polish-min-depth", optarg, 1, INT32_MAX); break;
            case 1016: r.correct.on = true; break;
            case 1017: r.correct.min_depth = number("--correct-min-depth", optarg, 1, INT32_MAX); break;
            case 1018: r.correct.min_alt = number("--correct-min-alt", optarg, 1, INT32_MAX); break;
            case 1019: r.correct.min_pct = number("--correct-min-pct", optarg, 1, 50); break;
            case 1020: r.correct.max_run = number("--correct-max-run", optarg, 0, 64); break;
            case 1021: r.isoforms.on = true; break;
            case 1022: r.isoforms.min_gap = number("--isoforms-min-gap", optarg, 1, INT32_MAX); break;
            case 1023: r.isoforms.min_depth = number("--isoforms-min-depth", optarg, 1, INT32_MAX); break;
            case 1024: r.isoforms.min_alt = number("--isoforms-min-alt", optarg, 1, INT32_MAX); break;
            case 1025: r.isoforms.min_pct = number("--isoforms-min-pct", optarg, 1, 50); break;
            case 1026: r.isoforms.min_block = number("--isoforms-min-block", optarg, 1, INT32_MAX); break;
            case 1027: r.isoforms.max_blocks = number("--isoforms-max", optarg, 1, 32); break;
            case 1028: iso_polish = true; break;
            case 1029: iso_polish_min_depth = number("--isoforms-polish-min-depth", optarg, 1, INT32_MAX); break;
            case 1030: r.isoforms.polish_max = number("--isoforms-polish-max", optarg, 1, INT32_MAX); break;
            case 1031: r.isoforms.polish_weighted = true; break;
            case 1032: r.isoforms.inserts = true; break;
            case 1033: r.isoforms.min_ins = number("--isoforms-min-ins", optarg, 1, 255); break;
            case 1034: r.isoforms.ins_slack = number("--isoforms-ins-slack", optarg, 0, 32); break;
            case 1035: r.isoforms.ins_max = number("--isoforms-ins-max", optarg, 1, 32); break;
            case 1036: r.isoforms.inserts_seq = true; break;
            case 1037: r.isoforms.ins_max_win = number("--isoforms-inserts-max-win", optarg, 1, IOC_WIN_MAX); break;
            case 1038: r.isoforms.full = true; break;
            case 1039: r.isoforms.full_max = number("--isoforms-full-max", optarg, 1, INT32_MAX); break;
            case 1040: r.isoforms.ends = true; break;
            case 1041: r.isoforms.ends_slack = number("--isoforms-ends-slack", optarg, 0, IOC_ENDS_SLACK_MAX); break;
            case 1042: r.isoforms.ends_min_over = number("--isoforms-ends-min-over", optarg, 1, INT32_MAX); break;
            case 1043: r.isoforms.ends_min_pct = number("--isoforms-ends-min-pct", optarg, 1, 100); break;
            case 1044: r.isoforms.ends_max = number("--isoforms-ends-max", optarg, 1, IOC_ENDS_MAX); break;
            case 1045: r.isoforms.ends_max_variants = number("--isoforms-ends-max-variants", optarg, 1, INT32_MAX); break;
            case 1046: r.isoforms.variants = true; break;
            case 1047: r.isoforms.variants_min_agree = number("--isoforms-inserts-variants-min-agree", optarg, 1, 100); break;
            case 1048: r.isoforms.full_variants = true; break;
            case 1049: r.isoforms.correct = true; break;
            case 'h': print_dump_help(); exit(0);
            default: break;
        }
    }
    if (optind >= argc) die("No input batch specified!");
    if (d.outdir.empty()) die("Specifying output directory is mandatory!");
    if (polish && polish_min_depth < 1) die("--polish-min-depth must be at least 1!");
    if (r.polish_weighted && !polish) die("--polish-weighted asks for --polish!");
    if (split_polish && !r.split.on) die("--split-polish asks for --split!");
    if (split_polish) r.split.polish_min_depth = split_polish_min_depth;
    if (iso_polish && !r.isoforms.on) die("--isoforms-polish asks for --isoforms!");
    if (r.isoforms.polish_weighted && !iso_polish) die("--isoforms-polish-weighted asks for --isoforms-polish!");
    if (iso_polish) r.isoforms.polish_min_depth = iso_polish_min_depth;
    if (r.isoforms.inserts && !r.isoforms.on) die("--isoforms-inserts asks for --isoforms!");
    if (r.isoforms.inserts && iso_polish) die("--isoforms-inserts is not offered together with --isoforms-polish!");
    if (r.isoforms.inserts_seq && !r.isoforms.inserts) die("--isoforms-inserts-seq asks for --isoforms-inserts!");
    if (r.isoforms.full && !r.isoforms.inserts_seq) die("--isoforms-full asks for --isoforms-inserts-seq!");
    if (r.isoforms.variants && !r.isoforms.inserts_seq) die("--isoforms-inserts-variants asks for --isoforms-inserts-seq!");
    if (r.isoforms.full_variants && r.isoforms.full) die("--isoforms-full-variants is not offered together with --isoforms-full: one fused call a run!");
    if (r.isoforms.variants && r.isoforms.full) die("--isoforms-inserts-variants is not offered together with --isoforms-full!");
    if (r.isoforms.full_variants && !r.isoforms.variants) die("--isoforms-full-variants asks for --isoforms-inserts-variants!");
    if (r.isoforms.ends && !r.isoforms.on) die("--isoforms-ends asks for --isoforms!");
    if (r.isoforms.ends && r.isoforms.inserts) die("--isoforms-ends is not offered together with --isoforms-inserts!");
    if (r.isoforms.ends && iso_polish) die("--isoforms-ends is not offered together with --isoforms-polish!");
    if (r.isoforms.correct && !r.isoforms.on) die("--isoforms-correct asks for --isoforms!");
    if (r.isoforms.correct && r.isoforms.inserts) die("--isoforms-correct is not offered together with --isoforms-inserts: one fused call a run!");
    if (r.isoforms.correct && r.isoforms.ends) die("--isoforms-correct is not offered together with --isoforms-ends: one fused call a run!");
    if (r.isoforms.correct && iso_polish) die("--isoforms-correct is not offered together with --isoforms-polish: one fused call a run!");
    if (polish) r.polish_min_depth = polish_min_depth;
    if (d.index.empty()) die("Specifying the sorted read index is mandatory!");
    d.batch = argv[optind];
    return d;
}

void write_batch_info(const string& outdir, const Batch& b)
{
    std::ofstream bi;
    create_file(outdir + "/batch_info.tsv", bi);
    int ncls = 0, nnt = 0;
    for (auto& c : b.Cls)
        if (c->at(0)->RawSeq && c->at(0)->RawSeq->score > -1) {
            ncls++;
            nnt += c->size() > 2;
        }
    bi << "Name\tValue\nBatchNumber\t" << b.BatchNr << "\nBatchStart\t" << b.BatchStart << "\nBatchEnd\t" << b.BatchEnd << "\nDepth\t"
       << b.Depth << "\nNrBases\t" << b.BatchBases << "\nNrClusters\t" << ncls << "\nNrNontrivialCls\t" << nnt << "\nMinDBsize\t0\n";
}

struct IdInfo {
    unsigned cls;
    int strand;
};
typedef std::unordered_map<string, IdInfo> IdMap;

// clusters_info.tsv, the cluster_fastq directory, and every read id's cluster and strand
IdMap write_clusters_info(const string& outdir, const Batch& b)
{
    IdMap id2cls;
    std::ofstream info;
    create_file(outdir + "/clusters_info.tsv", info);
    create_outdir(outdir + "/cluster_fastq");
    info << "ClusterId\tSize" << endl;
    unsigned i = 0;
    for (auto& cl : b.Cls) {
        info << i << "\t" << cl->size() - 1 << endl;
        for (auto& m : *cl) id2cls[m->Id] = IdInfo{i, m->MatchStrand};
        i++;
    }
    return id2cls;
}

void write_cluster_cons(const string& outdir, const Batch& b)
{
    std::ofstream cons;
    create_file(outdir + "/cluster_cons.fq", cons);
    for (size_t i = 0; i < b.Cls.size(); ++i) {
        auto& rep = b.Cls[i]->at(0);
        if (!rep->RawSeq) die("Null pointer instead of cluster rep sequence at index: " + std::to_string(i));
        if (rep->RawSeq->score < 0) continue;
        string seq = rep->RawSeq->seq.str();
        if (rep->MatchStrand == -1) seq = revcomp(seq);
        cons << "@cluster_" << i << " origin=" << rep->RawSeq->name << ":" << rep->MatchStrand << " length=" << seq.size()
             << " size=" << b.Cls[i]->size() - 1 << "\n" << seq << "\n+\n" << rep->RawSeq->qual << "\n";
    }
}

struct Piece {  // a read's four lines in the mapping
    const char *hb, *sb, *pb, *qb, *qe;  // header, sequence, separator, qualities; he = sb - 1, se = pb - 1, pe = qb - 1
    bool flip;      // MatchStrand -1: sequence reverse-complemented, qualities reversed
    bool whole;     // the record ends with its newline: it can go out as it lies
};
typedef std::unordered_map<unsigned, std::vector<Piece>> PieceMap;

// clusters.tsv; every clustered read's piece of the mapping by cluster, and (for the read reports) the rows of clusters.tsv
void walk_sorted_fastq(const string& outdir, const MappedFile& fqmap, const IdMap& id2cls, PieceMap& per_cluster, std::vector<ReadStatRow>* stat_rows)
{
    std::ofstream tsv;
    create_file(outdir + "/clusters.tsv", tsv);
    tsv << "ClusterId\tStrand\tRead" << endl;
    LineCursor in{fqmap.data, fqmap.data + fqmap.size};
    const char *hb, *he, *sb, *se, *pb, *pe, *qb, *qe;
    while (in.line(hb, he) && in.line(sb, se) && in.line(pb, pe) && in.line(qb, qe)) {
        if (he == hb) continue;  // (std::string::substr(1) of an empty header throws in the reference's reader; nothing to keep here)
        const string id(hb + 1, size_t(he - hb - 1));
        auto it = id2cls.find(id);
        if (it == id2cls.end()) continue;
        const IdInfo& at = it->second;
        tsv << at.cls << "\t" << at.strand << "\t" << id << "\n";
        per_cluster[at.cls].push_back(Piece{hb, sb, pb, qb, qe, at.strand == -1, in.p == qe + 1});
        if (stat_rows) stat_rows->push_back(ReadStatRow{at.cls, at.strand, hb + 1, size_t(he - hb - 1), sb, size_t(se - sb), qb, size_t(qe - qb)});
    }
}

// cluster_fastq/<id>.fq: a read that keeps its strand goes into its cluster's file as the four lines it is in the mapping (one
// piece of a gather), a read of the other strand as a reverse-complemented copy.  False when the file could not be written.
bool write_cluster_fastq(const string& path, const std::vector<Piece>& pieces, string& stage)
{
    GatherFile f;
    if (!f.open(path)) return false;
    size_t need = 0;
    for (auto& pc : pieces)
        if (pc.flip || !pc.whole) need += size_t(pc.qe - pc.hb) + 2;
    stage.clear();
    stage.reserve(need);  // (the gather points into it: it must not move before close())
    for (auto& pc : pieces) {
        if (!pc.flip && pc.whole) {
            f.put(pc.hb, size_t(pc.qe + 1 - pc.hb));
            continue;
        }
        const size_t at = stage.size();
        stage.append(pc.hb, size_t(pc.sb - pc.hb));            // header line with its newline
        const char* se = pc.pb - 1;
        if (pc.flip) {
            for (const char* c = se; c != pc.sb;) stage += complement(*--c);
            stage += '\n';
            stage.append(pc.pb, size_t(pc.qb - pc.pb));        // separator line with its newline
            stage.append(std::reverse_iterator<const char*>(pc.qe), std::reverse_iterator<const char*>(pc.qb));
        } else {
            stage.append(pc.sb, size_t(pc.qe - pc.sb));
        }
        stage += '\n';
        f.put(stage.data() + at, stage.size() - at);
    }
    return f.close();
}

// the cluster files are written side by side by a few threads
void write_cluster_fastqs(const string& outdir, const PieceMap& per_cluster)
{
    std::vector<const PieceMap::value_type*> jobs;
    for (auto& kv : per_cluster) jobs.push_back(&kv);
    std::atomic<size_t> next{0};
    std::atomic<int> failed{0};
    run_threads(host_threads(8), [&](unsigned) {
        string stage;  // the flipped records of ONE cluster (and a last record without its newline), built by this thread
        for (size_t x = next.fetch_add(1); x < jobs.size(); x = next.fetch_add(1))
            if (!write_cluster_fastq(outdir + "/cluster_fastq/" + std::to_string(jobs[x]->first) + ".fq", jobs[x]->second, stage)) failed = 1;
    });
    if (failed) die("Failed to write the cluster FASTQ files!");
}

}  // namespace

int main_dump(int argc, char** argv)
{
    const DumpOptions d = parse_dump_options(argc, argv);
    const ReportOpts& reports = d.reports;
    Batch b;
    string err, fastq;
    Lap lap("dump");
    if (!load_batch(b, d.batch, err)) die(err);
    lap("batch loaded");
    if (!load_sorted_idx(fastq, d.index)) die("Failed to load index " + d.index);
    create_outdir(d.outdir);
    b.Db.clear();
    // SortClustersBySize, cluster.cpp:570-580 (std::sort, same comparator)
    std::sort(b.Cls.begin(), b.Cls.end(), [](const std::shared_ptr<Cluster> x, const std::shared_ptr<Cluster> y) {
        if (x->size() == y->size()) return x->at(0)->RawSeq->score > y->at(0)->RawSeq->score;
        return x->size() > y->size();
    });
    write_batch_info(d.outdir, b);
    const IdMap id2cls = write_clusters_info(d.outdir, b);
    write_cluster_cons(d.outdir, b);
    // The sorted FASTQ is read out of a mapping (src/output.cpp:225-275 reads and writes record by record; per-cluster strings
    // once held the whole 8 GB of configs[4] in anonymous memory).
    lap("read ids, info files, consensus fastq");
    MappedFile fqmap;
    {
        string merr;
        if (!map_file(fastq, fqmap, merr)) die("Failed to open " + fastq + "!");
    }
    lap("sorted fastq mapped");
    PieceMap per_cluster;
    std::vector<ReadStatRow> stat_rows;
    walk_sorted_fastq(d.outdir, fqmap, id2cls, per_cluster, reports.any() ? &stat_rows : nullptr);
    lap("sorted fastq walked, clusters.tsv");
    write_cluster_fastqs(d.outdir, per_cluster);
    lap("cluster fastq files written");
    if (reports.any()) {
        write_read_reports(b, d.outdir, stat_rows, reports);
        const string names = string(reports.stats ? "read_stats.tsv, " : "") + (reports.pileup ? "cluster_pileup.tsv, " : "") +
                             (reports.polish() ? "cluster_polished.fq, " : "") + (reports.sites.on ? "cluster_sites.tsv, read_alleles.tsv, " : "") +
                             (reports.split.on ? "cluster_split.tsv, read_split.tsv, " : "") + (reports.group_polish() ? "cluster_split_polished.fq, " : "") +
                             (reports.correct.on ? "corrected_reads.fq, " : "") +
                             (reports.isoforms.on ? "cluster_blocks.tsv, cluster_isoforms.tsv, read_isoforms.tsv, " : "") + (reports.iso_polish() ? "cluster_isoforms.fq, " : "") +
                             (reports.isoforms.on && reports.isoforms.inserts ? "cluster_inserts.tsv, read_inserts.tsv, " : "") +
                             (reports.isoforms.on && reports.isoforms.inserts && reports.isoforms.inserts_seq ? "cluster_inserts.fq, " : "") +
                             (reports.isoforms.on && reports.isoforms.inserts_seq && reports.isoforms.full ? "cluster_isoforms_full.fq, " : "") +
                             (reports.isoforms.on && reports.isoforms.inserts_seq && reports.isoforms.variants ? "cluster_insert_variants.fq, read_insert_variants.tsv, " : "") +
                             (reports.isoforms.on && reports.isoforms.inserts_seq && reports.isoforms.variants && reports.isoforms.full_variants ? "cluster_isoforms_full_variants.fq, " : "") +
                             (reports.isoforms.on && reports.isoforms.ends ? "cluster_ends.tsv, cluster_end_variants.tsv, read_ends.tsv, " : "") +
                             (reports.isoforms.on && reports.isoforms.correct ? "corrected_reads_isoforms.fq, " : "");
        lap((names.substr(0, names.size() - 2) + " (GPU alignments)").c_str());
    }
    if (VERBOSE) cerr << "Dump complete." << endl;
    return 0;
}
