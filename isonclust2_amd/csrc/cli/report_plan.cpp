// The host-only half of the read reports: which rows count, how the clusters are cut into groups, what a group holds, how much
// room the calls need, and the record formats.  Nothing here touches the library (tools/cli_reports_check.cpp links it alone).
#include <algorithm>

#include "common.hpp"
#include "reports.hpp"

using namespace cer;
using std::string;

ReportRows keep_report_rows(const Batch& b, const std::vector<ReadStatRow>& rows)
{
    ReportRows out{rows, {}, std::vector<std::vector<size_t>>(b.Cls.size())};
    for (size_t x = 0; x < rows.size(); ++x) {
        const ReadStatRow& r = rows[x];
        if (r.cls >= b.Cls.size() || b.Cls[r.cls]->at(0)->RawSeq->score < 0) continue;
        out.rows_of[r.cls].push_back(out.kept.size());
        out.kept.push_back(x);
    }
    return out;
}

void ReportGroup::add_rowless_cluster(size_t ci)
{
    group_cls.emplace_back(ci, int64_t(-1));
    group_seg.push_back(-1);
}

void ReportGroup::add_cluster(const Batch& b, size_t ci, const ReportRows& rows, const ReportOpts& opts)
{
    const auto& rep = b.Cls[ci]->at(0);
    const std::vector<size_t>& ys = rows.rows_of[ci];
    const int32_t rc = rep->MatchStrand == -1 ? 1 : 0;
    if (offs.empty()) offs.push_back(0), qoffs.push_back(0);
    // the representative: its stored sequence (the pair asks for the reverse complement when its strand is -1), its quality
    // line as cluster_cons.fq has it
    const int32_t rep_seq = int32_t(offs.size() - 1), rep_q = int32_t(qoffs.size() - 1);
    pool.append(rep->RawSeq->seq.data(), rep->RawSeq->seq.size());
    offs.push_back(int64_t(pool.size()));
    quals.append(rep->RawSeq->qual.data(), rep->RawSeq->qual.size());
    qoffs.push_back(int64_t(quals.size()));
    if (opts.groups()) {
        group_cls.emplace_back(ci, group_rows);
        group_seg.push_back(int32_t(segs.size()));
        row_base.insert(row_base.end(), ys.size(), group_rows);
        group_rows += int64_t(rep->RawSeq->seq.size()) + 1;
    }
    if (opts.segs()) {
        seg_of_pair.insert(seg_of_pair.end(), ys.size(), int32_t(segs.size()));
        seg_reads.push_back(int32_t(ys.size()));
        segs.push_back(ioc_polish_seg{rep_seq, rc});
    }
    for (size_t y : ys) {
        const ReadStatRow& r = rows.row(y);
        const int32_t q_seq = int32_t(offs.size() - 1), q_q = int32_t(qoffs.size() - 1);
        if (r.strand == -1) {  // as cluster_fastq/<id>.fq has the read: reverse-complemented, its qualities reversed
            for (size_t t = r.seq_len; t > 0; --t) pool += complement(r.seq[t - 1]);
            for (size_t t = r.qual_len; t > 0; --t) quals += r.qual[t - 1];
        } else {
            pool.append(r.seq, r.seq_len);
            quals.append(r.qual, r.qual_len);
        }
        offs.push_back(int64_t(pool.size()));
        qoffs.push_back(int64_t(quals.size()));
        pairs.push_back(ioc_aln_pair{q_seq, rep_seq, rc, 0 /* no hint */, 0.0 /* set when the group is aligned */});
        pair_row.push_back(y);
        pair_q.push_back(q_q);
        pair_rep_q.push_back(rep_q);
    }
}

void ReportGroup::clear()
{
    pool.clear(), quals.clear(), offs.clear(), qoffs.clear(), pairs.clear(), pair_row.clear(), pair_q.clear(), pair_rep_q.clear();
    group_cls.clear(), group_seg.clear(), row_base.clear(), group_rows = 0;
    segs.clear(), seg_of_pair.clear(), seg_reads.clear();
}

void plan_report_groups(const Batch& b, const ReportRows& rows, const ReportOpts& opts, const std::function<void(ReportGroup&)>& emit, size_t pool_max)
{
    ReportGroup g;
    for (size_t ci = 0; ci < b.Cls.size(); ++ci) {
        const auto& rep = b.Cls[ci]->at(0);
        if (rows.rows_of[ci].empty()) {
            if (opts.groups() && rep->RawSeq->score >= 0) g.add_rowless_cluster(ci);
            continue;
        }
        size_t need = rep->RawSeq->seq.size();
        for (size_t y : rows.rows_of[ci]) need += rows.row(y).seq_len;
        if (g.would_overflow(need, pool_max)) {
            emit(g);
            g.clear();
        }
        g.add_cluster(b, ci, rows, opts);
    }
    emit(g);
}

static int64_t ref_len(const ReportGroup& g, const ioc_polish_seg& sg) { return g.offs[size_t(sg.ref) + 1] - g.offs[size_t(sg.ref)]; }

int64_t polish_capacity(const ReportGroup& g, int groups)
{
    int64_t cap = 0;
    for (const ioc_polish_seg& sg : g.segs) {
        const int64_t m = ref_len(g, sg);
        cap += groups * (m + IOC_PILE_INS_SLOTS * (m + 1));
    }
    return cap;
}

int64_t correct_capacity(const ReportGroup& g)
{
    int64_t cap = 0;
    for (size_t x = 0; x < g.pairs.size(); ++x) {
        const int64_t m = ref_len(g, g.segs[size_t(g.seg_of_pair[x])]);
        cap += m + IOC_PILE_INS_SLOTS * (m + 1);
    }
    return cap;
}

int64_t iso_correct_capacity(const ReportGroup& g)
{
    int64_t cap = correct_capacity(g);
    for (const ioc_aln_pair& p : g.pairs) cap += g.offs[size_t(p.query) + 1] - g.offs[size_t(p.query)];
    return cap;
}

int64_t blocks_capacity(const ReportGroup& g, int max_blocks)
{
    int64_t cap = 0;
    for (const ioc_polish_seg& sg : g.segs) cap += std::min<int64_t>(max_blocks, ref_len(g, sg));
    return cap;
}

int64_t inserts_capacity(const ReportGroup& g, int max_sites)
{
    int64_t cap = 0;
    for (const ioc_polish_seg& sg : g.segs) cap += std::min<int64_t>(max_sites, std::max<int64_t>(ref_len(g, sg) - 1, 0));
    return cap;
}

IsoCapacity iso_polish_capacity(const ReportGroup& g, int max_iso)
{
    IsoCapacity cap;
    for (size_t s = 0; s < g.segs.size(); ++s) {
        const int64_t m = ref_len(g, g.segs[s]), most = std::min<int64_t>(max_iso, g.seg_reads[s]);
        cap.isoforms += most;
        cap.bytes += most * (m + IOC_PILE_INS_SLOTS * (m + 1));
    }
    return cap;
}

IsoCapacity iso_full_capacity(const ReportGroup& g, int max_iso, int max_sites, int max_win)
{
    IsoCapacity cap;
    for (size_t s = 0; s < g.segs.size(); ++s) {
        const int64_t m = ref_len(g, g.segs[s]), most = std::min<int64_t>(max_iso, g.seg_reads[s]), sites = std::min<int64_t>(max_sites, std::max<int64_t>(m - 1, 0));
        cap.isoforms += most;
        cap.bytes += most * (m + IOC_PILE_INS_SLOTS * (m + 1) + sites * (7 * int64_t(max_win) + 6));
    }
    return cap;
}

SiteCapacity site_capacity(const ReportGroup& g, int max_sites)
{
    SiteCapacity cap;
    std::vector<int64_t> seg_cap(g.segs.size());
    for (size_t s = 0; s < g.segs.size(); ++s) {
        seg_cap[s] = std::min<int64_t>(max_sites, 2 * ref_len(g, g.segs[s]) + 1);
        cap.sites += seg_cap[s];
    }
    for (size_t x = 0; x < g.pairs.size(); ++x) cap.alleles += seg_cap[size_t(g.seg_of_pair[x])];
    return cap;
}

char allele_char(int32_t kind, int32_t a)
{
    return kind == IOC_SITE_INS ? (a == 0 ? '.' : a == 1 ? '+' : '?') : (a >= 0 && a <= IOC_ALLELE_DEL ? "ACGTN-"[a] : '?');
}

string polish_record(const string& name, int32_t reads, const ioc_polish_stats& z, const char* tail, const char* seq, const char* qual, size_t len)
{
    string text = "@" + name + " reads=" + std::to_string(reads) + " subs=" + std::to_string(z.n_sub) + " dels=" + std::to_string(z.n_del) +
                  " ins=" + std::to_string(z.n_ins) + " low=" + std::to_string(z.n_low) + tail + "\n";
    text.append(seq, len).append("\n+\n").append(qual, len).append("\n");
    return text;
}

string corrected_record(const char* id, size_t id_len, unsigned cls, const char* read, size_t read_len, const char* qual, size_t qual_len,
                        const ioc_aln_stats& a, const ioc_correct_stats& z, const char* cseq, const char* cqual, size_t clen)
{
    string own_qual(qual, std::min(qual_len, read_len));
    own_qual.resize(read_len, '!');
    const bool as_it_is = a.longest_ins > IOC_PILE_INS_SLOTS;
    const ioc_correct_stats k = as_it_is ? ioc_correct_stats{} : z;
    string text = "@" + string(id, id_len) + " cluster=" + std::to_string(cls) + " subs=" + std::to_string(k.n_sub) + " fills=" + std::to_string(k.n_fill) +
                  " removes=" + std::to_string(k.n_remove) + " ins_add=" + std::to_string(k.n_ins_add) + " ins_drop=" + std::to_string(k.n_ins_drop) +
                  " low=" + std::to_string(k.n_low) + " guarded=" + std::to_string(k.n_guarded) + (as_it_is ? " uncorrected=long_insertion" : "") + "\n";
    if (as_it_is) return text.append(read, read_len).append("\n+\n").append(own_qual).append("\n");
    const size_t lead = std::min(size_t(std::max(a.lead_i, 0)), read_len), trail = std::min(size_t(std::max(a.trail_i, 0)), read_len - lead);
    text.append(read, lead).append(cseq, clen).append(read + read_len - trail, trail).append("\n+\n");
    text.append(own_qual, 0, lead).append(cqual, clen).append(own_qual, read_len - trail, trail).append("\n");
    return text;
}

string iso_corrected_record(const char* id, size_t id_len, unsigned cls, const char* read, size_t read_len, const char* qual, size_t qual_len,
                            const ioc_aln_stats& a, const ioc_iso_correct_stats& z, int32_t isoform, const char* cseq, const char* cqual, size_t clen)
{
    string own_qual(qual, std::min(qual_len, read_len));
    own_qual.resize(read_len, '!');
    const bool as_it_is = (z.flags & IOC_ISOC_UNRESOLVED) != 0;
    string text = "@" + string(id, id_len) + " cluster=" + std::to_string(cls) + " subs=" + std::to_string(z.n_sub) + " fills=" + std::to_string(z.n_fill) +
                  " removes=" + std::to_string(z.n_remove) + " ins_add=" + std::to_string(z.n_ins_add) + " ins_drop=" + std::to_string(z.n_ins_drop) +
                  " low=" + std::to_string(z.n_low) + " guarded=" + std::to_string(z.n_guarded) + " isoform=" + (isoform >= 0 ? std::to_string(isoform) : string("-")) +
                  " table=" + (z.table >= 0 ? "isoform" : "cluster") + " long_runs=" + std::to_string(z.n_long_runs) + " long_bases=" + std::to_string(z.n_long_bases) +
                  (as_it_is ? " uncorrected=unresolved_insertion" : "") + "\n";
    if (as_it_is) return text.append(read, read_len).append("\n+\n").append(own_qual).append("\n");
    const size_t lead = std::min(size_t(std::max(a.lead_i, 0)), read_len), trail = std::min(size_t(std::max(a.trail_i, 0)), read_len - lead);
    text.append(read, lead).append(cseq, clen).append(read + read_len - trail, trail).append("\n+\n");
    text.append(own_qual, 0, lead).append(cqual, clen).append(own_qual, read_len - trail, trail).append("\n");
    return text;
}

string blocks_signature(uint64_t key, int32_t n_blocks)
{
    string text;
    for (int32_t b = 0; b < n_blocks && b < IOC_BLOCKS_MAX; ++b) text += "=-~."[(key >> (2 * b)) & 3u];
    return text.empty() ? "*" : text;
}

string cluster_blocks_rows(size_t cluster, const ioc_blocks_seg& z, const ioc_pile_block* blocks)
{
    const string id = std::to_string(cluster);
    string text;
    if (z.n_found > z.n_blocks) text += "# cluster " + id + ": kept " + std::to_string(z.n_blocks) + " of " + std::to_string(z.n_found) + " blocks\n";
    for (int32_t b = 0; b < z.n_blocks; ++b) {
        const ioc_pile_block& k = blocks[b];
        text += id + '\t' + std::to_string(b) + '\t' + std::to_string(k.first) + '\t' + std::to_string(k.end) + '\t' + std::to_string(k.n_keep) + '\t' +
                std::to_string(k.n_skip) + '\t' + std::to_string(k.n_part) + '\t' + std::to_string(k.n_none) + '\n';
    }
    return text;
}

string cluster_isoforms_rows(size_t cluster, const ioc_blocks_seg& z, const std::vector<ioc_read_blocks>& reads)
{
    const size_t n = size_t(std::max(z.n_groups, 0));
    std::vector<uint64_t> key(n, 0);
    std::vector<int64_t> direct(n, 0), assigned(n, 0);
    for (const ioc_read_blocks& r : reads) {
        if (r.group < 0 || size_t(r.group) >= n) continue;
        if (r.how == IOC_ISO_DIRECT) key[size_t(r.group)] = r.key, ++direct[size_t(r.group)];
        if (r.how == IOC_ISO_ASSIGNED) ++assigned[size_t(r.group)];
    }
    string text;
    for (size_t x = 0; x < n; ++x)
        text += std::to_string(cluster) + '\t' + std::to_string(x) + '\t' + blocks_signature(key[x], z.n_blocks) + '\t' + std::to_string(direct[x]) + '\t' +
                std::to_string(assigned[x]) + '\n';
    return text;
}

string cluster_isoform_records(size_t cluster, const ioc_blocks_seg& z, const std::vector<ioc_read_blocks>& reads, int64_t n_called, const int64_t* off,
                               const ioc_polish_stats* stats, const char* seq, const char* qual)
{
    if (z.n_blocks < 1) return "";
    const size_t n = size_t(std::max<int64_t>(std::min<int64_t>(n_called, z.n_groups), 0));
    std::vector<uint64_t> key(n, 0);
    std::vector<int32_t> mine(n, 0);
    for (const ioc_read_blocks& r : reads) {
        if (r.group < 0 || size_t(r.group) >= n) continue;
        if (r.how == IOC_ISO_DIRECT) key[size_t(r.group)] = r.key;
        if (r.how == IOC_ISO_DIRECT || r.how == IOC_ISO_ASSIGNED) ++mine[size_t(r.group)];
    }
    string text;
    for (size_t h = 0; h < n; ++h)
        text += polish_record("cluster_" + std::to_string(cluster) + "/iso" + std::to_string(h) + " key=" + blocks_signature(key[h], z.n_blocks), mine[h], stats[h], "",
                              seq + off[h], qual + off[h], size_t(off[h + 1] - off[h]));
    return text;
}

string inserts_signature(uint64_t key, int32_t n_sites)
{
    string text;
    for (int32_t b = 0; b < n_sites && b < IOC_INSERTS_MAX; ++b) text += "=+?."[(key >> (2 * b)) & 3u];
    return text.empty() ? "*" : text;
}

string cluster_inserts_rows(size_t cluster, const ioc_inserts_seg& z, const ioc_pile_insert* sites)
{
    const string id = std::to_string(cluster);
    string text;
    if (z.n_found > z.n_sites) text += "# cluster " + id + ": kept " + std::to_string(z.n_sites) + " of " + std::to_string(z.n_found) + " sites\n";
    for (int32_t b = 0; b < z.n_sites; ++b) {
        const ioc_pile_insert& k = sites[b];
        text += id + '\t' + std::to_string(k.first) + '\t' + std::to_string(k.end) + '\t' + std::to_string(k.n_carry) + '\t' + std::to_string(k.n_lack) + '\t' +
                std::to_string(k.n_none) + '\t' + std::to_string(k.len_min) + '\t' + std::to_string(k.len_max) + '\n';
    }
    return text;
}

string read_insert_columns(const ioc_read_inserts& r, int32_t n_sites)
{
    const char* const how = r.how == IOC_ISO_DIRECT ? "direct" : r.how == IOC_ISO_ASSIGNED ? "assigned" : r.how == IOC_ISO_RARE ? "rare" : "ambiguous";
    return inserts_signature(r.key, n_sites) + '\t' + (r.group < 0 ? string(".") : std::to_string(r.group)) + '\t' + how;
}

string variants_signature(uint64_t key2, int32_t n_sites)
{
    string text;
    for (int32_t b = 0; b < n_sites && b < IOC_INSERTS_MAX; ++b) text += "=AB."[(key2 >> (2 * b)) & 3u];
    return text.empty() ? "*" : text;
}

string read_variant_columns(const ioc_read_variants& r, int32_t n_sites)
{
    const char* const how = r.how == IOC_ISO_DIRECT ? "direct" : r.how == IOC_ISO_ASSIGNED ? "assigned" : r.how == IOC_ISO_RARE ? "rare" : "ambiguous";
    return variants_signature(r.key2, n_sites) + '\t' + (r.group < 0 ? string(".") : std::to_string(r.group)) + '\t' + how;
}

string full_variants_tail(uint64_t key2, const ioc_splice_site* sites, int64_t n_sites)
{
    string text;
    for (int64_t b = 0; b < n_sites && b < IOC_INSERTS_MAX; ++b)
        if (sites[b].state == IOC_SPLICE_DONE)
            text += " ins" + std::to_string(b) + '/' + (((key2 >> (2 * b)) & 3u) == IOC_INS_CARRY_B ? 'B' : 'A') + '@' + std::to_string(sites[b].at) + '+' + std::to_string(sites[b].len);
    return text;
}

EndsCapacity ends_capacity(const ReportGroup& g, int max_sites, int max_variants)
{
    EndsCapacity cap;
    for (size_t s = 0; s < g.segs.size(); ++s) {
        cap.sites += 2 * std::min<int64_t>(max_sites, ref_len(g, g.segs[s]) + 1);
        cap.variants += std::min<int64_t>(max_variants, g.seg_reads[s]);
    }
    return cap;
}

string cluster_ends_rows(size_t cluster, const ioc_ends_seg& z, const ioc_end_site* starts, const ioc_end_site* stops)
{
    const string id = std::to_string(cluster);
    string text;
    if (z.n_starts_found > z.n_starts) text += "# cluster " + id + ": kept " + std::to_string(z.n_starts) + " of " + std::to_string(z.n_starts_found) + " start sites\n";
    if (z.n_stops_found > z.n_stops) text += "# cluster " + id + ": kept " + std::to_string(z.n_stops) + " of " + std::to_string(z.n_stops_found) + " stop sites\n";
    for (int kind = 0; kind < 2; ++kind)
        for (int32_t b = 0; b < (kind ? z.n_stops : z.n_starts); ++b) {
            const ioc_end_site& k = (kind ? stops : starts)[b];
            text += id + '\t' + (kind ? "stop" : "start") + '\t' + std::to_string(b) + '\t' + std::to_string(k.first) + '\t' + std::to_string(k.end) + '\t' +
                    std::to_string(k.peak_row) + '\t' + std::to_string(k.peak_reads) + '\t' + std::to_string(k.n_reads) + '\t' + std::to_string(k.n_over) + '\n';
        }
    return text;
}

string cluster_end_variants_rows(size_t cluster, const ioc_ends_seg& z, const ioc_end_variant* variants)
{
    const string id = std::to_string(cluster);
    string text;
    if (z.n_variants_found > z.n_variants) text += "# cluster " + id + ": kept " + std::to_string(z.n_variants) + " of " + std::to_string(z.n_variants_found) + " variants\n";
    for (int32_t v = 0; v < z.n_variants; ++v) {
        const ioc_end_variant& k = variants[v];
        text += id + '\t' + std::to_string(v) + '\t' + std::to_string(k.pre_group) + '\t' + std::to_string(k.start_site) + '\t' + std::to_string(k.stop_site) + '\t' +
                std::to_string(k.n_reads) + '\n';
    }
    return text;
}

string read_end_columns(const ioc_read_extent& e, const ioc_read_ends& r)
{
    auto or_dot = [](int32_t v) { return v < 0 ? string(".") : std::to_string(v); };
    return std::to_string(e.first_row) + '\t' + std::to_string(e.end_row) + '\t' + std::to_string(e.head) + '\t' + std::to_string(e.tail) + '\t' + or_dot(r.start_site) +
           '\t' + or_dot(r.stop_site) + '\t' + or_dot(r.variant);
}

string read_isoform_columns(const ioc_read_blocks& r, int32_t n_blocks)
{
    const char* const how = r.how == IOC_ISO_DIRECT ? "direct" : r.how == IOC_ISO_ASSIGNED ? "assigned" : r.how == IOC_ISO_RARE ? "rare" : "ambiguous";
    return (r.group < 0 ? string(".") : std::to_string(r.group)) + '\t' + how + '\t' + blocks_signature(r.key, n_blocks) + '\t' + std::to_string(r.first_row) + '\t' +
           std::to_string(r.end_row) + '\t' + std::to_string(r.n_gaps) + '\t' + std::to_string(r.gap_rows);
}
