// ioc_align_sinks.cpp — the entry points of the batched GPU aligner that ask for the alignment itself, and the consensus call on
// top of them: each describes where the walks' operation bytes go (AlnSink, ioc_align_sink.h) and runs ioc_align_pairs_sink
// (ioc_align_gpu.hip).  Host code only: the kernels are behind the iock_* launchers.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ioc_align_sink.h"
#include "ioc_internal.h"
#include "ioc_plane_pile.h"

namespace {

struct AlnCall {  // what every aligning entry point passes on
    int32_t n_pairs;
    const ioc_aln_pair* pairs;
    int32_t k, match, mismatch, gap_extend;
    int32_t* score;
    int64_t* windows;
    double* ratio;
    int run(ioc_ctx* c, const AlnSink* sink) const { return ioc_align_pairs_sink(c, n_pairs, pairs, k, match, mismatch, gap_extend, score, windows, ratio, sink); }
};

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }


// the segments' bound on kept sites: a row yields at most two, its insertion site and its base site, and row rlen one
int64_t pile_sites_bound(const std::vector<IocPileSeg>& segs, int32_t max_sites)
{
    int64_t b = 0;
    for (const IocPileSeg& s : segs) b += std::min<int64_t>(max_sites, 2 * int64_t(s.rlen) + 1);
    return b;
}

// what a split is run with and where it leaves what it made (ioc_host_alleles_split's parameters and outputs, per call)
struct SplitCall {
    int32_t min_link, min_margin, rounds;
    int64_t* out_link;
    int8_t* out_phase;
    uint8_t* out_group;
    int32_t* out_vote;
    ioc_split_seg* out_seg;
    // (ioc_align_pairs_split_polish) where the split left the member lists and the group bytes on the device (a_split), for the
    // stage behind it; NULL: nobody asks
    struct Laid {
        const uint32_t *mem_off = nullptr, *members = nullptr;
        const uint8_t* group = nullptr;
    }* laid = nullptr;
};

// the parameters ioc_host_alleles_split refuses
bool split_rule_ok(int32_t min_link, int32_t min_margin, int32_t rounds) { return min_link >= 1 && min_margin >= 1 && rounds >= 0 && rounds <= 64; }

// The split kernels (ioc_site_split.hip) over sites and alleles that lie on the device — or on the host (on_device false), and are
// uploaded then — and what they made copied back.  site_off / allele_off / seg_of_pair are the host's; the member lists come from
// a counting sort of seg_of_pair (a segment's reads are its pairs in ascending order).  a_split holds, in this order, the host's
// tables [site_off][allele_off][seg_of_pair][mem_off][members][word_off][bit_off][tile_seg][seg_of_site], the kernels' own
// [marks][bits minor][bits major][g1][g0][link][phase][seed][group][vote][records] and, uploaded, [sites][alleles].  Under
// IOC_TRACE the steps are timed one by one (t.ms_split, in the order of IocSplitStep).
int split_device(ioc_ctx* c, const SplitCall& sp, size_t n, size_t np, const int32_t* seg_of_pair, const int64_t* site_off, const int64_t* allele_off,
                 const ioc_pile_site* sites, const uint8_t* alleles, bool on_device, AlnTally& t)
{
    const size_t S = n ? size_t(site_off[n]) : 0, bytes = np ? size_t(allele_off[np]) : 0;
    std::vector<uint32_t> mem_off(n + 1, 0), members(np), word_off(n + 1, 0);
    std::vector<int64_t> bit_off(n + 1, 0);
    for (size_t i = 0; i < np; ++i) ++mem_off[size_t(seg_of_pair[i]) + 1];
    for (size_t g = 0; g < n; ++g) mem_off[g + 1] += mem_off[g];
    {
        std::vector<uint32_t> next(mem_off.begin(), mem_off.end() - 1);
        for (size_t i = 0; i < np; ++i) members[next[size_t(seg_of_pair[i])]++] = uint32_t(i);
    }
    for (size_t g = 0; g < n; ++g) {
        const uint32_t words = (mem_off[g + 1] - mem_off[g] + 63u) / 64u;
        word_off[g + 1] = word_off[g] + words;
        bit_off[g + 1] = bit_off[g] + int64_t(words) * (site_off[g + 1] - site_off[g]);
    }
    const size_t T = word_off[n], P = size_t(bit_off[n]);
    std::vector<int32_t> tile_seg(T), seg_of_site(S);
    for (size_t g = 0; g < n; ++g) {
        std::fill(tile_seg.begin() + word_off[g], tile_seg.begin() + word_off[g + 1], int32_t(g));
        std::fill(seg_of_site.begin() + site_off[g], seg_of_site.begin() + site_off[g + 1], int32_t(g));
    }
    auto up16 = [](size_t v) { return (v + 15) & ~size_t(15); };
    size_t at = 0;
    auto take = [&](size_t b) { const size_t o = at; at += up16(b); return o; };
    const size_t o_soff = take((n + 1) * 8), o_aoff = take((np + 1) * 8), o_sop = take(np * 4), o_moff = take((n + 1) * 4), o_mem = take(np * 4),
                 o_woff = take((n + 1) * 4), o_boff = take((n + 1) * 8), o_tseg = take(T * 4), o_sos = take(S * 4), tables = at;
    const size_t o_marks = take(S * 8), o_bm = take(P * 8), o_bM = take(P * 8), o_g1 = take(T * 8), o_g0 = take(T * 8), o_link = take(S * 8),
                 o_phase = take(S), o_seed = take(n * 4), o_group = take(np), o_vote = take(np * 4), o_rec = take(n * sizeof(ioc_split_seg));
    const size_t o_sites = take(on_device ? 0 : S * sizeof(ioc_pile_site)), o_all = take(on_device ? 0 : bytes);
    std::vector<uint8_t> stage(tables, 0);
    const int64_t zero = 0;
    auto put = [&](size_t o, const void* src, size_t b) { if (b) memcpy(stage.data() + o, src, b); };
    put(o_soff, n ? site_off : &zero, (n + 1) * 8), put(o_aoff, np ? allele_off : &zero, (np + 1) * 8), put(o_sop, seg_of_pair, np * 4);
    put(o_moff, mem_off.data(), (n + 1) * 4), put(o_mem, members.data(), np * 4), put(o_woff, word_off.data(), (n + 1) * 4);
    put(o_boff, bit_off.data(), (n + 1) * 8), put(o_tseg, tile_seg.data(), T * 4), put(o_sos, seg_of_site.data(), S * 4);
    IOC_CHK(c, hipSetDevice(c->device));
    IOC_TRY(ioc_reserve(c, c->a_split, at));
    uint8_t* p = static_cast<uint8_t*>(c->a_split.p);
    IOC_CHK(c, hipMemcpyAsync(p, stage.data(), tables, hipMemcpyHostToDevice, c->stream));
    t.split_uploaded += int64_t(tables);
    if (!on_device) {
        if (S) IOC_CHK(c, hipMemcpyAsync(p + o_sites, sites, S * sizeof(ioc_pile_site), hipMemcpyHostToDevice, c->stream));
        if (bytes) IOC_CHK(c, hipMemcpyAsync(p + o_all, alleles, bytes, hipMemcpyHostToDevice, c->stream));
        t.split_uploaded += int64_t(S * sizeof(ioc_pile_site) + bytes);
    }
    auto u64p = [&](size_t o) { return reinterpret_cast<unsigned long long*>(p + o); };
    uint64_t most = 0;
    for (size_t g = 0; g < n; ++g) most = std::max<uint64_t>(most, uint64_t(site_off[g + 1] - site_off[g]));
    const IocSplitDev v{uint32_t(n), uint32_t(np), uint32_t(T), uint64_t(S), uint64_t(bytes), uint64_t(P), most,
                        on_device ? sites : reinterpret_cast<const ioc_pile_site*>(p + o_sites), reinterpret_cast<const long long*>(p + o_soff),
                        on_device ? alleles : p + o_all, reinterpret_cast<const long long*>(p + o_aoff), reinterpret_cast<const int32_t*>(p + o_sop),
                        reinterpret_cast<const uint32_t*>(p + o_moff), reinterpret_cast<const uint32_t*>(p + o_mem),
                        reinterpret_cast<const uint32_t*>(p + o_woff), reinterpret_cast<const long long*>(p + o_boff),
                        reinterpret_cast<const int32_t*>(p + o_tseg), reinterpret_cast<const int32_t*>(p + o_sos), reinterpret_cast<int2*>(p + o_marks),
                        u64p(o_bm), u64p(o_bM), u64p(o_g1), u64p(o_g0), reinterpret_cast<long long*>(p + o_link), reinterpret_cast<int8_t*>(p + o_phase),
                        reinterpret_cast<int32_t*>(p + o_seed), p + o_group, reinterpret_cast<int32_t*>(p + o_vote),
                        reinterpret_cast<ioc_split_seg*>(p + o_rec)};
    if (sp.laid) *sp.laid = SplitCall::Laid{reinterpret_cast<const uint32_t*>(p + o_moff), reinterpret_cast<const uint32_t*>(p + o_mem), p + o_group};
    std::vector<IocSplitStep> steps{IocSplitStep::marks, IocSplitStep::bits, IocSplitStep::link, IocSplitStep::seed, IocSplitStep::phase0,
                                    IocSplitStep::vote};
    for (int32_t r = 0; r < sp.rounds; ++r) steps.insert(steps.end(), {IocSplitStep::group_bits, IocSplitStep::rephase, IocSplitStep::vote});
    steps.push_back(IocSplitStep::record);
    const bool timed = getenv("IOC_TRACE") != nullptr;
    EventSet ev;
    if (timed) {
        ev.v.assign(steps.size() + 1, nullptr);
        for (auto& e : ev.v) IOC_CHK(c, hipEventCreate(&e));
        IOC_CHK(c, hipEventRecord(ev.v[0], c->stream));
    }
    for (size_t x = 0; x < steps.size(); ++x) {
        IOC_CHK(c, iock_site_split(c->stream, v, steps[x], sp.min_link, sp.min_margin));
        if (timed) IOC_CHK(c, hipEventRecord(ev.v[x + 1], c->stream));
    }
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    for (size_t x = 0; timed && x < steps.size(); ++x) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.v[x], ev.v[x + 1]) == hipSuccess) t.ms_split[size_t(steps[x])] += double(ms);
    }
    const auto t0 = std::chrono::steady_clock::now();
    const struct { void* dst; size_t off, b; } outs[] = {{sp.out_link, o_link, S * 8}, {sp.out_phase, o_phase, S}, {sp.out_group, o_group, np},
                                                         {sp.out_vote, o_vote, np * 4}, {sp.out_seg, o_rec, n * sizeof(ioc_split_seg)}};
    for (const auto& o : outs)
        if (o.dst && o.b) {
            IOC_CHK(c, hipMemcpy(o.dst, p + o.off, o.b, hipMemcpyDeviceToHost));
            t.copied += int64_t(o.b);
        }
    t.ms_copy += ms_since(t0);
    return IOC_OK;
}

// the split's part of a trace line
std::string split_trace(const AlnTally& t)
{
    char buf[480];
    snprintf(buf, sizeof buf, "k_site_marks %.3f ms, k_allele_bits %.3f ms, k_site_link %.3f ms, k_split_seed %.3f ms, k_split_phase0 %.3f ms, k_split_vote %.3f ms, k_group_bits %.3f ms, k_split_rephase %.3f ms, k_split_record %.3f ms, %lld bytes uploaded",
             t.ms_split[0], t.ms_split[1], t.ms_split[2], t.ms_split[3], t.ms_split[4], t.ms_split[5], t.ms_split[6], t.ms_split[7], t.ms_split[8],
             (long long)t.split_uploaded);
    return buf;
}

// where a site search leaves what it found and, where there are pairs with planes, their alleles
struct SitesCall {
    const std::vector<IocPileSeg>& segs;
    int32_t min_depth, min_alt, min_pct, max_sites;
    ioc_pile_site* out_sites;
    int64_t *site_off, *n_found;
    // the pairs (ioc_align_pairs_alleles; n_pairs 0: none): pair i's planes start at byte plane[i] of each of the two planes
    int32_t n_pairs = 0;
    const int32_t* seg_of_pair = nullptr;
    const int64_t* plane = nullptr;
    int64_t plane_bytes = 0, alleles_bound = 0;
    uint8_t* out_alleles = nullptr;  // (NULL with a split: the alleles stay on the device)
    int64_t* allele_off = nullptr;
    const SplitCall* split = nullptr;  // (ioc_align_pairs_split) the split, run where the sites and the alleles lie
    bool project_ins = false;          // (ioc_align_pairs_split_polish) the six slot planes behind the two: what every pair inserts
};

// The site kernels over a table that lies on the device (n_rows records), then k_site_alleles over the planes d_base / d_ins where
// the call has pairs, and what they made copied back: a_call holds [segments][seg_len][site_off][n_found][sites] and behind them
// [seg_of_pair][plane][allele_off][alleles].  Device times go to t.ms_sites / t.ms_alleles, the copies to t.ms_copy / t.copied.
int pile_sites_device(ioc_ctx* c, const SitesCall& sc, const ioc_pileup_col* d_cols, int64_t n_rows, const uint8_t* d_base, const uint8_t* d_ins,
                      AlnTally& t)
{
    const size_t n = sc.segs.size(), np = size_t(sc.n_pairs);
    const size_t bound = size_t(pile_sites_bound(sc.segs, sc.max_sites)), a_bound = size_t(sc.alleles_bound);
    auto up16 = [](size_t v) { return (v + 15) & ~size_t(15); };
    const size_t o_seg = 0, o_len = up16(n * sizeof(IocPileSeg)), o_off = o_len + up16(n * 8), o_found = o_off + up16((n + 1) * 8),
                 o_sites = o_found + up16(n * 8), o_sop = o_sites + up16(bound * sizeof(ioc_pile_site)), o_plane = o_sop + up16(np * 4),
                 o_aoff = o_plane + up16(np * 8), o_all = o_aoff + up16((np + 1) * 8), total = o_all + up16(a_bound);
    IOC_TRY(ioc_reserve(c, c->a_call, total));
    uint8_t* p = static_cast<uint8_t*>(c->a_call.p);
    IOC_CHK(c, hipMemcpyAsync(p + o_seg, sc.segs.data(), n * sizeof(IocPileSeg), hipMemcpyHostToDevice, c->stream));
    EventSet ev;
    ev.v.assign(4, nullptr);
    for (auto& e : ev.v) IOC_CHK(c, hipEventCreate(&e));
    IOC_CHK(c, hipEventRecord(ev.v[0], c->stream));
    IOC_CHK(c, iock_pile_sites(c->stream, reinterpret_cast<const IocPileSeg*>(p + o_seg), uint32_t(n), d_cols, uint64_t(n_rows), sc.min_depth, sc.min_alt,
                               sc.min_pct, sc.max_sites, reinterpret_cast<int64_t*>(p + o_found), reinterpret_cast<int64_t*>(p + o_len),
                               reinterpret_cast<int64_t*>(p + o_off), reinterpret_cast<ioc_pile_site*>(p + o_sites), uint64_t(bound)));
    IOC_CHK(c, hipEventRecord(ev.v[1], c->stream));
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    auto t0 = std::chrono::steady_clock::now();
    IOC_CHK(c, hipMemcpy(sc.site_off, p + o_off, (n + 1) * 8, hipMemcpyDeviceToHost));
    IOC_CHK(c, hipMemcpy(sc.n_found, p + o_found, n * 8, hipMemcpyDeviceToHost));
    const int64_t kept = sc.site_off[n];
    if (kept < 0 || size_t(kept) > bound) return ioc_fail(c, IOC_ERR_HIP, "the site search returned a count outside its bound");
    if (kept > 0) IOC_CHK(c, hipMemcpy(sc.out_sites, p + o_sites, size_t(kept) * sizeof(ioc_pile_site), hipMemcpyDeviceToHost));
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev.v[0], ev.v[1]) == hipSuccess) t.ms_sites += double(ms);
    t.ms_copy += ms_since(t0);
    t.copied += int64_t((2 * n + 1) * 8 + size_t(kept) * sizeof(ioc_pile_site));
    if (!sc.allele_off) return IOC_OK;
    sc.allele_off[0] = 0;
    for (size_t i = 0; i < np; ++i) sc.allele_off[i + 1] = sc.allele_off[i] + (sc.site_off[sc.seg_of_pair[i] + 1] - sc.site_off[sc.seg_of_pair[i]]);
    const int64_t bytes = sc.allele_off[np];
    if (bytes > sc.alleles_bound) return ioc_fail(c, IOC_ERR_HIP, "the site search kept more sites than its bound");
    auto split = [&]() {
        return sc.split ? split_device(c, *sc.split, n, np, sc.seg_of_pair, sc.site_off, sc.allele_off, reinterpret_cast<const ioc_pile_site*>(p + o_sites),
                                       p + o_all, true, t)
                        : IOC_OK;
    };
    if (bytes == 0) return split();
    IOC_CHK(c, hipMemcpyAsync(p + o_sop, sc.seg_of_pair, np * 4, hipMemcpyHostToDevice, c->stream));
    IOC_CHK(c, hipMemcpyAsync(p + o_plane, sc.plane, np * 8, hipMemcpyHostToDevice, c->stream));
    IOC_CHK(c, hipMemcpyAsync(p + o_aoff, sc.allele_off, (np + 1) * 8, hipMemcpyHostToDevice, c->stream));
    IOC_CHK(c, hipEventRecord(ev.v[2], c->stream));
    IOC_CHK(c, iock_site_alleles(c->stream, uint32_t(np), reinterpret_cast<const int32_t*>(p + o_sop), reinterpret_cast<const IocPileSeg*>(p + o_seg),
                                 uint32_t(n), reinterpret_cast<const uint64_t*>(p + o_plane), d_base, d_ins, uint64_t(sc.plane_bytes),
                                 reinterpret_cast<const ioc_pile_site*>(p + o_sites), reinterpret_cast<const int64_t*>(p + o_off),
                                 reinterpret_cast<const int64_t*>(p + o_aoff), p + o_all, uint64_t(bytes)));
    IOC_CHK(c, hipEventRecord(ev.v[3], c->stream));
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    t0 = std::chrono::steady_clock::now();
    if (sc.out_alleles) IOC_CHK(c, hipMemcpy(sc.out_alleles, p + o_all, size_t(bytes), hipMemcpyDeviceToHost));
    if (hipEventElapsedTime(&ms, ev.v[2], ev.v[3]) == hipSuccess) t.ms_alleles += double(ms);
    t.ms_copy += ms_since(t0);
    t.copied += sc.out_alleles ? bytes : 0;
    return split();
}

// the thresholds ioc_host_pileup_sites refuses
bool sites_rule_ok(int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_sites)
{
    return min_depth >= 1 && min_alt >= 1 && min_pct >= 1 && min_pct <= 50 && max_sites >= 1;
}

}  // namespace

// (pile_call_bound, pile_call_device, pileup_call_tables and align_pairs_polish stand inside extern "C", where they have always
// stood: their plain names stay in the library's symbol list)
extern "C" {
namespace {

// the segments' bound: what ioc_host_pileup_call asks of cap, summed
int64_t pile_call_bound(const std::vector<IocPileSeg>& segs)
{
    int64_t b = 0;
    for (const IocPileSeg& s : segs) b += int64_t(s.rlen) + int64_t(IOC_PILE_INS_SLOTS) * (int64_t(s.rlen) + 1);
    return b;
}

// where a consensus call reads its frames and leaves what it called
struct PileCall {
    const std::vector<IocPileSeg>& segs;
    const uint8_t* d_frames;
    uint64_t frame_bytes;
    int32_t min_depth;
    char *out_seq, *out_qual;
    int64_t* out_off;
    ioc_polish_stats* out_stats;
};

// The call kernels over tables that lie on the device (n_rows records each), and what they made copied back: a_call holds
// [segments][seg_len][out_off][records][sequence][qualities].  The kernels' device time is added to t.ms_call, the host's time
// over the copies and their bytes to t.ms_copy / t.copied.
int pile_call_device(ioc_ctx* c, const PileCall& pc, const ioc_pileup_col* d_cols, const ioc_pileup_ins* d_ins,
                     const ioc_pileup_col* d_gate /* the weighted call: d_cols / d_ins are weights, this the counts; else NULL */, int64_t n_rows,
                     AlnTally& t)
{
    const size_t n = pc.segs.size();
    const size_t bound = size_t(pile_call_bound(pc.segs));
    auto up16 = [](size_t v) { return (v + 15) & ~size_t(15); };
    const size_t o_seg = 0, o_len = up16(n * sizeof(IocPileSeg)), o_off = o_len + up16(n * 8), o_st = o_off + up16((n + 1) * 8),
                 o_seq = o_st + n * sizeof(ioc_polish_stats), o_qual = o_seq + up16(bound), total = o_qual + up16(bound);
    IOC_TRY(ioc_reserve(c, c->a_call, total));
    uint8_t* p = static_cast<uint8_t*>(c->a_call.p);
    IOC_CHK(c, hipMemcpyAsync(p + o_seg, pc.segs.data(), n * sizeof(IocPileSeg), hipMemcpyHostToDevice, c->stream));
    EventSet ev;
    ev.v.assign(2, nullptr);
    for (auto& e : ev.v) IOC_CHK(c, hipEventCreate(&e));
    IOC_CHK(c, hipEventRecord(ev.v[0], c->stream));
    if (d_gate)
        IOC_CHK(c, iock_pile_call_weighted(c->stream, reinterpret_cast<const IocPileSeg*>(p + o_seg), uint32_t(n), d_gate, d_cols, d_ins,
                                           uint64_t(n_rows), pc.d_frames, pc.frame_bytes, pc.min_depth, reinterpret_cast<int64_t*>(p + o_len),
                                           reinterpret_cast<ioc_polish_stats*>(p + o_st), reinterpret_cast<int64_t*>(p + o_off), p + o_seq,
                                           p + o_qual, uint64_t(bound)));
    else
        IOC_CHK(c, iock_pile_call(c->stream, reinterpret_cast<const IocPileSeg*>(p + o_seg), uint32_t(n), d_cols, d_ins, uint64_t(n_rows), pc.d_frames,
                                  pc.frame_bytes, pc.min_depth, reinterpret_cast<int64_t*>(p + o_len), reinterpret_cast<ioc_polish_stats*>(p + o_st),
                                  reinterpret_cast<int64_t*>(p + o_off), p + o_seq, p + o_qual, uint64_t(bound)));
    IOC_CHK(c, hipEventRecord(ev.v[1], c->stream));
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    const auto t0 = std::chrono::steady_clock::now();
    IOC_CHK(c, hipMemcpy(pc.out_off, p + o_off, (n + 1) * 8, hipMemcpyDeviceToHost));
    const int64_t len = pc.out_off[n];
    if (len < 0 || size_t(len) > bound) return ioc_fail(c, IOC_ERR_HIP, "the consensus call returned a length outside its bound");
    if (pc.out_stats) IOC_CHK(c, hipMemcpy(pc.out_stats, p + o_st, n * sizeof(ioc_polish_stats), hipMemcpyDeviceToHost));
    if (len > 0) {
        IOC_CHK(c, hipMemcpy(pc.out_seq, p + o_seq, size_t(len), hipMemcpyDeviceToHost));
        IOC_CHK(c, hipMemcpy(pc.out_qual, p + o_qual, size_t(len), hipMemcpyDeviceToHost));
    }
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev.v[0], ev.v[1]) == hipSuccess) t.ms_call += double(ms);
    t.ms_copy += ms_since(t0);
    t.copied += int64_t((n + 1) * 8 + (pc.out_stats ? n * sizeof(ioc_polish_stats) : 0) + 2 * size_t(len));
    return IOC_OK;
}

// ioc_pileup_call (wcols NULL: cols / ins are called by majority) and ioc_pileup_call_weighted (cols gates, wcols / ins decide).
// The tables are uploaded and called where they lie then (ioc_pile_call.hip); the frames travel as one pool of bytes.
int pileup_call_tables(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off, const ioc_pileup_col* cols,
                       const ioc_pileup_col* wcols, const ioc_pileup_ins* ins, int32_t min_depth, char* out_seq, char* out_qual, int64_t cap,
                       int64_t* out_off, ioc_polish_stats* out_stats)
{
    std::vector<IocPileSeg> segs(static_cast<size_t>(n_segs));
    int64_t n_rows = 0, frame_bytes = 0;
    for (int32_t g = 0; g < n_segs; ++g) {
        if (rlen[g] < 0 || frame_off[g] < 0 || (rlen[g] > 0 && !frames)) return ioc_fail(c, IOC_ERR_ARG, "ioc_pileup_call: segment " + std::to_string(g) + " has a negative length or frame offset");
        if (int64_t(rlen[g]) + int64_t(IOC_PILE_INS_SLOTS) * (int64_t(rlen[g]) + 1) > INT32_MAX)  // (the record's out_len, the kernels' byte counts)
            return ioc_fail(c, IOC_ERR_CAPACITY, "ioc_pileup_call: segment " + std::to_string(g) + " may call more than 2^31 - 1 bytes");
        segs[size_t(g)] = IocPileSeg{n_rows, frame_off[g], rlen[g], 0};
        n_rows += int64_t(rlen[g]) + 1;
        frame_bytes = std::max(frame_bytes, frame_off[g] + rlen[g]);
    }
    const int64_t bound = pile_call_bound(segs);
    if (cap < bound) return ioc_fail(c, IOC_ERR_CAPACITY, "ioc_pileup_call: cap " + std::to_string(cap) + " below the bound " + std::to_string(bound));
    if (bound > 0 && (!out_seq || !out_qual)) return IOC_ERR_ARG;
    out_off[0] = 0;
    if (n_segs == 0) return IOC_OK;
    IOC_CHK(c, hipSetDevice(c->device));
    const size_t b_cols = size_t(n_rows) * sizeof(ioc_pileup_col), b_ins = size_t(n_rows) * sizeof(ioc_pileup_ins);
    IOC_TRY(ioc_reserve(c, c->a_pile, b_cols));
    IOC_TRY(ioc_reserve(c, c->a_pile_ins, b_ins));
    DevBuf d_frames;
    IOC_TRY(ioc_alloc(c, d_frames, size_t(frame_bytes)));
    IOC_CHK(c, hipMemcpyAsync(c->a_pile.p, cols, b_cols, hipMemcpyHostToDevice, c->stream));
    IOC_CHK(c, hipMemcpyAsync(c->a_pile_ins.p, ins, b_ins, hipMemcpyHostToDevice, c->stream));
    if (wcols) {
        IOC_TRY(ioc_reserve(c, c->a_pile_w, b_cols));
        IOC_CHK(c, hipMemcpyAsync(c->a_pile_w.p, wcols, b_cols, hipMemcpyHostToDevice, c->stream));
    }
    if (frame_bytes > 0) IOC_CHK(c, hipMemcpyAsync(d_frames.p, frames, size_t(frame_bytes), hipMemcpyHostToDevice, c->stream));
    AlnTally t;
    const PileCall pc{segs, static_cast<const uint8_t*>(d_frames.p), uint64_t(frame_bytes), min_depth, out_seq, out_qual, out_off, out_stats};
    IOC_TRY(pile_call_device(c, pc, wcols ? c->a_pile_w.as<ioc_pileup_col>() : c->a_pile.as<ioc_pileup_col>(), c->a_pile_ins.as<ioc_pileup_ins>(),
                             wcols ? c->a_pile.as<ioc_pileup_col>() : nullptr, n_rows, t));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   consensus call: %d segments, %lld rows, %lld bytes called, k_pile_call%s %.3f ms\n", n_segs, (long long)n_rows,
                (long long)out_off[n_segs], wcols ? "<weighted>" : "", t.ms_call);
    return IOC_OK;
}

// what a polish of the groups of a split is run with and where it leaves what it made (ioc_planes_polish's outputs)
struct GroupPolish {
    int32_t min_depth;
    char *out_seq, *out_qual;
    int64_t cap;
    int64_t* out_off;
    ioc_polish_stats* out_polish;
    ioc_pileup_col* out_gcols;
    ioc_pileup_ins* out_gins;
};

// what a group polish refuses once the segments are known: IOC_OK, or the status with the message set
int group_polish_ok(ioc_ctx* c, const std::string& who, const GroupPolish& gp, const std::vector<IocPileSeg>& ds)
{
    for (size_t g = 0; g < ds.size(); ++g)
        if (int64_t(ds[g].rlen) + int64_t(IOC_PILE_INS_SLOTS) * (int64_t(ds[g].rlen) + 1) > INT32_MAX)  // (the record's out_len, the kernels' byte counts)
            return ioc_fail(c, IOC_ERR_CAPACITY, who + ": segment " + std::to_string(g) + " may call more than 2^31 - 1 bytes");
    const int64_t bound = 2 * pile_call_bound(ds);
    if (gp.cap < bound) return ioc_fail(c, IOC_ERR_CAPACITY, who + ": cap " + std::to_string(gp.cap) + " below the bound " + std::to_string(bound));
    if (bound > 0 && (!gp.out_seq || !gp.out_qual)) return IOC_ERR_ARG;
    return IOC_OK;
}

// where the planes, the member lists and the group bytes of a group polish lie on the device; a NULL pointer: the host's array is
// uploaded (ioc_planes_polish: all of them; behind a split: none)
struct PlanesDev {
    const uint32_t *mem_off, *members;
    const uint8_t *group, *base, *slots;
    uint64_t plane_bytes;
};
struct PlanesHost {
    const int32_t* seg_of_pair;
    const uint8_t* group;  // per pair: 0, 1 or IOC_SPLIT_NONE
    const int64_t* plane;  // per pair: where its rows start in every plane
    const uint8_t *base, *slots;
};

// k_plane_pile and the call kernels over the 2 n group-segments of the segments ds (frames in d_frames): a_gpile holds
// [group-segments][work items][plane offsets][mem_off][members][group][base plane][slot planes][gcols][gins], the middle five only
// where they are uploaded.  Group-segment 2 g + h owns the rows 2 * row0(g) + h * (rlen(g) + 1) .. of both tables, which are set
// to 0 first: k_plane_pile is launched over the group-segments that have reads alone.  Device times go to t.ms_plane_pile /
// t.ms_call, the copies to t.ms_copy / t.copied.
int group_polish_device(ioc_ctx* c, const GroupPolish& gp, const std::vector<IocPileSeg>& ds, const uint8_t* d_frames, uint64_t frame_bytes, size_t np,
                        const PlanesHost& ph, PlanesDev pd, AlnTally& t)
{
    const size_t n = ds.size();
    std::vector<IocPileSeg> gsegs(2 * n);
    std::vector<uint32_t> reads(2 * n, 0);
    int64_t n_rows = 0;
    for (size_t g = 0; g < n; ++g)
        for (int64_t h = 0; h < 2; ++h) {
            gsegs[2 * g + size_t(h)] = IocPileSeg{2 * ds[g].row0 + h * (int64_t(ds[g].rlen) + 1), ds[g].f_off, ds[g].rlen, ds[g].rc};
            n_rows += int64_t(ds[g].rlen) + 1;
        }
    for (size_t i = 0; i < np; ++i)
        if (ph.group[i] <= 1) ++reads[2 * size_t(ph.seg_of_pair[i]) + ph.group[i]];
    std::vector<IocPlaneWork> work;
    for (size_t x = 0; x < 2 * n; ++x)
        for (int64_t row = 0; reads[x] > 0 && row <= int64_t(gsegs[x].rlen); row += IOC_PLANE_PILE_ROWS) work.push_back(IocPlaneWork{uint32_t(x), uint32_t(row)});
    if (work.size() > size_t(INT32_MAX)) return ioc_fail(c, IOC_ERR_CAPACITY, "the group tables have more than 2^31 - 1 blocks of rows");
    std::vector<uint32_t> mem_off, members;
    if (!pd.members) {  // (a segment's reads are its pairs in ascending order, as the split has them)
        mem_off.assign(n + 1, 0), members.resize(np);
        for (size_t i = 0; i < np; ++i) ++mem_off[size_t(ph.seg_of_pair[i]) + 1];
        for (size_t g = 0; g < n; ++g) mem_off[g + 1] += mem_off[g];
        std::vector<uint32_t> next(mem_off.begin(), mem_off.end() - 1);
        for (size_t i = 0; i < np; ++i) members[next[size_t(ph.seg_of_pair[i])]++] = uint32_t(i);
    }
    const size_t P = size_t(pd.plane_bytes);
    auto up16 = [](size_t v) { return (v + 15) & ~size_t(15); };
    size_t at = 0;
    auto take = [&](size_t b) { const size_t o = at; at += up16(b); return o; };
    const size_t o_gseg = take(2 * n * sizeof(IocPileSeg)), o_work = take(work.size() * sizeof(IocPlaneWork)), o_plane = take(np * 8),
                 o_moff = take(pd.members ? 0 : (n + 1) * 4), o_mem = take(pd.members ? 0 : np * 4), o_group = take(pd.group ? 0 : np),
                 o_base = take(pd.base ? 0 : P), o_slots = take(pd.slots ? 0 : size_t(IOC_PILE_INS_SLOTS) * P),
                 o_cols = take(size_t(n_rows) * sizeof(ioc_pileup_col)), o_ins = take(size_t(n_rows) * sizeof(ioc_pileup_ins));
    IOC_CHK(c, hipSetDevice(c->device));
    IOC_TRY(ioc_reserve(c, c->a_gpile, at));
    uint8_t* p = static_cast<uint8_t*>(c->a_gpile.p);
    auto up = [&](size_t o, const void* src, size_t b) { return b ? hipMemcpyAsync(p + o, src, b, hipMemcpyHostToDevice, c->stream) : hipSuccess; };
    IOC_CHK(c, up(o_gseg, gsegs.data(), 2 * n * sizeof(IocPileSeg)));
    IOC_CHK(c, up(o_work, work.data(), work.size() * sizeof(IocPlaneWork)));
    IOC_CHK(c, up(o_plane, ph.plane, np * 8));
    if (!pd.members) {
        IOC_CHK(c, up(o_moff, mem_off.data(), (n + 1) * 4));
        IOC_CHK(c, up(o_mem, members.data(), np * 4));
        pd.mem_off = reinterpret_cast<const uint32_t*>(p + o_moff), pd.members = reinterpret_cast<const uint32_t*>(p + o_mem);
    }
    if (!pd.group) {
        IOC_CHK(c, up(o_group, ph.group, np));
        pd.group = p + o_group;
    }
    if (!pd.base) {
        IOC_CHK(c, up(o_base, ph.base, P));
        pd.base = p + o_base;
    }
    if (!pd.slots) {
        IOC_CHK(c, up(o_slots, ph.slots, size_t(IOC_PILE_INS_SLOTS) * P));
        pd.slots = p + o_slots;
    }
    ioc_pileup_col* const d_cols = reinterpret_cast<ioc_pileup_col*>(p + o_cols);
    ioc_pileup_ins* const d_ins = reinterpret_cast<ioc_pileup_ins*>(p + o_ins);
    if (n_rows > 0) IOC_CHK(c, hipMemsetAsync(p + o_cols, 0, at - o_cols, c->stream));
    EventSet ev;
    ev.v.assign(2, nullptr);
    for (auto& e : ev.v) IOC_CHK(c, hipEventCreate(&e));
    IOC_CHK(c, hipEventRecord(ev.v[0], c->stream));
    IOC_CHK(c, iock_plane_pile(c->stream, reinterpret_cast<const IocPlaneWork*>(p + o_work), uint32_t(work.size()), reinterpret_cast<const IocPileSeg*>(p + o_gseg),
                               pd.mem_off, pd.members, uint32_t(np), pd.group, reinterpret_cast<const uint64_t*>(p + o_plane), pd.base, pd.slots,
                               pd.plane_bytes, d_cols, d_ins, uint64_t(n_rows)));
    IOC_CHK(c, hipEventRecord(ev.v[1], c->stream));
    const PileCall pc{gsegs, d_frames, frame_bytes, gp.min_depth, gp.out_seq, gp.out_qual, gp.out_off, gp.out_polish};
    IOC_TRY(pile_call_device(c, pc, d_cols, d_ins, nullptr, n_rows, t));  // (waits for the stream)
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev.v[0], ev.v[1]) == hipSuccess) t.ms_plane_pile += double(ms);
    const auto t0 = std::chrono::steady_clock::now();
    const struct { void* dst; const void* src; size_t bytes; } outs[] = {{gp.out_gcols, d_cols, size_t(n_rows) * sizeof(ioc_pileup_col)},
                                                                         {gp.out_gins, d_ins, size_t(n_rows) * sizeof(ioc_pileup_ins)}};
    for (const auto& o : outs)
        if (o.dst && o.bytes) {
            IOC_CHK(c, hipMemcpy(o.dst, o.src, o.bytes, hipMemcpyDeviceToHost));
            t.copied += int64_t(o.bytes);
        }
    t.ms_copy += ms_since(t0);
    return IOC_OK;
}

// What ioc_align_pairs_pileup and the polish calls share.  The tables of `kind`, n_rows records each — a_pile; a_pile_ins beside it
// (ins), or a_pile_w as [wcols][wins] (weighted) — are reserved and zeroed, the pairs aligned into them (k_ops_pileup adds, where
// the walks' bytes lie, slice after slice and re-run after re-run) and, where `call` is given, called where they lie; then the
// tables asked for are copied out, once.  out_ins: the second table of its kind (ins, or wins).  `sites` (ioc_align_pairs_alleles):
// every pair is projected as well, into the planes of a_planes, [base planes][ins planes] and, where the call polishes the groups
// of a split, [slot planes x 6] behind them, set to IOC_ALLELE_NONE / 0 once here, and the sites are found and the alleles
// gathered where the table and the planes lie.
static int align_pairs_piled(ioc_ctx* c, const AlnCall& a, PileKind kind, ioc_aln_stats* out_stats, const int64_t* row_base, int64_t n_rows,
                             const PileCall* call, ioc_pileup_col* out_cols, ioc_pileup_col* out_wcols, ioc_pileup_ins* out_ins, AlnTally& t,
                             const SitesCall* sites = nullptr)
{
    IOC_CHK(c, hipSetDevice(c->device));
    const size_t b_cols = size_t(n_rows) * sizeof(ioc_pileup_col), b_ins = size_t(n_rows) * sizeof(ioc_pileup_ins);
    std::vector<int64_t> len(size_t(a.n_pairs), 0);
    std::vector<uint8_t> piled(size_t(a.n_pairs), 0);
    const bool weighted = kind == PileKind::weighted;
    DevBuf* second = kind == PileKind::ins ? &c->a_pile_ins : weighted ? &c->a_pile_w : nullptr;  // [ins], or [wcols][wins]
    const size_t b_second = weighted ? b_cols + b_ins : b_ins;
    IOC_TRY(ioc_reserve(c, c->a_pile, b_cols));
    if (second) IOC_TRY(ioc_reserve(c, *second, b_second));
    IOC_CHK(c, hipMemsetAsync(c->a_pile.p, 0, b_cols, c->stream));
    if (second) IOC_CHK(c, hipMemsetAsync(second->p, 0, b_second, c->stream));
    AlnSink::Pile pl{kind, c->a_pile.as<ioc_pileup_col>(), nullptr, nullptr, nullptr, n_rows, row_base, piled.data()};
    if (kind == PileKind::ins) pl.ins = second->as<ioc_pileup_ins>();
    if (weighted) pl.wcols = second->as<ioc_pileup_col>(), pl.wins = reinterpret_cast<ioc_pileup_ins*>(second->as<uint8_t>() + b_cols);  // (b_cols: a multiple of 32)
    if (sites) {
        const size_t b_plane = size_t(sites->plane_bytes);
        IOC_TRY(ioc_reserve(c, c->a_planes, (sites->project_ins ? 2 + size_t(IOC_PILE_INS_SLOTS) : 2) * b_plane));
        pl.project = true, pl.base_planes = c->a_planes.as<uint8_t>(), pl.ins_planes = pl.base_planes + b_plane;
        pl.plane_bytes = sites->plane_bytes, pl.plane = sites->plane;
        if (sites->project_ins) pl.project_ins = true, pl.slot_planes = pl.base_planes + 2 * b_plane;
        if (b_plane > 0) {
            IOC_CHK(c, hipMemsetAsync(pl.base_planes, IOC_ALLELE_NONE, b_plane, c->stream));
            IOC_CHK(c, hipMemsetAsync(pl.ins_planes, 0, (sites->project_ins ? 1 + size_t(IOC_PILE_INS_SLOTS) : 1) * b_plane, c->stream));  // (and the slot planes)
        }
    }
    const AlnSink sink{SinkKind::reduced, len.data(), &t, {}, out_stats != nullptr, out_stats, pl};
    IOC_TRY(a.run(c, a.n_pairs > 0 ? &sink : nullptr));
    if (sites)
        IOC_TRY(pile_sites_device(c, *sites, pl.cols, n_rows, pl.base_planes, pl.ins_planes, t));
    else if (call)
        IOC_TRY(pile_call_device(c, *call, weighted ? pl.wcols : pl.cols, weighted ? pl.wins : pl.ins, weighted ? pl.cols : nullptr, n_rows, t));
    else
        IOC_CHK(c, hipStreamSynchronize(c->stream));
    const auto t0 = std::chrono::steady_clock::now();
    const struct { void* dst; const void* src; size_t bytes; } outs[] = {{out_cols, pl.cols, b_cols}, {out_wcols, pl.wcols, b_cols}, {out_ins, weighted ? pl.wins : pl.ins, b_ins}};
    for (const auto& o : outs)
        if (o.dst) {
            IOC_CHK(c, hipMemcpy(o.dst, o.src, o.bytes, hipMemcpyDeviceToHost));
            t.copied += int64_t(o.bytes);
        }
    t.ms_copy += ms_since(t0);
    return IOC_OK;
}

// ioc_align_pairs_pileup with the second table beside the first, and the call kernels over both where they lie: what comes back
// is the called bytes (at most 7 per row), not the tables, unless they are asked for.  weighted (ioc_align_pairs_polish_weighted):
// the weighted variant of k_ops_pileup adds the counts into the first table and the weights into two tables of a_pile_w, [wcols]
// [wins], and the call is the weighted one; out_ins is then out_wins.
int align_pairs_polish(ioc_ctx* c, const AlnCall& a, ioc_aln_stats* out_stats, int32_t n_segs, const ioc_polish_seg* segs, const int32_t* seg_of_pair,
                       int32_t min_depth, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_polish,
                       ioc_pileup_col* out_cols, ioc_pileup_ins* out_ins, bool weighted, ioc_pileup_col* out_wcols)
{
    if (!c || a.n_pairs < 0 || n_segs < 0 || min_depth < 1 || !out_off || cap < 0 || (a.n_pairs > 0 && (!a.pairs || !seg_of_pair)) ||
        (n_segs > 0 && (!segs || !out_polish)))
        return IOC_ERR_ARG;
    if (weighted && !c->aln_qual_set) return ioc_fail(c, IOC_ERR_ARG, "ioc_align_pairs_polish_weighted: no qualities are set for the current pool (ioc_align_set_pool_qual)");
    const int64_t n_seqs = c->aln_offs.empty() ? 0 : int64_t(c->aln_offs.size()) - 1;
    std::vector<IocPileSeg> ds(static_cast<size_t>(n_segs));
    int64_t n_rows = 0;
    for (int32_t g = 0; g < n_segs; ++g) {
        if (segs[g].ref < 0 || segs[g].ref >= n_seqs) return ioc_fail(c, IOC_ERR_ARG, "ioc_align_pairs_polish: segment " + std::to_string(g) + " refers to a sequence outside the pool");
        const int64_t m = ioc_seq_len(c, segs[g].ref);
        ds[size_t(g)] = IocPileSeg{n_rows, c->aln_offs[size_t(segs[g].ref)], int32_t(m), segs[g].ref_revcomp ? 1 : 0};
        n_rows += m + 1;
    }
    std::vector<int64_t> row_base(size_t(a.n_pairs), 0);
    for (int32_t i = 0; i < a.n_pairs; ++i) {
        IOC_TRY(ioc_pair_in_pool(c, a.pairs[i]));
        if (seg_of_pair[i] < 0 || seg_of_pair[i] >= n_segs) return ioc_fail(c, IOC_ERR_ARG, "ioc_align_pairs_polish: pair " + std::to_string(i) + " names no segment");
        if (ioc_seq_len(c, a.pairs[i].ref) != ds[size_t(seg_of_pair[i])].rlen)
            return ioc_fail(c, IOC_ERR_ARG, "ioc_align_pairs_polish: the reference of pair " + std::to_string(i) + " is not as long as its segment's frame");
        row_base[size_t(i)] = ds[size_t(seg_of_pair[i])].row0;
    }
    const int64_t bound = pile_call_bound(ds);
    if (cap < bound) return ioc_fail(c, IOC_ERR_CAPACITY, "ioc_align_pairs_polish: cap " + std::to_string(cap) + " below the bound " + std::to_string(bound));
    if (bound > 0 && (!out_seq || !out_qual)) return IOC_ERR_ARG;
    for (int32_t i = 0; i < a.n_pairs && out_stats; ++i) out_stats[i] = ioc_aln_stats{};
    out_off[0] = 0;
    if (n_segs == 0) return a.run(c, nullptr);
    AlnTally t;
    const PileCall pc{ds, static_cast<const uint8_t*>(c->a_pool.p), uint64_t(c->aln_offs.back()), min_depth, out_seq, out_qual, out_off, out_polish};
    IOC_TRY(align_pairs_piled(c, a, weighted ? PileKind::weighted : PileKind::ins, out_stats, row_base.data(), n_rows, &pc, out_cols, out_wcols, out_ins, t));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner: polish: %d segments, %lld rows, %.3f MB (called bytes, records, lengths%s%s) copied from the device in %.3f ms, k_ops_pileup<%s> %.3f ms, k_pile_call%s %.3f ms%s\n",
                n_segs, (long long)n_rows, double(t.copied) * 1e-6, out_cols || out_ins || out_wcols ? ", tables" : "", out_stats ? ", statistics" : "", t.ms_copy,
                weighted ? "weighted" : "ins", t.ms_pileup, weighted ? "<weighted>" : "", t.ms_call, out_stats ? (", k_ops_stats " + std::to_string(t.ms_stats) + " ms").c_str() : "");
    return IOC_OK;
}

}  // namespace

int64_t ioc_align_ops_bound(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs)
{
    if (!c || n_pairs < 0 || (n_pairs > 0 && !pairs)) return IOC_ERR_ARG;
    int64_t bound = 0;
    for (int32_t i = 0; i < n_pairs; ++i) {
        IOC_TRY(ioc_pair_in_pool(c, pairs[i]));
        bound += ioc_seq_len(c, pairs[i].query) + ioc_seq_len(c, pairs[i].ref);
    }
    return bound;
}

// The walks write a pair's bytes into a region of its own of the caller's buffer (as long as the pair's share of the bound);
// the regions are packed when all runs — the call's own, the re-runs' — are over.
int ioc_align_pairs_ops(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                        int32_t* out_score, int64_t* out_windows, double* out_ratio, char* out_ops, int64_t ops_cap, int64_t* ops_off)
{
    if (!c || n_pairs < 0 || (n_pairs > 0 && !pairs) || !ops_off || ops_cap < 0 || (ops_cap > 0 && !out_ops)) return IOC_ERR_ARG;
    const int64_t bound = ioc_align_ops_bound(c, n_pairs, pairs);
    if (bound < 0) return int(bound);
    if (ops_cap < bound) return ioc_fail(c, IOC_ERR_CAPACITY, "ioc_align_pairs_ops: ops_cap " + std::to_string(ops_cap) + " below the bound " + std::to_string(bound));
    std::vector<int64_t> base(size_t(n_pairs) + 1, 0), len(size_t(n_pairs), 0);
    for (int32_t i = 0; i < n_pairs; ++i) base[size_t(i) + 1] = base[size_t(i)] + ioc_seq_len(c, pairs[i].query) + ioc_seq_len(c, pairs[i].ref);
    AlnTally t;
    const AlnSink sink{SinkKind::bytes, len.data(), &t, {reinterpret_cast<uint8_t*>(out_ops), base.data()}};
    IOC_TRY((AlnCall{n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}.run(c, &sink)));
    ops_off[0] = 0;
    for (int32_t i = 0; i < n_pairs; ++i) {  // (a packed position never lies behind the region's own)
        if (len[size_t(i)] > 0 && ops_off[i] != base[size_t(i)]) memmove(out_ops + ops_off[i], out_ops + base[size_t(i)], size_t(len[size_t(i)]));
        ops_off[i + 1] = ops_off[i] + len[size_t(i)];
    }
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner: operation bytes: %.1f MB copied from the device in %.3f ms, %.1f MB packed\n", double(t.copied) * 1e-6, t.ms_copy,
                double(ops_off[n_pairs]) * 1e-6);
    return IOC_OK;
}

// The walks write a slice's bytes as for ioc_align_pairs_ops; k_ops_stats (ioc_ops_stats.hip) reduces them where they lie, and
// the records of the run that counted — the call's own, a re-run's — end up in out_stats.
int ioc_align_pairs_stats(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                          int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats)
{
    if (!c || n_pairs < 0 || (n_pairs > 0 && (!pairs || !out_stats))) return IOC_ERR_ARG;
    for (int32_t i = 0; i < n_pairs && out_stats; ++i) out_stats[i] = ioc_aln_stats{};
    std::vector<int64_t> len(size_t(n_pairs), 0);
    AlnTally t;
    const AlnSink sink{SinkKind::reduced, len.data(), &t, {}, true, out_stats};
    IOC_TRY((AlnCall{n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}.run(c, &sink)));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner: alignment statistics: %lld records (%.3f MB with the lengths) copied from the device in %.3f ms, k_ops_stats %.3f ms\n",
                (long long)t.records, double(t.copied) * 1e-6, t.ms_copy, t.ms_stats);
    return IOC_OK;
}

// The walks write a slice's bytes as for ioc_align_pairs_ops; k_ops_pileup (ioc_ops_pileup.hip) adds them, where they lie, into a
// table of the call's rows that stays on the device over the slices and the re-runs and is copied out once.
int ioc_align_pairs_pileup(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                           int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, const int64_t* row_base, int64_t
                           n_rows, ioc_pileup_col* out_cols)
{
    if (!c || n_pairs < 0 || n_rows < 0 || (n_pairs > 0 && (!pairs || !row_base || !out_cols))) return IOC_ERR_ARG;
    for (int32_t i = 0; i < n_pairs; ++i) {
        IOC_TRY(ioc_pair_in_pool(c, pairs[i]));
        if (row_base[i] < 0 || row_base[i] > n_rows - ioc_seq_len(c, pairs[i].ref) - 1)
            return ioc_fail(c, IOC_ERR_ARG, "ioc_align_pairs_pileup: the rows of pair " + std::to_string(i) + " lie outside the table");
    }
    for (int32_t i = 0; i < n_pairs && out_stats; ++i) out_stats[i] = ioc_aln_stats{};
    if (out_cols && n_rows > 0) memset(out_cols, 0, size_t(n_rows) * sizeof(ioc_pileup_col));
    const AlnCall a{n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio};
    if (n_pairs == 0 || n_rows == 0) return a.run(c, nullptr);
    AlnTally t;
    IOC_TRY(align_pairs_piled(c, a, PileKind::counts, out_stats, row_base, n_rows, nullptr, out_cols, nullptr, nullptr, t));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner: pileup: %lld rows, %.3f MB (table, lengths%s) copied from the device in %.3f ms, k_ops_pileup %.3f ms%s\n",
                (long long)n_rows, double(t.copied) * 1e-6, out_stats ? ", statistics" : "", t.ms_copy, t.ms_pileup,
                out_stats ? (", k_ops_stats " + std::to_string(t.ms_stats) + " ms").c_str() : "");
    return IOC_OK;
}

int ioc_pileup_sites(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, const ioc_pileup_col* cols, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                     int32_t max_sites, ioc_pile_site* out_sites, int64_t sites_cap, int64_t* site_off, int64_t* n_found)
{
    if (!c || n_segs < 0 || !sites_rule_ok(min_depth, min_alt, min_pct, max_sites) || !site_off || sites_cap < 0 ||
        (n_segs > 0 && (!rlen || !cols || !n_found)))
        return IOC_ERR_ARG;
    std::vector<IocPileSeg> segs(static_cast<size_t>(n_segs));
    int64_t n_rows = 0;
    for (int32_t g = 0; g < n_segs; ++g) {
        if (rlen[g] < 0) return ioc_fail(c, IOC_ERR_ARG, "ioc_pileup_sites: segment " + std::to_string(g) + " has a negative length");
        if (rlen[g] > (1 << 30)) return ioc_fail(c, IOC_ERR_CAPACITY, "ioc_pileup_sites: segment " + std::to_string(g) + " is longer than 2^30 bases");
        segs[size_t(g)] = IocPileSeg{n_rows, 0, rlen[g], 0};
        n_rows += int64_t(rlen[g]) + 1;
    }
    const int64_t bound = pile_sites_bound(segs, max_sites);
    if (sites_cap < bound) return ioc_fail(c, IOC_ERR_CAPACITY, "ioc_pileup_sites: sites_cap " + std::to_string(sites_cap) + " below the bound " + std::to_string(bound));
    if (bound > 0 && !out_sites) return IOC_ERR_ARG;
    site_off[0] = 0;
    if (n_segs == 0) return IOC_OK;
    IOC_CHK(c, hipSetDevice(c->device));
    const size_t b_cols = size_t(n_rows) * sizeof(ioc_pileup_col);
    IOC_TRY(ioc_reserve(c, c->a_pile, b_cols));
    IOC_CHK(c, hipMemcpyAsync(c->a_pile.p, cols, b_cols, hipMemcpyHostToDevice, c->stream));
    AlnTally t;
    const SitesCall sc{segs, min_depth, min_alt, min_pct, max_sites, out_sites, site_off, n_found};
    IOC_TRY(pile_sites_device(c, sc, c->a_pile.as<ioc_pileup_col>(), n_rows, nullptr, nullptr, t));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   site search: %d segments, %lld rows, %lld sites kept, k_pile_sites %.3f ms\n", n_segs, (long long)n_rows,
                (long long)site_off[n_segs], t.ms_sites);
    return IOC_OK;
}

// ioc_align_pairs_pileup into the rows of the segments, with every pair projected beside it, and the site kernels over the table
// and the planes where they lie: what comes back is the sites and one byte per (pair, kept site of its segment).
// (`split`: ioc_align_pairs_split — the split runs behind k_site_alleles, out_alleles is optional)
static int align_pairs_alleles(const char* who_, ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch,
                               int32_t gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                               const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                               int32_t max_sites, ioc_pile_site* out_sites, int64_t sites_cap, int64_t* site_off, int64_t* n_found, uint8_t* out_alleles,
                               int64_t alleles_cap, int64_t* allele_off, ioc_pileup_col* out_cols, const SplitCall* split,
                               const GroupPolish* gp = nullptr /* (ioc_align_pairs_split_polish, with `split`) both groups of every segment are called */)
{
    const std::string who = who_;
    if (gp && (!split || gp->min_depth < 1 || !gp->out_off || gp->cap < 0)) return IOC_ERR_ARG;
    if (split && (!split_rule_ok(split->min_link, split->min_margin, split->rounds) || (n_pairs > 0 && !split->out_group) || (n_segs > 0 && !split->out_seg)))
        return IOC_ERR_ARG;
    if (!c || n_pairs < 0 || n_segs < 0 || !sites_rule_ok(min_depth, min_alt, min_pct, max_sites) || !site_off || !allele_off || sites_cap < 0 ||
        alleles_cap < 0 || (n_pairs > 0 && (!pairs || !seg_of_pair)) || (n_segs > 0 && (!segs || !n_found)))
        return IOC_ERR_ARG;
    const AlnCall a{n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio};
    const int64_t n_seqs = c->aln_offs.empty() ? 0 : int64_t(c->aln_offs.size()) - 1;
    std::vector<IocPileSeg> ds(static_cast<size_t>(n_segs));
    int64_t n_rows = 0;
    for (int32_t g = 0; g < n_segs; ++g) {
        if (segs[g].ref < 0 || segs[g].ref >= n_seqs) return ioc_fail(c, IOC_ERR_ARG, who + ": segment " + std::to_string(g) + " refers to a sequence outside the pool");
        const int64_t m = ioc_seq_len(c, segs[g].ref);
        if (m > (1 << 30)) return ioc_fail(c, IOC_ERR_CAPACITY, who + ": segment " + std::to_string(g) + " is longer than 2^30 bases");
        ds[size_t(g)] = IocPileSeg{n_rows, c->aln_offs[size_t(segs[g].ref)], int32_t(m), segs[g].ref_revcomp ? 1 : 0};
        n_rows += m + 1;
    }
    std::vector<int64_t> row_base(size_t(n_pairs), 0), plane(size_t(n_pairs), 0);
    int64_t plane_bytes = 0, alleles_bound = 0;
    for (int32_t i = 0; i < n_pairs; ++i) {
        IOC_TRY(ioc_pair_in_pool(c, pairs[i]));
        if (seg_of_pair[i] < 0 || seg_of_pair[i] >= n_segs) return ioc_fail(c, IOC_ERR_ARG, who + ": pair " + std::to_string(i) + " names no segment");
        const IocPileSeg& sg = ds[size_t(seg_of_pair[i])];
        if (ioc_seq_len(c, pairs[i].ref) != sg.rlen)
            return ioc_fail(c, IOC_ERR_ARG, who + ": the reference of pair " + std::to_string(i) + " is not as long as its segment's frame");
        row_base[size_t(i)] = sg.row0;
        plane[size_t(i)] = plane_bytes;
        plane_bytes += int64_t(sg.rlen) + 1;
        alleles_bound += std::min<int64_t>(max_sites, 2 * int64_t(sg.rlen) + 1);
    }
    const int64_t bound = pile_sites_bound(ds, max_sites);
    if (sites_cap < bound) return ioc_fail(c, IOC_ERR_CAPACITY, who + ": sites_cap " + std::to_string(sites_cap) + " below the bound " + std::to_string(bound));
    if ((out_alleles || !split) && alleles_cap < alleles_bound)
        return ioc_fail(c, IOC_ERR_CAPACITY, who + ": alleles_cap " + std::to_string(alleles_cap) + " below the bound " + std::to_string(alleles_bound));
    if ((bound > 0 && !out_sites) || (alleles_bound > 0 && !out_alleles && !split)) return IOC_ERR_ARG;
    if (gp) IOC_TRY(group_polish_ok(c, who, *gp, ds));
    for (int32_t i = 0; i < n_pairs && out_stats; ++i) out_stats[i] = ioc_aln_stats{};
    if (gp) gp->out_off[0] = 0;
    site_off[0] = 0;
    for (int32_t i = 0; i <= n_pairs; ++i) allele_off[i] = 0;
    if (n_segs == 0) return a.run(c, nullptr);
    AlnTally t;
    SplitCall::Laid laid;
    SplitCall sp_laid = split ? *split : SplitCall{};
    sp_laid.laid = &laid;
    const SitesCall sc{ds, min_depth, min_alt, min_pct, max_sites, out_sites, site_off, n_found, n_pairs, seg_of_pair, plane.data(), plane_bytes,
                       alleles_bound, out_alleles, allele_off, gp ? &sp_laid : split, gp != nullptr};
    IOC_TRY(align_pairs_piled(c, a, PileKind::counts, out_stats, row_base.data(), n_rows, nullptr, out_cols, nullptr, nullptr, t, &sc));
    if (gp) {  // (the planes are where the walks left them, the lists and the group bytes where the split did; the groups are the host's too)
        const uint8_t* planes = c->a_planes.as<uint8_t>();
        const PlanesDev pd{laid.mem_off, laid.members, laid.group, planes, planes + 2 * size_t(plane_bytes), uint64_t(plane_bytes)};
        if (!pd.members || !pd.group) return ioc_fail(c, IOC_ERR_HIP, who + ": the split left no member lists");
        IOC_TRY(group_polish_device(c, *gp, ds, static_cast<const uint8_t*>(c->a_pool.p), uint64_t(c->aln_offs.back()), size_t(n_pairs),
                                    PlanesHost{seg_of_pair, split->out_group, plane.data(), nullptr, nullptr}, pd, t));
    }
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner: sites: %d segments, %lld rows, %lld sites kept, %lld allele bytes, %.3f MB (sites, alleles, lengths%s%s) copied from the device in %.3f ms, k_ops_pileup %.3f ms, k_ops_project %.3f ms, k_pile_sites %.3f ms, k_site_alleles %.3f ms%s\n",
                n_segs, (long long)n_rows, (long long)site_off[n_segs], (long long)allele_off[n_pairs], double(t.copied) * 1e-6, out_cols ? ", table" : "",
                out_stats ? ", statistics" : "", t.ms_copy, t.ms_pileup, t.ms_project, t.ms_sites, t.ms_alleles,
                out_stats ? (", k_ops_stats " + std::to_string(t.ms_stats) + " ms").c_str() : "");
    if (split && getenv("IOC_TRACE")) fprintf(stderr, "[ioc]   aligner: split: %s\n", split_trace(t).c_str());
    if (gp && getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner: split polish: %d group-segments, %lld bytes called, k_ops_project_ins %.3f ms, k_plane_pile %.3f ms, k_pile_call %.3f ms\n",
                2 * n_segs, (long long)gp->out_off[2 * n_segs], t.ms_project_ins, t.ms_plane_pile, t.ms_call);
    return IOC_OK;
}

int ioc_align_pairs_alleles(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                            int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                            const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_sites,
                            ioc_pile_site* out_sites, int64_t sites_cap, int64_t* site_off, int64_t* n_found, uint8_t* out_alleles, int64_t alleles_cap,
                            int64_t* allele_off, ioc_pileup_col* out_cols)
{
    return align_pairs_alleles("ioc_align_pairs_alleles", c, n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio, out_stats,
                               n_segs, segs, seg_of_pair, min_depth, min_alt, min_pct, max_sites, out_sites, sites_cap, site_off, n_found, out_alleles,
                               alleles_cap, allele_off, out_cols, nullptr);
}

// ioc_align_pairs_alleles with the split kernels (ioc_site_split.hip) run over the sites and the alleles where k_pile_sites and
// k_site_alleles left them: one byte per read comes back, and the alleles only where they are asked for.
int ioc_align_pairs_split(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                          int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                          const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_sites,
                          ioc_pile_site* out_sites, int64_t sites_cap, int64_t* site_off, int64_t* n_found, uint8_t* out_alleles, int64_t alleles_cap,
                          int64_t* allele_off, ioc_pileup_col* out_cols, int32_t min_link, int32_t min_margin, int32_t rounds, int64_t* out_link,
                          int8_t* out_phase, uint8_t* out_group, int32_t* out_vote, ioc_split_seg* out_seg)
{
    const SplitCall sp{min_link, min_margin, rounds, out_link, out_phase, out_group, out_vote, out_seg};
    return align_pairs_alleles("ioc_align_pairs_split", c, n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio, out_stats,
                               n_segs, segs, seg_of_pair, min_depth, min_alt, min_pct, max_sites, out_sites, sites_cap, site_off, n_found, out_alleles,
                               alleles_cap, allele_off, out_cols, &sp);
}

// ioc_align_pairs_split with the six slot planes projected beside the two, and behind k_split_record k_plane_pile and the call
// kernels over the planes: the consensus of both groups of every segment, with no pair aligned a second time.
int ioc_align_pairs_split_polish(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                                 int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                                 const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                                 int32_t max_sites, ioc_pile_site* out_sites, int64_t sites_cap, int64_t* site_off, int64_t* n_found, uint8_t* out_alleles,
                                 int64_t alleles_cap, int64_t* allele_off, ioc_pileup_col* out_cols, int32_t min_link, int32_t min_margin, int32_t rounds,
                                 int64_t* out_link, int8_t* out_phase, uint8_t* out_group, int32_t* out_vote, ioc_split_seg* out_seg,
                                 int32_t polish_min_depth, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_polish,
                                 ioc_pileup_col* out_gcols, ioc_pileup_ins* out_gins)
{
    const SplitCall sp{min_link, min_margin, rounds, out_link, out_phase, out_group, out_vote, out_seg};
    const GroupPolish gp{polish_min_depth, out_seq, out_qual, cap, out_off, out_polish, out_gcols, out_gins};
    return align_pairs_alleles("ioc_align_pairs_split_polish", c, n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio,
                               out_stats, n_segs, segs, seg_of_pair, min_depth, min_alt, min_pct, max_sites, out_sites, sites_cap, site_off, n_found,
                               out_alleles, alleles_cap, allele_off, out_cols, &sp, &gp);
}

// The group polish from planes the caller holds: everything is uploaded, and the kernels run as behind ioc_align_pairs_split_polish.
int ioc_planes_polish(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off, int32_t n_pairs,
                      const int32_t* seg_of_pair, const uint8_t* group, const uint8_t* base, const uint8_t* slots, int32_t min_depth, char* out_seq,
                      char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_polish, ioc_pileup_col* out_gcols, ioc_pileup_ins* out_gins)
{
    if (!c || n_segs < 0 || n_pairs < 0 || min_depth < 1 || !out_off || cap < 0 || (n_segs > 0 && (!rlen || !frame_off)) ||
        (n_pairs > 0 && (!seg_of_pair || !group)))
        return IOC_ERR_ARG;
    std::vector<IocPileSeg> ds(static_cast<size_t>(n_segs));
    int64_t n_rows = 0, frame_bytes = 0;
    for (int32_t g = 0; g < n_segs; ++g) {
        if (rlen[g] < 0 || frame_off[g] < 0 || (rlen[g] > 0 && !frames)) return ioc_fail(c, IOC_ERR_ARG, "ioc_planes_polish: segment " + std::to_string(g) + " has a negative length or frame offset");
        ds[size_t(g)] = IocPileSeg{n_rows, frame_off[g], rlen[g], 0};
        n_rows += int64_t(rlen[g]) + 1;
        frame_bytes = std::max(frame_bytes, frame_off[g] + rlen[g]);
    }
    std::vector<int64_t> plane(size_t(n_pairs), 0);
    int64_t plane_bytes = 0;
    for (int32_t i = 0; i < n_pairs; ++i) {
        if (seg_of_pair[i] < 0 || seg_of_pair[i] >= n_segs) return ioc_fail(c, IOC_ERR_ARG, "ioc_planes_polish: pair " + std::to_string(i) + " names no segment");
        if (group[i] > 1 && group[i] != IOC_SPLIT_NONE) return ioc_fail(c, IOC_ERR_ARG, "ioc_planes_polish: the group byte of pair " + std::to_string(i) + " is neither 0, 1 nor IOC_SPLIT_NONE");
        plane[size_t(i)] = plane_bytes;
        plane_bytes += int64_t(ds[size_t(seg_of_pair[i])].rlen) + 1;
    }
    if (plane_bytes > 0 && (!base || !slots)) return IOC_ERR_ARG;
    const GroupPolish gp{min_depth, out_seq, out_qual, cap, out_off, out_polish, out_gcols, out_gins};
    IOC_TRY(group_polish_ok(c, "ioc_planes_polish", gp, ds));
    out_off[0] = 0;
    if (n_segs == 0) return IOC_OK;
    IOC_CHK(c, hipSetDevice(c->device));
    DevBuf d_frames;
    IOC_TRY(ioc_alloc(c, d_frames, size_t(frame_bytes)));
    if (frame_bytes > 0) IOC_CHK(c, hipMemcpyAsync(d_frames.p, frames, size_t(frame_bytes), hipMemcpyHostToDevice, c->stream));
    AlnTally t;
    IOC_TRY(group_polish_device(c, gp, ds, static_cast<const uint8_t*>(d_frames.p), uint64_t(frame_bytes), size_t(n_pairs),
                                PlanesHost{seg_of_pair, group, plane.data(), base, slots}, PlanesDev{nullptr, nullptr, nullptr, nullptr, nullptr, uint64_t(plane_bytes)}, t));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   planes polish: %d group-segments, %lld rows, %d pairs, %lld plane bytes, %lld bytes called, k_plane_pile %.3f ms, k_pile_call %.3f ms\n",
                2 * n_segs, (long long)(2 * n_rows), n_pairs, (long long)(8 * plane_bytes), (long long)out_off[2 * n_segs], t.ms_plane_pile, t.ms_call);
    return IOC_OK;
}

// The split of segments whose sites and alleles the caller holds: both are uploaded, and the kernels run as behind
// ioc_align_pairs_split.
int ioc_alleles_split(ioc_ctx* c, int32_t n_segs, int32_t n_pairs, const int32_t* seg_of_pair, const ioc_pile_site* sites, const int64_t* site_off,
                      const uint8_t* alleles, const int64_t* allele_off, int32_t min_link, int32_t min_margin, int32_t rounds, int64_t* out_link,
                      int8_t* out_phase, uint8_t* out_group, int32_t* out_vote, ioc_split_seg* out_seg)
{
    if (!c || n_segs < 0 || n_pairs < 0 || !split_rule_ok(min_link, min_margin, rounds) || (n_segs > 0 && (!site_off || !out_seg)) ||
        (n_pairs > 0 && (!seg_of_pair || !allele_off || !out_group)))
        return IOC_ERR_ARG;
    if (n_segs > 0 && site_off[0] != 0) return ioc_fail(c, IOC_ERR_ARG, "ioc_alleles_split: site_off does not start at 0");
    for (int32_t g = 0; g < n_segs; ++g)
        if (site_off[g + 1] < site_off[g] || site_off[g + 1] - site_off[g] > INT32_MAX)
            return ioc_fail(c, IOC_ERR_ARG, "ioc_alleles_split: site_off descends or segment " + std::to_string(g) + " has more than 2^31 - 1 sites");
    if (n_pairs > 0 && allele_off[0] != 0) return ioc_fail(c, IOC_ERR_ARG, "ioc_alleles_split: allele_off does not start at 0");
    for (int32_t i = 0; i < n_pairs; ++i) {
        if (seg_of_pair[i] < 0 || seg_of_pair[i] >= n_segs) return ioc_fail(c, IOC_ERR_ARG, "ioc_alleles_split: pair " + std::to_string(i) + " names no segment");
        if (allele_off[i + 1] - allele_off[i] != site_off[seg_of_pair[i] + 1] - site_off[seg_of_pair[i]])
            return ioc_fail(c, IOC_ERR_ARG, "ioc_alleles_split: the alleles of pair " + std::to_string(i) + " are not one byte per site of its segment");
    }
    if ((n_segs > 0 && site_off[n_segs] > 0 && !sites) || (n_pairs > 0 && allele_off[n_pairs] > 0 && !alleles)) return IOC_ERR_ARG;
    if (n_segs == 0) return IOC_OK;
    AlnTally t;
    const SplitCall sp{min_link, min_margin, rounds, out_link, out_phase, out_group, out_vote, out_seg};
    IOC_TRY(split_device(c, sp, size_t(n_segs), size_t(n_pairs), seg_of_pair, site_off, allele_off, sites, alleles, false, t));
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   split: %d segments, %d pairs, %lld sites, %lld allele bytes, %s\n", n_segs, n_pairs, (long long)site_off[n_segs],
                (long long)(n_pairs ? allele_off[n_pairs] : 0), split_trace(t).c_str());
    return IOC_OK;
}

int ioc_pileup_call(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off, const ioc_pileup_col* cols,
                    const ioc_pileup_ins* ins, int32_t min_depth, char* out_seq, char* out_qual, int64_t cap, int64_t* out_off, ioc_polish_stats* out_stats)
{
    if (!c || n_segs < 0 || min_depth < 1 || !out_off || cap < 0 || (n_segs > 0 && (!rlen || !frame_off || !cols || !ins))) return IOC_ERR_ARG;
    return pileup_call_tables(c, n_segs, rlen, frames, frame_off, cols, nullptr, ins, min_depth, out_seq, out_qual, cap, out_off, out_stats);
}

int ioc_pileup_call_weighted(ioc_ctx* c, int32_t n_segs, const int32_t* rlen, const char* frames, const int64_t* frame_off,
                             const ioc_pileup_col* cols, const ioc_pileup_col* wcols, const ioc_pileup_ins* wins, int32_t min_depth, char* out_seq, char* out_qual, int64_t
                             cap, int64_t* out_off, ioc_polish_stats* out_stats)
{
    if (!c || n_segs < 0 || min_depth < 1 || !out_off || cap < 0 || (n_segs > 0 && (!rlen || !frame_off || !cols || !wcols || !wins))) return IOC_ERR_ARG;
    return pileup_call_tables(c, n_segs, rlen, frames, frame_off, cols, wcols, wins, min_depth, out_seq, out_qual, cap, out_off, out_stats);
}

int ioc_align_pairs_polish(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                           int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                           const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_depth, char* out_seq, char* out_qual, int64_t cap,
                           int64_t* out_off, ioc_polish_stats* out_polish, ioc_pileup_col* out_cols, ioc_pileup_ins* out_ins)
{
    return align_pairs_polish(c, AlnCall{n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}, out_stats, n_segs, segs,
                              seg_of_pair, min_depth, out_seq, out_qual, cap, out_off, out_polish, out_cols, out_ins, false, nullptr);
}

int ioc_align_pairs_polish_weighted(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t
                                    gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio, ioc_aln_stats* out_stats, int32_t n_segs,
                                    const ioc_polish_seg* segs, const int32_t* seg_of_pair, int32_t min_depth, char* out_seq, char* out_qual, int64_t
                                    cap, int64_t* out_off, ioc_polish_stats* out_polish, ioc_pileup_col* out_cols, ioc_pileup_col* out_wcols,
                                    ioc_pileup_ins* out_wins)
{
    return align_pairs_polish(c, AlnCall{n_pairs, pairs, k, match, mismatch, gap_extend, out_score, out_windows, out_ratio}, out_stats, n_segs, segs,
                              seg_of_pair, min_depth, out_seq, out_qual, cap, out_off, out_polish, out_cols, out_wins, true, out_wcols);
}

}  // extern "C"
