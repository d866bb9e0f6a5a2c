// iso_splice_variants_check.cpp — the slot-aware plan kernel of isonclust2_amd/csrc/ioc_iso_splice.hip (k_splice_plan<true>), restated
// lane by lane on the CPU, feeding the call passes as tools/iso_splice_check.cpp restates them (k_splice_call is the same code for both
// plans), and compared with the definition, ioc_host_isoform_splice_variants (ioc_align.cpp):
//
//  * k_splice_plan<true>: a lane per kept site.  The lane loads its window record, its variant record and both ends of the slot its
//    key2 state takes — slot_off[2 (s0 + lane) + which] and the entry after it, which = 1 for IOC_INS_CARRY_B and 0 otherwise —; the
//    wave walks the sites in turn, lane b decides site b (splice_state_variants) against the hi of the last DONE site and its answer is
//    broadcast; the site records, the splice record and the plan of at most 32 ascending intervals whose `off` points into the slots;
//  * k_splice_call, count and write pass, over that plan: a lane per row in chunks of IOC_PILE_CALL_CHUNK, the wave scan, the waves'
//    totals, the carry down the chunks, the windows' bytes copied by the whole workgroup, strided.
// The segment stands behind others in its call: s0 sites and 2 s0 slots lie in front of it, so site_off and slot_off do not begin at 0.
// Every index into the packed records and offsets is checked against the arrays' sizes, every output byte and record word counts its
// writers: one each.  A fixed sweep: 0, 1, 31 and 32 sites; for every site every state 0 .. 3 of key2 there, at a site that splits and
// at one that does not, the other sites random; tables of 2 .. 600 rows; slots of 0 .. 3590 bytes.
//
// Host code only; meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/iso_splice_variants_check tools/iso_splice_variants_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/iso_splice_variants_check
//
// Exit status 0 and "ok" when everything agrees.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ioc_iso_splice.h"
#include "ioc_pile_call.h"
#include "isonclust2_hip.h"

namespace {

int faults = 0;
long long cases_seen = 0, done_seen[2] = {0, 0}, uncalled_b_seen = 0, overlap_seen = 0, bytes_seen = 0;

#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            if (++faults < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
        }                                                                   \
    } while (0)

constexpr uint32_t CHUNK = IOC_PILE_CALL_CHUNK, WAVES = CHUNK / 64u;

// one segment as the kernel sees it: the packed records and offsets of a whole call, of which sites s0 .. s0 + ns are this segment's
struct Case {
    int32_t rlen, min_depth;
    std::vector<ioc_pileup_col> cols;
    std::vector<ioc_pileup_ins> ins;
    std::string frame;
    uint64_t key;
    size_t s0, ns;
    std::vector<ioc_insert_window> win;   // s0 + ns records
    std::vector<ioc_window_variant> var;  // s0 + ns records
    std::vector<int64_t> slot_off;        // 2 (s0 + ns) + 1 entries
    std::string sseq, squal;
};

// k_splice_plan<true>, one wave
void plan_wave(const Case& c, std::vector<ioc_splice_site>& rec, std::vector<int>& rec_writers, ioc_splice_stats& ss, std::vector<IocSpliceIv>& plan, uint32_t& plan_n)
{
    const uint32_t ns = uint32_t(c.ns);
    const uint64_t n_sites = c.win.size();
    ioc_insert_window w[64];
    ioc_window_variant wv[64];
    long long off[64], end[64];
    bool mine[64];
    for (uint32_t l = 0; l < 64u; ++l) {  // the loads of a lane
        w[l] = ioc_insert_window{}, wv[l] = ioc_window_variant{}, off[l] = end[l] = 0;
        mine[l] = l < ns && uint64_t(c.s0) + l < n_sites;
        if (!mine[l]) continue;
        EXPECT(l < 32u);  // (the shift of the key)
        w[l] = c.win[c.s0 + l], wv[l] = c.var[c.s0 + l];
        const int32_t which = splice_variant_which(uint32_t(c.key >> (2u * l)) & 3u);
        const uint64_t slot = 2u * (uint64_t(c.s0) + l) + uint32_t(which > 0);
        EXPECT(slot + 1u < c.slot_off.size());
        if (slot + 1u < c.slot_off.size()) off[l] = c.slot_off[slot], end[l] = c.slot_off[slot + 1u];
    }
    int32_t state[64], last_hi[64];
    uint32_t idx[64], n_done[64];
    for (uint32_t l = 0; l < 64u; ++l) state[l] = IOC_SPLICE_LACK, last_hi[l] = 0, idx[l] = 0, n_done[l] = 0;
    for (uint32_t b = 0; b < ns; ++b) {
        const int32_t s = mine[b] ? splice_state_variants(c.key, b, w[b], wv[b], last_hi[b]) : IOC_SPLICE_LACK;  // (lane b's; every lane's last_hi is the same)
        const int32_t hi = w[b].hi;                                                                               // (the two broadcasts from lane b)
        for (uint32_t l = 0; l < 64u; ++l) {
            if (l == b) state[l] = s, idx[l] = n_done[l];
            if (s == IOC_SPLICE_DONE) last_hi[l] = hi, ++n_done[l];
        }
    }
    ss = ioc_splice_stats{};
    std::vector<int> plan_writers(IOC_SPLICE_PLAN_MAX, 0);
    for (uint32_t l = 0; l < 64u; ++l) {
        const bool done = state[l] == IOC_SPLICE_DONE;
        const int32_t len = done ? int32_t(end[l] - off[l]) : 0;
        ss.n_uncalled += state[l] == IOC_SPLICE_UNCALLED, ss.n_overlap += state[l] == IOC_SPLICE_OVERLAP;  // (the ballots and the wave sums)
        if (done) ss.rows_replaced += w[l].hi - w[l].lo, ss.spliced_bytes += len;
        if (l < ns) {
            rec[l].state = state[l], rec[l].len = len, rec[l].reserved = 0;
            if (!done) rec[l].at = -1, ++rec_writers[l];
        }
        if (done) {
            EXPECT(idx[l] < IOC_SPLICE_PLAN_MAX);
            if (idx[l] < IOC_SPLICE_PLAN_MAX) plan[idx[l]] = IocSpliceIv{w[l].lo, w[l].hi, len, int32_t(l), off[l]}, ++plan_writers[idx[l]];
            const uint32_t st = uint32_t(c.key >> (2u * l)) & 3u;
            ++done_seen[st == uint32_t(IOC_INS_CARRY_B)];
            EXPECT(st == uint32_t(IOC_INS_CARRY) || (st == uint32_t(IOC_INS_CARRY_B) && wv[l].split == 1));
        }
        if (l < ns && state[l] == IOC_SPLICE_UNCALLED && (uint32_t(c.key >> (2u * l)) & 3u) == uint32_t(IOC_INS_CARRY_B)) ++uncalled_b_seen;
    }
    plan_n = n_done[0], ss.n_done = int32_t(n_done[0]);
    for (uint32_t x = 0; x < IOC_SPLICE_PLAN_MAX; ++x) EXPECT(plan_writers[x] == (x < plan_n ? 1 : 0));
    for (uint32_t x = 0; x + 1 < plan_n; ++x) EXPECT(plan[x].hi <= plan[x + 1].lo);
}

PileRowCall decide(const Case& c, uint32_t p)
{
    const bool has_base = int32_t(p) < c.rlen;
    const unsigned long long d_ins = has_base ? pile_depth(c.cols[p]) : c.rlen > 0 ? pile_depth(c.cols[p - 1u]) : 0ull;
    return pile_call_row(c.cols[p], c.ins[p], d_ins, has_base, has_base ? uint8_t(c.frame[p]) : uint8_t(0), c.min_depth);
}

void wave_scan_incl(uint32_t* v)  // (the kernel's: steps of 1, 2, .. 32, every lane reads the value of the step before)
{
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        uint32_t up[64];
        for (uint32_t l = 0; l < 64u; ++l) up[l] = l >= d ? v[l - d] : 0u;
        for (uint32_t l = 0; l < 64u; ++l)
            if (l >= d) v[l] += up[l];
    }
}

void run(const Case& c)
{
    ++cases_seen;
    const uint32_t ns = uint32_t(c.ns), rows = uint32_t(c.rlen) + 1u, nchunks = (rows + CHUNK - 1u) / CHUNK;
    const int64_t* const my_off = c.slot_off.data() + 2 * c.s0;
    const int64_t bound = int64_t(c.rlen) + int64_t(IOC_PILE_INS_SLOTS) * (int64_t(c.rlen) + 1) + (my_off[2 * ns] - my_off[0]);
    // the definition, over the segment's own records and the whole packed bytes
    std::vector<char> want_seq(size_t(bound) + 1), want_qual(size_t(bound) + 1);
    std::vector<ioc_splice_site> want_rec(ns);
    ioc_polish_stats want_st{};
    ioc_splice_stats want_ss{};
    const int64_t want_len = ioc_host_isoform_splice_variants(c.cols.data(), c.ins.data(), c.frame.data(), c.rlen, c.min_depth, c.key, c.win.data() + c.s0,
                                                              c.var.data() + c.s0, int32_t(ns), c.sseq.data(), c.squal.data(), my_off, want_seq.data(), want_qual.data(),
                                                              bound, &want_st, want_rec.data(), &want_ss);
    EXPECT(want_len >= 0 && want_len <= bound);
    if (want_len < 0) return;
    if (bound > 0) {  // below capacity: refused, nothing written
        std::vector<char> s(size_t(bound), '?');
        std::vector<ioc_splice_site> untouched(ns, ioc_splice_site{-9, -9, -9, -9});
        EXPECT(ioc_host_isoform_splice_variants(c.cols.data(), c.ins.data(), c.frame.data(), c.rlen, c.min_depth, c.key, c.win.data() + c.s0, c.var.data() + c.s0,
                                                int32_t(ns), c.sseq.data(), c.squal.data(), my_off, s.data(), s.data(), bound - 1, nullptr, untouched.data(),
                                                nullptr) == IOC_ERR_CAPACITY);
        EXPECT(std::all_of(s.begin(), s.end(), [](char ch) { return ch == '?'; }));
        EXPECT(std::all_of(untouched.begin(), untouched.end(), [](const ioc_splice_site& r) { return r.state == -9 && r.at == -9; }));
    }

    // k_splice_plan<true>
    std::vector<ioc_splice_site> rec(ns, ioc_splice_site{-9, -9, -9, -9});
    std::vector<int> at_writers(ns, 0);
    std::vector<IocSpliceIv> plan(IOC_SPLICE_PLAN_MAX);
    uint32_t np = 0;
    ioc_splice_stats ss{};
    plan_wave(c, rec, at_writers, ss, plan, np);
    EXPECT(memcmp(&ss, &want_ss, sizeof ss) == 0);
    overlap_seen += ss.n_overlap;

    // k_splice_call, the count pass
    uint32_t part[WAVES][5] = {};
    for (uint32_t tid = 0; tid < CHUNK; ++tid) {
        uint32_t n = 0, k[4] = {0, 0, 0, 0};
        for (uint32_t ch = 0; ch < nchunks; ++ch) {
            const uint32_t p = ch * CHUNK + tid;
            if (p >= rows) break;
            const int32_t what = splice_row(plan.data(), np, int32_t(p));
            if (what == IOC_SPLICE_ROW_GONE) continue;
            if (what >= 0) {
                n += uint32_t(plan[what].len);
                continue;
            }
            const PileRowCall r = decide(c, p);
            n += r.n, k[0] += r.n_ins, k[1] += r.n_sub, k[2] += r.n_del, k[3] += r.n_low;
        }
        part[tid >> 6][0] += n;
        for (uint32_t y = 0; y < 4u; ++y) part[tid >> 6][1 + y] += k[y];
    }
    uint32_t t[5] = {0, 0, 0, 0, 0};
    for (uint32_t w = 0; w < WAVES; ++w)
        for (uint32_t y = 0; y < 5u; ++y) t[y] += part[w][y];
    EXPECT(int64_t(t[0]) == want_len && int32_t(t[0]) == want_st.out_len);
    EXPECT(int32_t(t[1]) == want_st.n_ins && int32_t(t[2]) == want_st.n_sub && int32_t(t[3]) == want_st.n_del && int32_t(t[4]) == want_st.n_low);

    // k_splice_call, the write pass, into blocks of exactly the counted size
    const size_t out_bytes = size_t(t[0]);
    std::vector<char> seq(out_bytes), qual(out_bytes);
    std::vector<int> writers(out_bytes, 0);
    std::vector<unsigned long long> win_at(IOC_SPLICE_PLAN_MAX, ~0ull);
    unsigned long long carry = 0;
    for (uint32_t ch = 0; ch < nchunks; ++ch) {
        uint32_t n[CHUNK], incl[CHUNK], tot[WAVES];
        int32_t what[CHUNK];
        PileRowCall r[CHUNK];
        for (uint32_t tid = 0; tid < CHUNK; ++tid) {
            const uint32_t p = ch * CHUNK + tid;
            what[tid] = p < rows ? splice_row(plan.data(), np, int32_t(p)) : IOC_SPLICE_ROW_GONE;
            r[tid] = PileRowCall{};
            if (p < rows && what[tid] == IOC_SPLICE_ROW_CALL) r[tid] = decide(c, p);
            n[tid] = incl[tid] = what[tid] >= 0 ? uint32_t(plan[what[tid]].len) : r[tid].n;
        }
        for (uint32_t w = 0; w < WAVES; ++w) wave_scan_incl(incl + 64u * w), tot[w] = incl[64u * w + 63u];
        uint32_t all = 0;
        for (uint32_t w = 0; w < WAVES; ++w) all += tot[w];
        for (uint32_t tid = 0; tid < CHUNK; ++tid) {
            uint32_t before = 0;
            for (uint32_t w = 0; w < (tid >> 6); ++w) before += tot[w];
            unsigned long long at = carry + before + (incl[tid] - n[tid]);
            if (what[tid] >= 0) {
                win_at[what[tid]] = at;
                const int32_t site = plan[what[tid]].site;
                EXPECT(site >= 0 && uint32_t(site) < ns);
                if (site >= 0 && uint32_t(site) < ns) rec[site].at = int32_t(at), ++at_writers[site];
            }
            for (uint32_t y = 0; y < r[tid].n; ++y, ++at) {
                EXPECT(at < out_bytes);
                if (at < out_bytes) seq[at] = char(r[tid].seq >> (8u * y)), qual[at] = char(r[tid].qual >> (8u * y)), ++writers[at];
            }
        }
        carry += all;
    }
    for (uint32_t i = 0; i < np; ++i)
        for (uint32_t tid = 0; tid < CHUNK; ++tid)
            for (uint32_t y = tid; y < uint32_t(plan[i].len); y += CHUNK) {
                const uint64_t from = uint64_t(plan[i].off) + y, at = win_at[i] + y;
                EXPECT(from < c.sseq.size() && at < out_bytes);
                if (from < c.sseq.size() && at < out_bytes) seq[at] = c.sseq[from], qual[at] = c.squal[from], ++writers[at];
            }
    EXPECT(carry == out_bytes);
    EXPECT(std::all_of(writers.begin(), writers.end(), [](int w) { return w == 1; }));
    EXPECT(std::all_of(at_writers.begin(), at_writers.end(), [](int w) { return w == 1; }));
    EXPECT(out_bytes == 0 || (memcmp(seq.data(), want_seq.data(), out_bytes) == 0 && memcmp(qual.data(), want_qual.data(), out_bytes) == 0));
    EXPECT(ns == 0 || memcmp(rec.data(), want_rec.data(), ns * sizeof(ioc_splice_site)) == 0);
    bytes_seen += (long long)out_bytes;
}

// a segment of ns sites behind s0 others; site `fix` (if < ns) has the state and the split flag given, the others are drawn
Case make_case(std::mt19937_64& rng, int32_t rlen, uint32_t ns, uint32_t s0, uint32_t fix, uint32_t fix_state, int32_t fix_split, const std::vector<int32_t>& lens)
{
    Case c;
    c.rlen = rlen, c.min_depth = 1 + int32_t(rng() % 4u);
    c.cols.assign(size_t(rlen) + 1, ioc_pileup_col{}), c.ins.assign(size_t(rlen) + 1, ioc_pileup_ins{});
    const uint32_t values[6] = {0, 1, 2, 3, 5, 0xFFFFFFFFu};
    for (auto& r : c.cols) r = ioc_pileup_col{values[rng() % 5u], values[rng() % 5u], values[rng() % 5u], values[rng() % 6u], values[rng() % 5u], values[rng() % 5u], 0, 0};
    for (auto& r : c.ins)
        for (uint32_t s = 0; s < uint32_t(IOC_PILE_INS_SLOTS) && rng() % 2u; ++s)
            for (uint32_t ch = 0; ch < 5u; ++ch) r.slot[s][ch] = values[rng() % 5u];
    for (int32_t p = 0; p < rlen; ++p) c.frame.push_back("ACGTN"[rng() % 5u]);
    c.s0 = s0, c.ns = ns;
    c.slot_off.push_back(0);
    for (uint32_t b = 0; b < s0; ++b) {  // the sites of the segments in front: records nobody of this wave reads, bytes nobody copies
        c.win.push_back(ioc_insert_window{1, 2, 0, 3, 0, 0, 0, 0}), c.var.push_back(ioc_window_variant{1, 0, 3, 1, 1, 0, 1, 0});
        c.slot_off.push_back(c.slot_off.back() + 5), c.slot_off.push_back(c.slot_off.back() + 3);
    }
    std::vector<int32_t> lo(ns);
    for (auto& x : lo) x = 1 + int32_t(rng() % uint64_t(rlen - 1));
    std::sort(lo.begin(), lo.end());
    uint64_t key = 0;
    for (uint32_t b = 0; b < ns; ++b) {
        const int32_t hi = std::min<int32_t>(rlen, lo[b] + 1 + int32_t(rng() % uint64_t(std::max<int32_t>(2, 2 * rlen / int32_t(ns + 1)))));
        const int32_t tlen = rng() % 5u ? 7 : 0;
        const int32_t split = b == fix ? fix_split : int32_t(rng() % 2u);
        const int32_t tlen_b = split ? (rng() % 6u ? 6 : 0) : (rng() % 4u ? 0 : 9);  // (a stray tlen_b where nothing split is not read)
        c.win.push_back(ioc_insert_window{lo[b], hi, 0, tlen, 0, 0, 0, 0});
        c.var.push_back(ioc_window_variant{split, split ? 0 : -1, tlen_b, 0, 0, 0, 0, 0});
        c.slot_off.push_back(c.slot_off.back() + (tlen ? lens[rng() % lens.size()] : 0));
        c.slot_off.push_back(c.slot_off.back() + (split && tlen_b ? lens[rng() % lens.size()] : 0));
        key |= uint64_t(b == fix ? fix_state : uint32_t("\1\1\2\2\0\3"[rng() % 6u])) << (2u * b);
    }
    c.key = key | (ns < 32u ? ~0ull << (2u * ns) : 0ull);  // (bits behind the segment's sites mean nothing)
    for (int64_t x = 0; x < c.slot_off.back(); ++x) c.sseq.push_back("ACGTN"[rng() % 5u]), c.squal.push_back(char(33 + rng() % 41u));
    return c;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20261021);
    const std::vector<int32_t> small{0, 1, 8, 40}, big{0, 1, 8, 3590};
    const int32_t rlens[] = {2, 5, 63, 64, 65, 255, 256, 257, 600};
    uint32_t turn = 0;
    for (uint32_t ns : {0u, 1u, 31u, 32u})
        for (uint32_t fix = 0; fix < std::max(ns, 1u); ++fix)
            for (uint32_t state = 0; state < 4u; ++state)
                for (int32_t split = 0; split < 2; ++split, ++turn) {
                    const int32_t rlen = ns >= 31u ? 40 + int32_t(rng() % 560u) : rlens[turn % 9u];
                    run(make_case(rng, rlen, ns, turn % 3u ? 3u + turn % 5u : 0u, fix, state, split, turn % 4u ? small : big));
                }
    {   // 32 sites back to back, all split, alternating A and B: all DONE, the slot indices run to 2 (s0 + 31) + 1
        Case c = make_case(rng, 100, 0, 4, 0, 0, 0, small);
        c.ns = 32;
        for (int32_t b = 0; b < 32; ++b) {
            c.win.push_back(ioc_insert_window{1 + 3 * b, 4 + 3 * b, 0, 5, 0, 0, 0, 0}), c.var.push_back(ioc_window_variant{1, 0, 5, 0, 0, 0, 0, 0});
            c.slot_off.push_back(c.slot_off.back() + b % 9), c.slot_off.push_back(c.slot_off.back() + (b + 4) % 7);
        }
        while (int64_t(c.sseq.size()) < c.slot_off.back()) c.sseq.push_back("ACGT"[c.sseq.size() % 4u]), c.squal.push_back(char(40 + c.squal.size() % 30u));
        c.key = 0x6666666666666666ull, run(c);  // B A B A ..
        c.key = 0x9999999999999999ull, run(c);  // A B A B ..
    }
    printf("%lld cases, %lld sites done with A, %lld with B, %lld B uncalled, %lld overlapping, %lld bytes\n", cases_seen, done_seen[0], done_seen[1], uncalled_b_seen,
           overlap_seen, bytes_seen);
    EXPECT(done_seen[0] > 0 && done_seen[1] > 0 && uncalled_b_seen > 0 && overlap_seen > 0);
    if (faults) return fprintf(stderr, "%d faults\n", faults), 1;
    printf("ok\n");
    return 0;
}
