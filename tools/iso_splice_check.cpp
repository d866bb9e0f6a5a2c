// iso_splice_check.cpp — the lane logic of the kernels of isonclust2_amd/csrc/ioc_iso_splice.hip, restated lane by lane on the CPU and
// compared with the definition, ioc_host_isoform_splice (ioc_align.cpp):
//
//  * k_splice_plan: a lane per site; the wave walks the sites in turn, lane b decides site b against the hi of the last DONE site and
//    its answer is broadcast; the site records, the splice record and the plan of at most 32 ascending intervals;
//  * k_splice_call, count pass: a lane per row in chunks of IOC_PILE_CALL_CHUNK, a row asks splice_row what it is; sums over the wave
//    and over the workgroup's waves;
//  * k_splice_call, write pass: the inclusive scan over the 64 lanes of a wave in steps of 1, 2, .. 32, the waves' totals, the carry
//    down the chunks; the lane of a row lo notes where its window begins, and the whole workgroup copies the window's bytes, strided.
// Every output buffer is a block of exactly its size and every output byte and record word counts its writers: one each.  The
// inputs: random tables of 1 .. 700 rows, random plans of 0 .. 32 windows of 0 .. 3590 bytes, some overlapping, some not called, under
// random keys, at min_depth 1 .. 4.
//
// Host code only; meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/iso_splice_check tools/iso_splice_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/iso_splice_check
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
long long cases_seen = 0, done_seen = 0, overlap_seen = 0, bytes_seen = 0;

#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            if (++faults < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
        }                                                                   \
    } while (0)

constexpr uint32_t CHUNK = IOC_PILE_CALL_CHUNK, WAVES = CHUNK / 64u;

struct Case {
    int32_t rlen, min_depth;
    std::vector<ioc_pileup_col> cols;
    std::vector<ioc_pileup_ins> ins;
    std::string frame;
    uint64_t key;
    std::vector<ioc_insert_window> win;
    std::vector<int64_t> win_off;
    std::string wseq, wqual;
};

// k_splice_plan, one wave: what lane b holds of site b, the walk with its broadcasts, and what the lanes write
void plan_wave(const Case& c, std::vector<ioc_splice_site>& rec, std::vector<int>& rec_writers, ioc_splice_stats& ss, std::vector<IocSpliceIv>& plan, uint32_t& plan_n)
{
    const uint32_t ns = uint32_t(c.win.size());
    int32_t state[64], last_hi[64];
    uint32_t idx[64], n_done[64];
    for (uint32_t l = 0; l < 64u; ++l) state[l] = IOC_SPLICE_LACK, last_hi[l] = 0, idx[l] = 0, n_done[l] = 0;
    for (uint32_t b = 0; b < ns; ++b) {
        const int32_t s = splice_state(c.key, b, c.win[b], last_hi[b]);  // (lane b's; every lane's last_hi is the same)
        const int32_t hi = c.win[b].hi;                                   // (the two broadcasts from lane b)
        for (uint32_t l = 0; l < 64u; ++l) {
            if (l == b) state[l] = s, idx[l] = n_done[l];
            if (s == IOC_SPLICE_DONE) last_hi[l] = hi, ++n_done[l];
        }
    }
    ss = ioc_splice_stats{};
    std::vector<int> plan_writers(IOC_SPLICE_PLAN_MAX, 0);
    for (uint32_t l = 0; l < 64u; ++l) {
        const bool done = state[l] == IOC_SPLICE_DONE;
        const int32_t len = done ? int32_t(c.win_off[l + 1] - c.win_off[l]) : 0;
        ss.n_uncalled += state[l] == IOC_SPLICE_UNCALLED, ss.n_overlap += state[l] == IOC_SPLICE_OVERLAP;  // (the ballots and the wave sums)
        if (done) ss.rows_replaced += c.win[l].hi - c.win[l].lo, ss.spliced_bytes += len;
        if (l < ns) {
            rec[l].state = state[l], rec[l].len = len, rec[l].reserved = 0;
            if (!done) rec[l].at = -1, ++rec_writers[l];
        }
        if (done) {
            EXPECT(idx[l] < IOC_SPLICE_PLAN_MAX);
            if (idx[l] < IOC_SPLICE_PLAN_MAX) plan[idx[l]] = IocSpliceIv{c.win[l].lo, c.win[l].hi, len, int32_t(l), c.win_off[l]}, ++plan_writers[idx[l]];
        }
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
    const uint32_t ns = uint32_t(c.win.size()), rows = uint32_t(c.rlen) + 1u, nchunks = (rows + CHUNK - 1u) / CHUNK;
    const int64_t bound = int64_t(c.rlen) + int64_t(IOC_PILE_INS_SLOTS) * (int64_t(c.rlen) + 1) + (c.win_off[ns] - c.win_off[0]);
    // the definition
    const size_t room = size_t(bound);
    std::vector<char> want_seq(room), want_qual(room);
    std::vector<ioc_splice_site> want_rec(ns);
    ioc_polish_stats want_st{};
    ioc_splice_stats want_ss{};
    const int64_t want_len = ioc_host_isoform_splice(c.cols.data(), c.ins.data(), c.frame.data(), c.rlen, c.min_depth, c.key, c.win.data(), int32_t(ns), c.wseq.data(),
                                                     c.wqual.data(), c.win_off.data(), want_seq.data(), want_qual.data(), bound, &want_st, want_rec.data(), &want_ss);
    EXPECT(want_len >= 0 && want_len <= bound);
    if (want_len < 0) return;
    // below capacity: refused, nothing written
    if (bound > 0) {
        std::vector<char> s(size_t(bound), '?');
        EXPECT(ioc_host_isoform_splice(c.cols.data(), c.ins.data(), c.frame.data(), c.rlen, c.min_depth, c.key, c.win.data(), int32_t(ns), c.wseq.data(), c.wqual.data(),
                                       c.win_off.data(), s.data(), s.data(), bound - 1, nullptr, want_rec.data(), nullptr) == IOC_ERR_CAPACITY);
        EXPECT(std::all_of(s.begin(), s.end(), [](char ch) { return ch == '?'; }));
    }

    // k_splice_plan
    std::vector<ioc_splice_site> rec(ns, ioc_splice_site{-9, -9, -9, -9});
    std::vector<int> at_writers(ns, 0);
    std::vector<IocSpliceIv> plan(IOC_SPLICE_PLAN_MAX);
    uint32_t np = 0;
    ioc_splice_stats ss{};
    plan_wave(c, rec, at_writers, ss, plan, np);
    EXPECT(memcmp(&ss, &want_ss, sizeof ss) == 0);
    done_seen += ss.n_done, overlap_seen += ss.n_overlap;

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
                EXPECT(from < c.wseq.size() && at < out_bytes);
                if (from < c.wseq.size() && at < out_bytes) seq[at] = c.wseq[from], qual[at] = c.wqual[from], ++writers[at];
            }
    EXPECT(carry == out_bytes);
    EXPECT(std::all_of(writers.begin(), writers.end(), [](int w) { return w == 1; }));
    EXPECT(std::all_of(at_writers.begin(), at_writers.end(), [](int w) { return w == 1; }));
    EXPECT(out_bytes == 0 || (memcmp(seq.data(), want_seq.data(), out_bytes) == 0 && memcmp(qual.data(), want_qual.data(), out_bytes) == 0));
    EXPECT(ns == 0 || memcmp(rec.data(), want_rec.data(), ns * sizeof(ioc_splice_site)) == 0);
    bytes_seen += (long long)out_bytes;
}

Case random_case(std::mt19937_64& rng, int32_t rlen, uint32_t ns, const std::vector<int32_t>& lens)
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
    if (rlen < 2) ns = 0;
    std::vector<int32_t> lo(ns);
    for (auto& x : lo) x = 1 + int32_t(rng() % uint64_t(rlen - 1));
    std::sort(lo.begin(), lo.end());
    c.win_off.push_back(int64_t(rng() % 3u));  // (need not begin at 0)
    uint64_t key = 0;
    for (uint32_t b = 0; b < ns; ++b) {
        const int32_t hi = std::min<int32_t>(rlen, lo[b] + 1 + int32_t(rng() % uint64_t(std::max<int32_t>(2, 2 * rlen / int32_t(ns + 1)))));
        const int32_t tlen = rng() % 5u ? 7 : 0;
        c.win.push_back(ioc_insert_window{lo[b], hi, 0, tlen, 0, 0, 0, 0});
        c.win_off.push_back(c.win_off.back() + (tlen ? lens[rng() % lens.size()] : 0));
        key |= uint64_t("\1\1\1\0\3\2"[rng() % 6u]) << (2u * b);
    }
    c.key = key;
    for (int64_t x = 0; x < c.win_off.back(); ++x) c.wseq.push_back("ACGTN"[rng() % 5u]), c.wqual.push_back(char(33 + rng() % 41u));
    return c;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20261020);
    const std::vector<int32_t> small{0, 1, 8, 40}, big{0, 1, 8, 3590};
    for (int32_t rlen : {0, 1, 2, 5, 63, 64, 65, 255, 256, 257, 600, 700})
        for (int rep = 0; rep < 12; ++rep) run(random_case(rng, rlen, uint32_t(rng() % 9u), rep % 3 ? small : big));
    for (int rep = 0; rep < 30; ++rep) run(random_case(rng, 40 + int32_t(rng() % 600u), 32, rep % 2 ? small : big));
    {   // 32 sites back to back, all DONE, and the same under a key that carries every other one
        Case c = random_case(rng, 100, 0, small);
        for (int32_t b = 0; b < 32; ++b) c.win.push_back(ioc_insert_window{1 + 3 * b, 4 + 3 * b, 0, 5, 0, 0, 0, 0}), c.win_off.push_back(c.win_off.back() + b % 9);
        for (int64_t x = c.win_off.front(); x < c.win_off.back(); ++x) c.wseq.push_back('A'), c.wqual.push_back('I');
        c.key = 0x5555555555555555ull, run(c);
        c.key = 0x1111111111111111ull, run(c);
    }
    printf("%lld cases, %lld done sites, %lld overlapping, %lld bytes\n", cases_seen, done_seen, overlap_seen, bytes_seen);
    if (faults) return fprintf(stderr, "%d faults\n", faults), 1;
    printf("ok\n");
    return 0;
}
