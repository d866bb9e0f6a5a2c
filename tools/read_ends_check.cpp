// read_ends_check.cpp — the word and wave logic of the kernels of isonclust2_amd/csrc/ioc_read_ends.hip, restated lane by lane on
// the CPU and compared with the definition, ioc_host_reads_ends (ioc_align.cpp):
//
//  * k_end_hist, k_end_rows: the two histograms by adds, Ws and We from two prefix sums over 64 lanes each, the 64 rows and a halo
//    of 32 either side (window_sums), the row test, the start-row and stop-row words, the row table;
//  * k_end_list: the k-th start and the k-th end of the runs of either plane, a run going on across a word by its neighbour's edge
//    bit and across a batch of 64 words by a carried bit and a word read ahead; the first max_sites kept;
//  * k_end_class: lanes 0 .. 31 the start sites and lanes 32 .. 63 the stop sites, (distance, site) as one word and its minimum
//    over each half by the xor steps 16, 8, 4, 2, 1;
//  * k_end_count: n_reads and n_over over the members 64 at a time, and the peak as the largest (count, rlen - row) word over the
//    site's rows 64 at a time;
//  * k_end_support, k_end_variants, k_ends_record: counts over the members with UNSIGNED compares of one 64-bit key, unplaced reads
//    left out by their flag; every variant slot counts its writers: one each.
// Every buffer is a block of exactly its size.  The inputs: segments of 0, 1, 2, 63, 64, 65, 127, 128, 129, 600, 4200 and 9000 rows
// with 0 to 130 reads, ends in a few clusters with jitter so that sites form, windows across 63 | 64 and 4095 | 4096, reads that
// take no part, 35 sites under max_sites 32, pre_group of -1 and 2^31 - 1 — under rules of slack 0, 1, 10 and 32.
//
// Host code only; meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/read_ends_check tools/read_ends_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/read_ends_check
//
// Exit status 0 and "ok" when everything agrees.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "ioc_read_ends.h"
#include "isonclust2_hip.h"

namespace {

typedef unsigned long long u64;
int faults = 0;
long long sites_seen = 0, cut_lists = 0, batches_crossed = 0, windows_seen = 0, ties_seen = 0, variants_seen = 0, unplaced_seen = 0, empty_peaks = 0;

#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            if (++faults < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
        }                                                                   \
    } while (0)

struct Segment {
    int32_t rlen = 0;
    std::vector<ioc_read_extent> ext;
    std::vector<int32_t> pre;
    bool with_pre = true;
};

uint32_t scan_incl(const uint32_t* v, uint32_t lane)
{
    uint32_t s = 0;
    for (uint32_t l = 0; l <= lane; ++l) s += v[l];
    return s;
}

// window_sums: W(p0 + lane) for the 64 lanes from the lanes' own counts and their halo
void window_sums(const uint32_t* own, const uint32_t* halo, uint32_t slack, uint32_t* win)
{
    uint32_t sV[64], sH[64];
    for (uint32_t l = 0; l < 64u; ++l) sV[l] = scan_incl(own, l), sH[l] = scan_incl(halo, l);
    const uint32_t left = sH[31], mid = sV[63];
    auto prefix = [&](int idx) -> uint32_t {
        const uint32_t fromH = sH[uint32_t(idx < 32 ? idx : idx - 64) & 63u], fromV = sV[uint32_t(idx - 32) & 63u];
        return idx < 0 ? 0u : idx < 32 ? fromH : idx < 96 ? left + fromV : mid + fromH;
    };
    for (uint32_t l = 0; l < 64u; ++l) win[l] = prefix(int(32u + l + slack)) - prefix(int(32u + l) - int(slack) - 1);
    ++windows_seen;
}

void check_segment(const Segment& s, const EndsRule& rule)
{
    const uint32_t n = uint32_t(s.ext.size()), rlen = uint32_t(s.rlen), W = rlen / 64u + 1u, rows = rlen + 1u;
    const uint32_t most = uint32_t(ends_sites_most(s.rlen, rule.max_sites)), vmost = uint32_t(ends_variants_most(n, rule.max_variants));
    // the definition
    std::vector<ioc_end_row> want_rows(rows);
    std::vector<ioc_end_site> want_sites[2] = {std::vector<ioc_end_site>(most), std::vector<ioc_end_site>(most)};
    std::vector<ioc_end_variant> want_vars(vmost);
    std::vector<ioc_read_ends> want_reads(n);
    ioc_ends_seg want_seg{};
    ioc_end_variant none{};
    EXPECT(ioc_host_reads_ends(s.ext.data(), s.with_pre ? s.pre.data() : nullptr, int32_t(n), s.rlen, rule.slack, rule.min_over, rule.min_depth, rule.min_alt,
                               rule.min_pct, rule.max_sites, rule.max_variants, want_rows.data(), want_sites[0].data(), want_sites[1].data(),
                               vmost ? want_vars.data() : &none, want_reads.data(), &want_seg) == IOC_OK);
    auto pre_of = [&](uint32_t i) { return s.with_pre ? s.pre.at(i) : 0; };

    // k_end_hist
    std::vector<uint32_t> hist[2] = {std::vector<uint32_t>(rows, 0), std::vector<uint32_t>(rows, 0)};
    uint32_t N = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (ends_extent_ok(s.ext[i], s.rlen) && ends_takes_part(s.ext[i])) ++hist[0].at(size_t(s.ext[i].first_row)), ++hist[1].at(size_t(s.ext[i].end_row)), ++N;
    EXPECT(int32_t(N) == want_seg.n_reads);

    // k_end_rows
    std::vector<u64> bits[2] = {std::vector<u64>(W, 0), std::vector<u64>(W, 0)};
    for (uint32_t t = 0; t < W; ++t) {
        const long long p0 = (long long)t * 64;
        for (int kind = 0; kind < 2; ++kind) {
            auto at = [&](long long q) -> uint32_t { return q >= 0 && q <= (long long)rlen ? hist[kind].at(size_t(q)) : 0u; };
            uint32_t own[64], halo[64], win[64];
            for (uint32_t l = 0; l < 64u; ++l) own[l] = at(p0 + l), halo[l] = at(l < 32u ? p0 - 32 + l : p0 + 32 + l);
            window_sums(own, halo, uint32_t(rule.slack), win);
            for (uint32_t l = 0; l < 64u; ++l) {
                const long long p = p0 + l;
                if (p > (long long)rlen) continue;
                if (rule.row(N, win[l])) bits[kind].at(t) |= 1ull << l;
                EXPECT(win[l] == (kind ? want_rows.at(size_t(p)).w_stops : want_rows.at(size_t(p)).w_starts));
                EXPECT(own[l] == (kind ? want_rows.at(size_t(p)).stops : want_rows.at(size_t(p)).starts));
            }
        }
    }

    // k_end_list
    std::vector<ioc_end_site> sites[2] = {std::vector<ioc_end_site>(most, ioc_end_site{}), std::vector<ioc_end_site>(most, ioc_end_site{})};
    uint32_t kept[2] = {0, 0};
    for (int kind = 0; kind < 2; ++kind) {
        auto load = [&](uint32_t i) -> u64 { return i < W ? bits[kind].at(i) : 0ull; };
        std::vector<int> first_writers(most, 0), end_writers(most, 0);
        uint32_t base_s = 0, base_e = 0;
        u64 top = 0;
        for (uint32_t b0 = 0; b0 < W; b0 += 64u) {
            u64 w[64];
            uint32_t ns[64], ne[64];
            u64 st[64], en[64];
            for (uint32_t l = 0; l < 64u; ++l) w[l] = load(b0 + l);
            for (uint32_t l = 0; l < 64u; ++l) {
                const uint32_t left = uint32_t(l ? w[l - 1] >> 63 : top), right = uint32_t((l < 63u ? w[l + 1] : load(b0 + 64u)) & 1ull);
                st[l] = run_starts(w[l], left), en[l] = run_ends(w[l], right);
                ns[l] = uint32_t(__builtin_popcountll(st[l])), ne[l] = uint32_t(__builtin_popcountll(en[l]));
                if (l == 0 && b0 && top && (w[0] & 1ull)) ++batches_crossed;
            }
            for (uint32_t l = 0; l < 64u; ++l) {
                const uint32_t is = scan_incl(ns, l), ie = scan_incl(ne, l), row = (b0 + l) * 64u;
                for (uint32_t k = base_s + is - ns[l]; st[l] && k < most; ++k, st[l] &= st[l] - 1ull)
                    sites[kind].at(k).first = int32_t(row + uint32_t(__builtin_ctzll(st[l]))), ++first_writers.at(k);
                for (uint32_t k = base_e + ie - ne[l]; en[l] && k < most; ++k, en[l] &= en[l] - 1ull)
                    sites[kind].at(k).end = int32_t(row + uint32_t(__builtin_ctzll(en[l])) + 1u), ++end_writers.at(k);
            }
            base_s += scan_incl(ns, 63), base_e += scan_incl(ne, 63);
            top = w[63] >> 63;
        }
        EXPECT(base_s == base_e);
        kept[kind] = std::min(base_s, most);
        EXPECT(int32_t(kept[kind]) == (kind ? want_seg.n_stops : want_seg.n_starts) && int32_t(base_s) == (kind ? want_seg.n_stops_found : want_seg.n_starts_found));
        for (uint32_t k = 0; k < most; ++k) EXPECT(first_writers[k] == (k < kept[kind] ? 1 : 0) && end_writers[k] == (k < kept[kind] ? 1 : 0));
        sites_seen += kept[kind], cut_lists += base_s > most;
    }

    // k_end_class
    std::vector<ioc_read_ends> reads(n);
    std::vector<u64> key(n, 0);
    std::vector<uint8_t> placed(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const ioc_read_extent e = s.ext[i];
        const bool part = ends_extent_ok(e, s.rlen) && ends_takes_part(e);
        uint32_t word[64];
        for (uint32_t l = 0; l < 64u; ++l) {
            const uint32_t kind = l >> 5, b = l & 31u;
            word[l] = ENDS_FAR;
            if (part && b < std::min(kept[kind], uint32_t(IOC_ENDS_MAX)))
                word[l] = ends_near_word(ends_distance(sites[kind].at(b).first, sites[kind].at(b).end, kind ? e.end_row : e.first_row), b, rule.slack);
        }
        uint32_t at_best[2] = {0, 0};
        for (uint32_t l = 0; l < 64u; ++l) at_best[l >> 5] += word[l] != ENDS_FAR && (word[l] >> 8) == (*std::min_element(word + (l & 32u), word + (l & 32u) + 32) >> 8);
        ties_seen += (at_best[0] > 1) + (at_best[1] > 1);
        for (uint32_t d = 16; d >= 1u; d >>= 1) {
            uint32_t next[64];
            for (uint32_t l = 0; l < 64u; ++l) next[l] = std::min(word[l], word[l ^ d]);
            memcpy(word, next, sizeof word);
        }
        const int32_t start = ends_near_site(word[0]), stop = ends_near_site(word[32]);
        reads[i] = ioc_read_ends{start, stop, -1, 0};
        placed[i] = ends_placed(pre_of(i), start, stop);
        key[i] = placed[i] ? ends_key(pre_of(i), start, stop) : 0ull;
        unplaced_seen += !placed[i];
    }

    // k_end_count
    for (int kind = 0; kind < 2; ++kind)
        for (uint32_t k = 0; k < kept[kind]; ++k) {
            uint32_t n_reads = 0, n_over = 0;
            for (uint32_t m0 = 0; m0 < n; m0 += 64u)
                for (uint32_t l = 0; l < 64u && m0 + l < n; ++l) {
                    const uint32_t i = m0 + l;
                    const bool mine = (kind ? reads[i].stop_site : reads[i].start_site) == int32_t(k);
                    n_reads += mine, n_over += mine && (kind ? s.ext[i].tail : s.ext[i].head) >= rule.min_over;
                }
            ioc_end_site& r = sites[kind].at(k);
            u64 peak = 0;
            for (long long p0 = r.first; p0 < r.end; p0 += 64)
                for (uint32_t l = 0; l < 64u; ++l) {
                    const long long p = p0 + l;
                    if (p < r.end && p <= (long long)rlen) peak = std::max(peak, ends_peak_word(hist[kind].at(size_t(p)), rlen, uint32_t(p)));
                }
            r.n_reads = n_reads, r.n_over = n_over, r.peak_row = ends_peak_row(peak, rlen), r.peak_reads = ends_peak_count(peak), r.kind = kind, r.reserved = 0;
            empty_peaks += r.peak_reads == 0;
            EXPECT(r.peak_row >= r.first && r.peak_row < r.end);
            EXPECT(memcmp(&r, &want_sites[kind].at(k), sizeof r) == 0);
        }

    // k_end_support, k_end_variants, k_ends_record
    const uint32_t FIRST = 0x80000000u, COUNT = 0x7FFFFFFFu;
    std::vector<uint32_t> same(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t cnt = 0, earlier = 0;
        if (placed[i])
            for (uint32_t x = 0; x < n; ++x) {
                const bool hit = placed[x] && key[x] == key[i];
                cnt += hit, earlier += hit && x < i;
            }
        same[i] = cnt ? (cnt & COUNT) | (earlier == 0u ? FIRST : 0u) : 0u;
    }
    std::vector<ioc_end_variant> vars(vmost, ioc_end_variant{});
    std::vector<int> var_writers(vmost, 0);
    uint32_t found = 0, n_placed = 0;
    for (uint32_t i = 0; i < n; ++i) {
        n_placed += placed[i];
        const bool lead = placed[i] && (same[i] & FIRST) && (same[i] & COUNT) >= uint32_t(rule.min_alt);
        found += lead;
        if ((same[i] & COUNT) < uint32_t(rule.min_alt)) continue;
        uint32_t rank = 0;
        for (uint32_t x = 0; x < n; ++x) rank += placed[x] && (same[x] & FIRST) && (same[x] & COUNT) >= uint32_t(rule.min_alt) && key[x] < key[i];
        if (rank >= vmost) continue;
        reads[i].variant = int32_t(rank);
        if (same[i] & FIRST)
            vars.at(rank) = ioc_end_variant{int32_t(uint32_t(key[i] >> 32)), int32_t((key[i] >> 8) & 0xFFull), int32_t(key[i] & 0xFFull), same[i] & COUNT}, ++var_writers.at(rank);
    }
    const uint32_t n_vars = std::min(found, vmost);
    variants_seen += n_vars, cut_lists += found > vmost;
    EXPECT(int32_t(n_vars) == want_seg.n_variants && int32_t(found) == want_seg.n_variants_found && int32_t(n_placed) == want_seg.n_placed);
    for (uint32_t k = 0; k < vmost; ++k) EXPECT(var_writers[k] == (k < n_vars ? 1 : 0));
    for (uint32_t k = 0; k < n_vars && k < vmost; ++k) EXPECT(memcmp(&vars[k], &want_vars[k], sizeof vars[k]) == 0);
    for (uint32_t i = 0; i < n; ++i) EXPECT(memcmp(&reads[i], &want_reads[i], sizeof reads[i]) == 0);
}

Segment make_segment(std::mt19937& rng, int32_t rlen, uint32_t n, bool many_sites)
{
    Segment s;
    s.rlen = rlen;
    auto clip = [&](long long v) { return int32_t(std::min<long long>(std::max<long long>(v, 0), rlen)); };
    int32_t starts[3], stops[3];
    for (int x = 0; x < 3; ++x) starts[x] = int32_t(rng() % uint32_t(rlen + 1)), stops[x] = int32_t(rng() % uint32_t(rlen + 1));
    if (rlen >= 129) starts[0] = 63, stops[0] = 64;
    if (rlen >= 4200) starts[1] = 4095, stops[1] = 4097;
    const int32_t pres[] = {-1, 0, 0, 1, 1, 2, INT32_MAX};
    for (uint32_t i = 0; i < n; ++i) {
        int32_t a, z;
        if (many_sites) {
            a = clip(50ll * (i % 35u) + 25), z = rlen;
        } else {
            a = rng() % 5u ? clip(starts[rng() % 3u] + int(rng() % 5u) - 2) : clip(rng() % uint32_t(rlen + 1));
            z = rng() % 5u ? clip(stops[rng() % 3u] + int(rng() % 5u) - 2) : clip(rng() % uint32_t(rlen + 1));
            if (a > z) std::swap(a, z);
        }
        const int32_t beyond[] = {0, 19, 20, 400};
        s.ext.push_back(ioc_read_extent{a, z, beyond[rng() % 4u], beyond[rng() % 4u]});
        s.pre.push_back(pres[rng() % 7u]);
    }
    return s;
}

}  // namespace

int main()
{
    std::mt19937 rng(12345);
    const int32_t lens[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 600, 4200, 9000};
    const uint32_t counts[] = {0, 1, 3, 6, 64, 65, 130};
    const EndsRule rules[] = {{10, 20, 3, 3, 10, 32, 64}, {0, 20, 1, 1, 1, 32, 64}, {1, 1, 2, 2, 5, 32, 2}, {32, 20, 1, 2, 100, 1, 64}, {10, 20, 1, 1, 1, 3, 1}};
    for (int32_t rlen : lens)
        for (uint32_t n : counts)
            for (const EndsRule& rule : rules) {
                Segment s = make_segment(rng, rlen, n, false);
                check_segment(s, rule);
                s.with_pre = false;
                check_segment(s, rule);
            }
    const Segment many = make_segment(rng, 2000, 130, true);  // 35 start sites of three or four reads each
    check_segment(many, EndsRule{10, 20, 3, 3, 2, 32, 64});
    check_segment(many, EndsRule{10, 20, 3, 3, 2, 1, 64});
    Segment dense = make_segment(rng, 9000, 130, false);  // every row a start row and a stop row: runs across words and batches
    check_segment(dense, EndsRule{32, 20, 1, 1, 1, 32, 64});
    for (uint32_t i = 0; i < 130u; ++i) dense.ext[i] = ioc_read_extent{int32_t(4090 + i % 12u), int32_t(8180 + i % 24u), 0, 0};
    check_segment(dense, EndsRule{2, 20, 1, 1, 1, 32, 64});
    printf("%s: %lld sites, %lld cut lists, %lld runs across a batch, %lld windows, %lld ties, %lld variants, %lld unplaced reads, %lld sites whose peak has no read, %d faults\n",
           faults ? "FAILED" : "ok", sites_seen, cut_lists, batches_crossed, windows_seen, ties_seen, variants_seen, unplaced_seen, empty_peaks, faults);
    return faults ? 1 : 0;
}
