// site_split_check.cpp — the host-callable logic behind the split of a cluster's reads by linked sites, driven on the CPU as the
// kernels of isonclust2_amd/csrc/ioc_site_split.hip drive it and compared, segment by segment, with the definition
// ioc_host_alleles_split (ioc_align.cpp):
//
//  * the member lists: the counting sort of seg_of_pair, the tiles (tile_seg, word_off), the planes' offsets (bit_off);
//  * k_allele_bits lane by lane: the tile of 64 reads x 64 sites written with lane = site and read with lane = read, one ballot
//    word per site and plane, stored word-major at bit_off[g] + w * n_sites + t;
//  * k_site_link, k_split_seed and k_split_phase0: d from split_d_word over the words, the first maximum through the butterfly
//    with "the lower index wins", the first phases; k_split_vote; k_group_bits and k_split_rephase per round; k_split_record.
// Every buffer has exactly the size the library gives it, so that a store or load outside it is the sanitizer's to find, and every
// word of the planes must be written exactly once.  Random matrices with reads per segment around 64 and 128, sites around 64,
// segments without reads and without sites, seg_of_pair interleaved.
//
// Host code only; meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/site_split_check tools/site_split_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/site_split_check
//
// Exit status 0 and "ok" when everything agrees.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "ioc_site_split.h"
#include "isonclust2_hip.h"

namespace {

using u64 = unsigned long long;
constexpr uint32_t TILE_ROW = 68;

struct Call {
    uint32_t n_segs = 0, n_pairs = 0;
    std::vector<int32_t> seg_of_pair;
    std::vector<ioc_pile_site> sites;
    std::vector<int64_t> site_off, allele_off;
    std::vector<uint8_t> alleles;
};

struct Out {
    std::vector<int64_t> link;
    std::vector<int8_t> phase;
    std::vector<uint8_t> group;
    std::vector<int32_t> vote;
    std::vector<ioc_split_seg> rec;
};

// the launch sequence of ioc_align_sinks.cpp's split_device over the call, every kernel as loops over its lanes
int drive(const Call& c, int32_t min_link, int32_t min_margin, int32_t rounds, Out& o)
{
    int faults = 0;
    const size_t n = c.n_segs, np = c.n_pairs, S = size_t(c.site_off[n]), bytes = c.alleles.size();
    std::vector<uint32_t> mem_off(n + 1, 0), members(np), word_off(n + 1, 0);
    std::vector<int64_t> bit_off(n + 1, 0);
    for (size_t i = 0; i < np; ++i) ++mem_off[size_t(c.seg_of_pair[i]) + 1];
    for (size_t g = 0; g < n; ++g) mem_off[g + 1] += mem_off[g];
    {
        std::vector<uint32_t> next(mem_off.begin(), mem_off.end() - 1);
        for (size_t i = 0; i < np; ++i) members[next[size_t(c.seg_of_pair[i])]++] = uint32_t(i);
    }
    for (size_t g = 0; g < n; ++g) {
        const uint32_t words = (mem_off[g + 1] - mem_off[g] + 63u) / 64u;
        word_off[g + 1] = word_off[g] + words;
        bit_off[g + 1] = bit_off[g] + int64_t(words) * (c.site_off[g + 1] - c.site_off[g]);
    }
    const size_t T = word_off[n], P = size_t(bit_off[n]);
    std::vector<int32_t> tile_seg(T), seg_of_site(S);
    for (size_t g = 0; g < n; ++g) {
        for (size_t x = word_off[g]; x < word_off[g + 1]; ++x) tile_seg[x] = int32_t(g);
        for (int64_t s = c.site_off[g]; s < c.site_off[g + 1]; ++s) seg_of_site[size_t(s)] = int32_t(g);
    }
    std::vector<int32_t> mark_minor(S), mark_major(S);
    for (size_t s = 0; s < S; ++s) mark_minor[s] = c.sites[s].minor, mark_major[s] = c.sites[s].major;
    std::vector<u64> bm(P, 0), bM(P, 0), g1(T, 0), g0(T, 0);
    std::vector<uint8_t> written(P, 0);
    o.link.assign(S, -7), o.phase.assign(S, -7), o.group.assign(np, 0xA5), o.vote.assign(np, -7), o.rec.assign(n, ioc_split_seg{});
    std::vector<int32_t> seed(n, -7);

    // k_allele_bits: one wave per tile
    for (size_t x = 0; x < T; ++x) {
        const uint32_t g = uint32_t(tile_seg[x]), w = uint32_t(x) - word_off[g], m0 = mem_off[g], nr = mem_off[g + 1] - m0;
        const uint64_t s0 = uint64_t(c.site_off[g]), ns = uint64_t(c.site_off[g + 1]) - s0, bo = uint64_t(bit_off[g]);
        u64 a0[64];
        bool valid[64];
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t r = w * 64u + lane;
            valid[lane] = r < nr;
            a0[lane] = valid[lane] ? u64(c.allele_off[members[m0 + r]]) : 0ull;
        }
        const uint32_t in_tile = nr - w * 64u < 64u ? nr - w * 64u : 64u;
        std::vector<uint8_t> tile(64 * TILE_ROW, 0xEE);
        // (the steps of 64 sites are shared out over gridDim.y workgroups of the tile: every step has one of them, whatever gridDim.y)
        const uint32_t grid_y = 1u + uint32_t(x % 3u);
        for (uint32_t by = 0; by < grid_y; ++by)
        for (uint64_t t0 = uint64_t(by) * 64u; t0 < ns; t0 += uint64_t(grid_y) * 64u) {
            std::fill(tile.begin(), tile.end(), uint8_t(0xEE));  // (another workgroup's LDS: nothing carries over)
            for (uint32_t k = 0; k < in_tile; ++k)
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const uint64_t t = t0 + lane;
                    uint8_t b = 0;
                    if (t < ns && a0[k] + t < bytes) b = c.alleles[a0[k] + t];
                    tile[k * TILE_ROW + lane] = b;
                }
            for (uint32_t s = 0; s < 64; ++s) {
                const uint64_t ts = t0 + s;
                const int32_t mi = ts < ns ? mark_minor[s0 + ts] : -1, ma = ts < ns ? mark_major[s0 + ts] : -1;
                u64 b_minor = 0, b_major = 0;
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const int32_t mk = valid[lane] ? split_mark(tile[lane * TILE_ROW + s], mi, ma) : 0;
                    if (mk > 0) b_minor |= 1ull << lane;
                    if (mk < 0) b_major |= 1ull << lane;
                }
                if (ts < ns) {  // (lane s of the wave stores the word of site t0 + s)
                    const uint64_t at = bo + uint64_t(w) * ns + ts;
                    if (at >= P) return printf("k_allele_bits: word %llu outside the planes\n", (u64)at), 1;
                    bm[at] = b_minor, bM[at] = b_major;
                    faults += written[at]++ != 0;
                }
            }
        }
    }
    for (size_t at = 0; at < P; ++at) faults += written[at] != 1;
    if (faults) return printf("k_allele_bits: a word of the planes without exactly one writer\n"), faults;

    auto d_with_site = [&](const u64* a_minor, const u64* a_major, uint64_t stride, uint64_t bo, uint64_t ns, uint32_t W, uint64_t t) {
        int32_t d = 0;
        for (uint32_t w = 0; w < W; ++w) d += split_d_word(a_minor[w * stride], a_major[w * stride], bm[bo + w * ns + t], bM[bo + w * ns + t]);
        return d;
    };
    // k_site_link: one wave per site
    for (size_t Sx = 0; Sx < S; ++Sx) {
        const uint32_t g = uint32_t(seg_of_site[Sx]), W = word_off[g + 1] - word_off[g];
        const uint64_t s0 = uint64_t(c.site_off[g]), ns = uint64_t(c.site_off[g + 1]) - s0, s = Sx - s0, bo = uint64_t(bit_off[g]);
        u64 acc = 0;
        for (uint32_t lane = 0; lane < 64; ++lane)
            for (uint64_t t = lane; t < ns; t += 64u) {
                const int32_t d = d_with_site(bm.data() + bo + s, bM.data() + bo + s, ns, bo, ns, W, t);
                const uint32_t ad = uint32_t(d < 0 ? -d : d);
                if (t != s && ad >= uint32_t(min_link)) acc += ad;
            }
        o.link[Sx] = (long long)acc;
    }
    // k_split_seed: one wave per segment (and k_split_phase0, a thread per site, behind it)
    for (size_t g = 0; g < n; ++g) {
        const uint32_t W = word_off[g + 1] - word_off[g];
        const uint64_t s0 = uint64_t(c.site_off[g]), ns = uint64_t(c.site_off[g + 1]) - s0, bo = uint64_t(bit_off[g]);
        long long best[64];
        uint32_t at[64];
        for (uint32_t lane = 0; lane < 64; ++lane) {
            best[lane] = -1, at[lane] = 0xFFFFFFFFu;
            for (uint64_t t = lane; t < ns; t += 64u)
                if (o.link[s0 + t] > best[lane]) best[lane] = o.link[s0 + t], at[lane] = uint32_t(t);
        }
        for (uint32_t d = 32; d >= 1u; d >>= 1) {
            long long nb[64];
            uint32_t na[64];
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const long long ob = best[lane ^ d];
                const uint32_t oa = at[lane ^ d];
                const bool take = ob > best[lane] || (ob == best[lane] && oa < at[lane]);
                nb[lane] = take ? ob : best[lane], na[lane] = take ? oa : at[lane];
            }
            memcpy(best, nb, sizeof best), memcpy(at, na, sizeof at);
        }
        for (uint32_t lane = 1; lane < 64; ++lane) faults += best[lane] != best[0] || at[lane] != at[0];  // (every lane holds the result)
        const bool split = ns > 0 && best[0] > 0;
        seed[g] = split ? int32_t(at[0]) : -1;
        for (uint64_t t = 0; t < ns; ++t)
            o.phase[s0 + t] = !split ? int8_t(0)
                              : t == at[0] ? int8_t(1)
                                           : split_phase(d_with_site(bm.data() + bo + at[0], bM.data() + bo + at[0], ns, bo, ns, W, t), min_link);
    }
    auto vote = [&]() {  // k_split_vote: one wave per pair
        for (size_t i = 0; i < np; ++i) {
            const uint32_t g = uint32_t(c.seg_of_pair[i]);
            const uint64_t s0 = uint64_t(c.site_off[g]), ns = uint64_t(c.site_off[g + 1]) - s0, a0 = uint64_t(c.allele_off[i]);
            int32_t sum = 0;
            for (uint32_t lane = 0; lane < 64; ++lane)
                for (uint64_t t = lane; t < ns; t += 64u) {
                    if (a0 + t >= bytes) break;
                    sum += int32_t(o.phase[s0 + t]) * split_mark(c.alleles[a0 + t], mark_minor[s0 + t], mark_major[s0 + t]);
                }
            o.vote[i] = sum, o.group[i] = split_group(sum, min_margin);
        }
    };
    vote();
    for (int32_t r = 0; r < rounds; ++r) {
        for (size_t x = 0; x < T; ++x) {  // k_group_bits: one wave per tile
            const uint32_t g = uint32_t(tile_seg[x]), m0 = mem_off[g], nr = mem_off[g + 1] - m0;
            u64 b1 = 0, b0 = 0;
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t rr = (uint32_t(x) - word_off[g]) * 64u + lane;
                const uint32_t grp = rr < nr ? o.group[members[m0 + rr]] : uint32_t(IOC_SPLIT_NONE);
                if (grp == 1u) b1 |= 1ull << lane;
                if (grp == 0u) b0 |= 1ull << lane;
            }
            g1[x] = b1, g0[x] = b0;
        }
        for (size_t Sx = 0; Sx < S; ++Sx) {  // k_split_rephase: a thread per site
            const uint32_t g = uint32_t(seg_of_site[Sx]), wo = word_off[g], W = word_off[g + 1] - wo;
            const uint64_t s0 = uint64_t(c.site_off[g]), ns = uint64_t(c.site_off[g + 1]) - s0;
            o.phase[Sx] = split_phase(d_with_site(g1.data() + wo, g0.data() + wo, 1, uint64_t(bit_off[g]), ns, W, Sx - s0), min_link);
        }
        vote();
    }
    for (size_t g = 0; g < n; ++g) {  // k_split_record
        const uint64_t s0 = uint64_t(c.site_off[g]), ns = uint64_t(c.site_off[g + 1]) - s0;
        const uint32_t m0 = mem_off[g], nr = mem_off[g + 1] - m0;
        int32_t linked = 0, c0 = 0, c1 = 0;
        for (uint64_t t = 0; t < ns; ++t) linked += o.phase[s0 + t] != 0;
        for (uint32_t r = 0; r < nr; ++r) c0 += o.group[members[m0 + r]] == 0, c1 += o.group[members[m0 + r]] == 1;
        o.rec[g] = ioc_split_seg{seed[g], linked, int32_t(nr), c0, c1, int32_t(nr) - c0 - c1, seed[g] >= 0 ? int64_t(o.link[s0 + uint32_t(seed[g])]) : int64_t(0)};
    }
    return faults;
}

// the definition, segment by segment, against what the driven kernels left
int compare(const Call& c, int32_t min_link, int32_t min_margin, int32_t rounds, const Out& o)
{
    int faults = 0;
    for (uint32_t g = 0; g < c.n_segs; ++g) {
        const int64_t s0 = c.site_off[g], ns = c.site_off[g + 1] - s0;
        std::vector<uint32_t> mem;
        for (uint32_t i = 0; i < c.n_pairs; ++i)
            if (uint32_t(c.seg_of_pair[i]) == g) mem.push_back(i);
        std::vector<uint8_t> a(mem.size() * size_t(ns) + 1);
        for (size_t r = 0; r < mem.size() && ns > 0; ++r) memcpy(a.data() + r * size_t(ns), c.alleles.data() + c.allele_off[mem[r]], size_t(ns));
        std::vector<int64_t> link(size_t(ns) + 1);
        std::vector<int8_t> phase(size_t(ns) + 1);
        std::vector<uint8_t> group(mem.size() + 1);
        std::vector<int32_t> vote(mem.size() + 1);
        ioc_split_seg rec{};
        if (ioc_host_alleles_split(c.sites.data() + s0, int32_t(ns), a.data(), int32_t(mem.size()), min_link, min_margin, rounds, link.data(), phase.data(),
                                   group.data(), vote.data(), &rec) != IOC_OK)
            return printf("the definition refused segment %u\n", g), 1;
        for (int64_t t = 0; t < ns; ++t) faults += link[size_t(t)] != o.link[size_t(s0 + t)] || phase[size_t(t)] != o.phase[size_t(s0 + t)];
        for (size_t r = 0; r < mem.size(); ++r) faults += group[r] != o.group[mem[r]] || vote[r] != o.vote[mem[r]];
        faults += memcmp(&rec, &o.rec[g], sizeof rec) != 0;
        if (faults) return printf("segment %u (%lld sites, %zu reads) differs from the definition\n", g, (long long)ns, mem.size()), faults;
    }
    return 0;
}

// a call of the given (reads, sites) per segment, the pairs dealt out in a shuffled order; planted two-group matrices with noise,
// or any bytes
Call make(std::mt19937& rng, const std::vector<std::pair<uint32_t, uint32_t>>& shape, bool planted)
{
    Call c;
    c.n_segs = uint32_t(shape.size());
    c.site_off.assign(1, 0);
    for (const auto& sh : shape) {
        for (uint32_t s = 0; s < sh.second; ++s) {
            const int32_t major = int32_t(rng() % 6u), minor = int32_t((uint32_t(major) + 1u + rng() % 5u) % 6u);
            c.sites.push_back(ioc_pile_site{int32_t(s), IOC_SITE_BASE, major, minor, 0, 0, 0, 0});
        }
        c.site_off.push_back(int64_t(c.sites.size()));
        for (uint32_t r = 0; r < sh.first; ++r) c.seg_of_pair.push_back(int32_t(c.site_off.size()) - 2);
    }
    for (size_t i = c.seg_of_pair.size(); i > 1; --i) std::swap(c.seg_of_pair[i - 1], c.seg_of_pair[rng() % i]);
    c.n_pairs = uint32_t(c.seg_of_pair.size());
    c.allele_off.assign(1, 0);
    const uint8_t any[8] = {0, 1, 2, 3, 4, 5, 7, 9};
    for (uint32_t i = 0; i < c.n_pairs; ++i) {
        const int32_t g = c.seg_of_pair[i];
        const bool side = rng() & 1u;
        for (int64_t s = c.site_off[g]; s < c.site_off[g + 1]; ++s) {
            uint8_t b = any[rng() % 8u];
            if (planted && rng() % 10u != 0) b = rng() % 5u == 0 ? uint8_t(IOC_ALLELE_NONE) : uint8_t(side ? c.sites[size_t(s)].minor : c.sites[size_t(s)].major);
            c.alleles.push_back(b);
        }
        c.allele_off.push_back(int64_t(c.alleles.size()));
    }
    return c;
}

}  // namespace

int main()
{
    std::mt19937 rng(12345);
    int faults = 0, calls = 0;
    // the four word rules against their definitions in words
    for (int x = 0; x < 2000 && !faults; ++x) {
        const u64 a = (u64(rng()) << 32 | rng()), b = (u64(rng()) << 32 | rng()) & ~a, p = (u64(rng()) << 32 | rng()), q = (u64(rng()) << 32 | rng()) & ~p;
        int32_t d = 0;
        for (uint32_t l = 0; l < 64; ++l) d += (int32_t((a >> l) & 1) - int32_t((b >> l) & 1)) * (int32_t((p >> l) & 1) - int32_t((q >> l) & 1));
        faults += d != split_d_word(a, b, p, q);
    }
    for (int d = -5; d <= 5; ++d) {
        faults += split_phase(d, 3) != (d >= 3 ? 1 : d <= -3 ? -1 : 0);
        faults += split_group(d, 2) != (d >= 2 ? 1 : d <= -2 ? 0 : IOC_SPLIT_NONE);
    }
    faults += split_mark(1, 1, 0) != 1 || split_mark(0, 1, 0) != -1 || split_mark(7, 1, 0) != 0 || split_mark(2, 1, 0) != 0 || split_mark(3, 3, 3) != 1;
    if (faults) return printf("the word rules: %d faults\n", faults), 1;

    const uint32_t reads[] = {0, 1, 63, 64, 65, 127, 128, 129, 200}, sites[] = {0, 1, 2, 63, 64, 65, 130};
    std::vector<std::pair<uint32_t, uint32_t>> all;
    for (uint32_t r : reads)
        for (uint32_t s : sites) {
            all.emplace_back(r, s);
            for (int planted = 0; planted < 2 && !faults; ++planted) {  // each size alone
                const Call c = make(rng, {{r, s}}, planted != 0);
                Out o;
                const int32_t ml = 1 + int32_t(rng() % 4u), mm = 1 + int32_t(rng() % 3u), rounds = int32_t(rng() % 4u);
                faults += drive(c, ml, mm, rounds, o);
                if (!faults) faults += compare(c, ml, mm, rounds, o);
                ++calls;
            }
        }
    for (int planted = 0; planted < 2 && !faults; ++planted)  // all in one call
        for (int32_t rounds : {0, 1, 3}) {
            const Call c = make(rng, all, planted != 0);
            Out o;
            faults += drive(c, 3, 1, rounds, o);
            if (!faults) faults += compare(c, 3, 1, rounds, o);
            ++calls;
        }
    {  // more than 64 segments of a few reads each
        std::vector<std::pair<uint32_t, uint32_t>> many;
        for (uint32_t g = 0; g < 150; ++g) many.emplace_back(rng() % 12u, rng() % 9u);
        const Call c = make(rng, many, true);
        Out o;
        faults += drive(c, 2, 1, 2, o);
        if (!faults) faults += compare(c, 2, 1, 2, o);
        ++calls;
    }
    if (faults) return printf("%d faults\n", faults), 1;
    printf("ok (%d calls)\n", calls);
    return 0;
}
