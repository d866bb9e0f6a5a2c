// pile_sites_check.cpp — the host-callable logic behind the variable sites, driven on the CPU as its kernels drive it and compared
// with the definitions in ioc_align.cpp:
//
//  * PileAcc (isonclust2_amd/csrc/ioc_ops_pileup.h) as k_ops_project uses it — 64-byte steps from the aligned-down address at
//    every head offset 0 .. 3, one "lane" per byte, a base or 'D' lane storing its channel into the base plane at its row, the
//    lane of the first 'I' of a run storing 1 into the ins plane — against ioc_host_ops_project: runs of 'I' across step
//    boundaries at every phase, random strings.  Every byte of the planes must have at most one writer;
//  * pile_sites_row (ioc_pile_sites.h) as k_pile_sites uses it — a lane per row, insertion site before base site, emission cut at
//    max_sites — against ioc_host_pileup_sites over random tables, counters up to 2^32 - 1 included;
//  * pile_site_allele as k_site_alleles uses it against ioc_host_site_alleles.
//
// Host code only; meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/pile_sites_check tools/pile_sites_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/pile_sites_check
//
// Exit status 0 and "ok" when everything agrees.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ioc_pile_sites.h"
#include "isonclust2_hip.h"

namespace {

// k_ops_project's loop over one string that stands `head` bytes behind a dword boundary.  The planes are handed over in blocks of
// exactly rlen + 1 bytes, so that a store outside them is the sanitizer's to find; `writers` counts the stores per byte.
int drive(const std::string& ops, const std::string& query, uint32_t rlen, uint32_t head, std::vector<uint8_t>& base, std::vector<uint8_t>& insf,
          std::vector<uint8_t>& writers)
{
    int faults = 0;
    const uint32_t qlen = uint32_t(query.size());
    const uint32_t span = head + uint32_t(ops.size());
    const uint32_t nsteps = (((span + 3u) / 4u + 63u) / 64u) * 4u;
    auto mask = [&](uint32_t step, char what) {
        unsigned long long m = 0;
        for (uint32_t l = 0; l < 64u; ++l) {
            const uint32_t pos = step * 64u + l;
            const char b = (pos >= head && pos < span) ? ops[pos - head] : char(0);
            if (b == what) m |= 1ull << l;
        }
        return m;
    };
    PileAcc acc;
    for (uint32_t s = 0; s < nsteps; ++s) {
        acc.begin(mask(s, '='), mask(s, 'X'), mask(s, 'I'), mask(s, 'D'), mask(s, 'i'), mask(s, 'd'));
        for (uint32_t l = 0; l < 64u; ++l) {
            const uint32_t row = acc.row(l), at = acc.qpos(l);
            if (!acc.is_base(l) && !acc.is_del(l) && !acc.run_start(l)) continue;
            if (row > rlen) {
                ++faults;
                continue;
            }
            if (acc.is_base(l)) {
                if (at >= qlen) {
                    ++faults;
                    continue;
                }
                base[row] = uint8_t(PileAcc::channel(uint8_t(query[at])));
                ++writers[row];
            } else if (acc.is_del(l)) {
                base[row] = uint8_t(IOC_ALLELE_DEL);
                ++writers[row];
            } else {
                insf[row] = 1;
                ++writers[size_t(rlen) + 1u + row];
            }
        }
        acc.end();
    }
    return faults;
}

long g_strings = 0, g_tables = 0, g_alleles = 0, g_run_over_edge = 0, g_cut = 0, g_two = 0;

// `one_run`: no two runs of 'I' in front of one row (as an aligner's strings are), so that every byte has exactly one writer
bool check(const std::string& ops, std::mt19937& rng, bool one_run)
{
    uint32_t qlen = 0, rlen = 0;
    for (char b : ops) {
        qlen += b == '=' || b == 'X' || b == 'I' || b == 'i';
        rlen += b == '=' || b == 'X' || b == 'D' || b == 'd';
    }
    std::string query(qlen, 'A');
    for (char& ch : query) ch = "ACGTACGTACGTNacR"[rng() % 16u];
    std::vector<uint8_t> want_b(rlen + 1u, 0xEE), want_i(rlen + 1u, 0xEE);
    if (ioc_host_ops_project(ops.data(), int64_t(ops.size()), query.data(), int32_t(qlen), int32_t(rlen), want_b.data(), want_i.data()) != IOC_OK) {
        fprintf(stderr, "the definition refused a string of %zu bytes\n", ops.size());
        return false;
    }
    for (uint32_t head = 0; head < 4u; ++head) {
        std::vector<uint8_t> got_b(rlen + 1u, uint8_t(IOC_ALLELE_NONE)), got_i(rlen + 1u, 0), writers(2u * (rlen + 1u), 0);
        const int faults = drive(ops, query, rlen, head, got_b, got_i, writers);
        ++g_strings;
        if (faults || got_b != want_b || got_i != want_i) {
            fprintf(stderr, "mismatch: %zu bytes, head %u, %d faults: %.120s\n", ops.size(), head, faults, ops.c_str());
            return false;
        }
        for (size_t x = 0; x < writers.size(); ++x)
            if (writers[x] > 1u && (one_run || x <= rlen)) {
                fprintf(stderr, "byte %zu has %u writers: %.120s\n", x, unsigned(writers[x]), ops.c_str());
                return false;
            }
        for (size_t x = 1; x < ops.size(); ++x) g_run_over_edge += ops[x] == 'I' && ops[x - 1] == 'I' && (head + x) % 64u == 0u;
    }
    // the alleles of this projection at a site of either kind on every row: the shared function against the definition
    std::vector<ioc_pile_site> sites;
    for (uint32_t p = 0; p <= rlen; ++p) {
        sites.push_back(ioc_pile_site{int32_t(p), IOC_SITE_INS, 0, 1, 0, 0, 0, 0});
        if (p < rlen) sites.push_back(ioc_pile_site{int32_t(p), IOC_SITE_BASE, 0, 1, 0, 0, 0, 0});
    }
    std::vector<uint8_t> want_a(sites.size(), 0xEE);
    if (ioc_host_site_alleles(want_b.data(), want_i.data(), int32_t(rlen), sites.data(), int32_t(sites.size()), want_a.data()) != IOC_OK) return false;
    const uint8_t b_last = rlen > 0u ? want_b[rlen - 1u] : uint8_t(IOC_ALLELE_NONE);
    for (size_t s = 0; s < sites.size(); ++s) {
        const uint32_t row = uint32_t(sites[s].row);
        ++g_alleles;
        if (pile_site_allele(sites[s].kind, row == rlen, want_b[row], want_i[row], b_last) != want_a[s]) {
            fprintf(stderr, "allele mismatch at row %u kind %d\n", row, sites[s].kind);
            return false;
        }
    }
    return true;
}

// one segment as k_pile_sites walks it — the count pass, then the emission with its running index — against the definition
bool check_sites(int32_t rlen, const PileSiteRule& rule, int32_t max_sites, bool big, std::mt19937& rng)
{
    const uint32_t small[8] = {0u, 1u, 2u, 3u, 4u, 5u, 10u, 40u}, large[6] = {0u, 1u, 3u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
    auto draw = [&]() { return big ? large[rng() % 6u] : small[rng() % 8u]; };
    std::vector<ioc_pileup_col> cols(size_t(rlen) + 1u, ioc_pileup_col{});
    for (auto& c : cols) c = rng() % 6u ? ioc_pileup_col{draw(), draw(), draw(), draw(), draw(), draw(), draw(), draw()} : ioc_pileup_col{};
    std::vector<ioc_pile_site> want(static_cast<size_t>(max_sites), ioc_pile_site{});
    int64_t want_found = -1;
    const int64_t n = ioc_host_pileup_sites(cols.data(), rlen, rule.min_depth, rule.min_alt, rule.min_pct, max_sites, want.data(), &want_found);
    if (n < 0 || n > max_sites || n > want_found || want_found > 2 * int64_t(rlen) + 1) {
        fprintf(stderr, "the definition returned %lld of %lld for rlen %d\n", (long long)n, (long long)want_found, rlen);
        return false;
    }
    std::vector<ioc_pile_site> got;
    uint32_t k = 0;
    for (int32_t p = 0; p <= rlen; ++p) {  // (as `decide` of ioc_pile_sites.hip puts the row's arguments together)
        const bool has_base = p < rlen;
        const size_t at = size_t(p);
        const unsigned long long d_ins = has_base ? pile_depth(cols[at]) : rlen > 0 ? pile_depth(cols[at - 1u]) : 0ull;
        const PileRowSites r = pile_sites_row(cols[at], d_ins, has_base, p, rule);
        if (r.n() != uint32_t(r.has_ins) + uint32_t(r.has_base)) return false;
        const uint32_t k0 = k, k1 = k0 + uint32_t(r.has_ins);
        if (r.has_ins && k0 < uint32_t(max_sites)) got.push_back(r.ins);
        if (r.has_base && k1 < uint32_t(max_sites)) got.push_back(r.base);
        g_two += r.n() == 2u;
        k += r.n();
    }
    ++g_tables;
    g_cut += int64_t(k) > n;
    if (int64_t(k) != want_found || int64_t(got.size()) != n || (n > 0 && memcmp(got.data(), want.data(), size_t(n) * sizeof(ioc_pile_site)) != 0)) {
        fprintf(stderr, "sites mismatch: rlen %d, rule %d %d %d, max %d\n", rlen, rule.min_depth, rule.min_alt, rule.min_pct, max_sites);
        return false;
    }
    return true;
}

}  // namespace

int main()
{
    static_assert(sizeof(ioc_pile_site) == 32, "record layout");
    std::mt19937 rng(4321);
    bool ok = true;
    for (const char* s : {"", "=", "D", "I", "i", "d", "I=", "=I", "iI=", "dD=", "=Dd", "=Ii", "ddii=X=iidd", "iiII==DDdd", "=IDIDID=", "=IIDDDIIII=",
                          "IIIIIIII", "=IIIIIIIID=", "d=XIID=i"})
        ok = ok && check(s, rng, true);
    // one run of G 'I's at every phase of a step: across every step boundary at every offset; a 'D' directly behind it
    for (uint32_t G : {1u, 2u, 6u, 7u, 8u, 63u, 64u, 65u, 130u, 300u})
        for (uint32_t p = 0; p < 80u && ok; ++p)
            ok = ok && check(std::string(40u + p, '=') + std::string(G, 'I') + std::string(70u, '='), rng, true) &&
                 check(std::string(p, '=') + std::string(G, 'I') + "D" + std::string(G, 'I'), rng, true) &&
                 check(std::string(p, 'd') + std::string(G, 'I') + std::string(G, 'D') + std::string(p, 'X') + std::string(G, 'i'), rng, true);
    // random strings over the six bytes, short runs and long ones: one run of 'I' per row, then anything
    for (int t = 0; t < 4000 && ok; ++t) {
        std::string s;
        const uint32_t runs = rng() % 60u;
        char last = 0;
        for (uint32_t x = 0; x < runs; ++x) {
            const uint32_t n = (rng() % 4u == 0) ? 1u + rng() % 150u : 1u + rng() % 8u;
            char b = "=XIDidDI"[rng() % 8u];
            if (t % 2 == 0 && (b == 'I' || b == 'i') && (last == 'I' || last == 'i')) b = '=';
            s.append(n, b);
            last = b;
        }
        ok = check(s, rng, t % 2 == 0);
    }
    if (!ok) return 1;
    for (int32_t rlen : {0, 1, 2, 63, 64, 65, 300})
        for (const PileSiteRule rule : {PileSiteRule{1, 1, 1}, PileSiteRule{3, 3, 25}, PileSiteRule{11, 2, 50}, PileSiteRule{3, 1, 10}})
            for (int32_t mx : {1, 2, 7, 4096})
                for (int big = 0; big < 2; ++big)
                    for (int t = 0; t < 10 && ok; ++t) ok = check_sites(rlen, rule, mx, big != 0, rng);
    if (!ok) return 1;
    if (!g_run_over_edge || !g_cut || !g_two) {
        fprintf(stderr, "a case the check is for did not occur\n");
        return 1;
    }
    printf("ok: %ld projections agree with ioc_host_ops_project (a run of 'I' across a step boundary %ld times), %ld alleles with "
           "ioc_host_site_alleles, %ld tables with ioc_host_pileup_sites (%ld cut at max_sites, %ld rows with two records)\n",
           g_strings, g_run_over_edge, g_alleles, g_tables, g_cut, g_two);
    return 0;
}
