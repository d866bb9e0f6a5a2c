// window_variants_check.cpp — the lane logic of the kernels of isonclust2_amd/csrc/ioc_window_variants.hip, restated lane by lane on the
// CPU and compared with the definitions, ioc_host_ops_agreement and ioc_host_insert_window_variants (ioc_align.cpp):
//
//  * k_win_agree: a lane per template row in chunks of 64 over the voter's base plane in the template's frame (as
//    ioc_host_ops_project leaves it for the bytes of ioc_host_align_global_ops) and the template's bytes — eq and del by ballot, the
//    agreement from the two lengths (winvar_plane_agreement) against the agreement of the bytes; templates of 1, 63, 64, 65, 128, 129
//    and 512 bases, voters identical, unrelated and mutated at 8 %, under three scoring sets;
//  * k_win_template_far: n_far by ballot and the rank of every far voter as the number of far voters with a smaller (length, pair),
//    over the members 64 at a time;
//  * k_win_decide: the counts by ballot, the decision, the record and the variant byte of every entry, one writer each;
//  * k_win_rekey: a lane per site, key2 and mask2 by an OR over the lanes.
// The segments: 1 .. 130 reads whose windows at two sites come from up to three families of strings, with carriers that are no
// voters, so that sites split, do not split for either reason, and leave voters over.  Every buffer is a block of exactly its size.
//
// Host code only; meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/window_variants_check tools/window_variants_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/window_variants_check
//
// Exit status 0 and "ok" when everything agrees.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ioc_ops_pileup.h"
#include "ioc_read_blocks.h"
#include "ioc_window_variants.h"
#include "isonclust2_hip.h"

namespace {

typedef unsigned long long u64;
int faults = 0;
long long alignments_seen = 0, sites_seen = 0, splits_seen = 0, round_b_seen = 0, others_seen = 0, reads_seen = 0;

#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            if (++faults < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
        }                                                                   \
    } while (0)

// ---- k_win_agree: one wave ----
int32_t lane_agreement(const std::string& q, const std::string& t, int32_t match, int32_t mismatch, int32_t gap)
{
    const uint32_t qlen = uint32_t(q.size()), tlen = uint32_t(t.size());
    std::vector<char> ops(qlen + tlen + 1);
    const int64_t L = ioc_host_align_global_ops(q.data(), int32_t(qlen), t.data(), int32_t(tlen), match, mismatch, gap, ops.data(), qlen + tlen, nullptr);
    EXPECT(L >= 0);
    int32_t want = 0;
    EXPECT(ioc_host_ops_agreement(ops.data(), L, &want) == IOC_OK);
    std::vector<uint8_t> base(tlen + 1), insf(tlen + 1);  // (exactly the plane: tlen + 1 bytes)
    EXPECT(ioc_host_ops_project(ops.data(), L, q.data(), int32_t(qlen), int32_t(tlen), base.data(), insf.data()) == IOC_OK);
    uint32_t eq = 0, del = 0;
    for (uint32_t j0 = 0; j0 < tlen; j0 += 64u) {
        u64 m_eq = 0, m_del = 0;
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            const uint32_t j = j0 + lane;
            if (j >= tlen) continue;
            const uint32_t b = base[j], ch = PileAcc::channel(uint8_t(t[j]));
            if (b == ch) m_eq |= 1ull << lane;
            if (b == uint32_t(IOC_ALLELE_DEL)) m_del |= 1ull << lane;
        }
        eq += uint32_t(__builtin_popcountll(m_eq)), del += uint32_t(__builtin_popcountll(m_del));
    }
    EXPECT(tlen - del <= qlen);
    const int32_t got = winvar_plane_agreement(qlen, tlen, eq, del);
    EXPECT(got == want);
    ++alignments_seen;
    return got;
}

std::string random_bases(std::mt19937& rng, size_t n)
{
    std::string s(n, 'A');
    for (char& c : s) c = "ACGT"[rng() & 3u];
    return s;
}
std::string mutate(std::mt19937& rng, const std::string& s, double rate)
{
    std::string out;
    std::uniform_real_distribution<double> u(0, 1);
    for (char c : s) {
        const double x = u(rng);
        if (x < rate / 3) continue;
        out.push_back(x < 2 * rate / 3 ? "ACGT"[rng() & 3u] : c);
        if (x > 1 - rate / 3) out.push_back("ACGT"[rng() & 3u]);
    }
    return out.empty() ? std::string("A") : out;
}

// ---- one segment through the four kernels, the members 64 at a time ----
// A segment of 40 rows and two sites, [10, 11) and [30, 31), at slack 0: a read's window at a site is what it inserts in front of the
// site's row and that row's base.  kind[i][k]: 0 lacks, 1 .. 3 a copy of family 1 .. 3 mutated at 5 %, 4 carries and does not
// cover (IOC_WIN_SHORT), 5 carries more than max_win bases (IOC_WIN_LONG).
void segment(std::mt19937& rng, size_t n, const uint32_t share[6], const WinVarRule& rule)
{
    const int32_t rlen = 40, slack = 0, max_win = 64;
    const size_t rows = size_t(rlen) + 1, S = 2;
    const uint32_t site_row[2] = {10, 30};
    const std::string frame = random_bases(rng, size_t(rlen));
    std::string family[2][3];
    for (auto& f : family)
        for (auto& s : f) s = random_bases(rng, 30 + rng() % 20u);
    std::vector<uint8_t> base(n * rows, 0);
    std::vector<uint32_t> qpos(n * rows, 0);
    std::vector<int32_t> qlen(n);
    std::vector<uint64_t> keys(n, 0);
    std::vector<int64_t> read_off{0};
    std::string reads;
    const uint32_t total = share[0] + share[1] + share[2] + share[3] + share[4] + share[5];
    for (size_t i = 0; i < n; ++i) {
        std::string rd;
        size_t k = 0;
        for (uint32_t r = 0; r <= uint32_t(rlen); ++r) {
            qpos[i * rows + r] = uint32_t(rd.size());  // (the bytes up to and including row r - 1's: what a read inserts in front of row r begins here)
            base[i * rows + r] = r < uint32_t(rlen) ? uint8_t(PileAcc::channel(uint8_t(frame[r]))) : uint8_t(IOC_ALLELE_NONE);
            if (k < S && r == site_row[k]) {
                uint32_t pick = rng() % total, kind = 0;
                while (pick >= share[kind]) pick -= share[kind++];
                if (kind >= 1 && kind <= 3) rd += mutate(rng, family[k][kind - 1], 0.05);
                if (kind == 4) rd += random_bases(rng, 20), base[i * rows + r - 1] = uint8_t(IOC_ALLELE_NONE);  // (row lo - 1 of the site)
                if (kind == 5) rd += random_bases(rng, size_t(max_win) + 5);
                if (kind) keys[i] |= uint64_t(IOC_INS_CARRY) << (2 * k);
                ++k;
            }
            if (r < uint32_t(rlen)) rd += frame[r];
        }
        qlen[i] = int32_t(rd.size()), reads += rd, read_off.push_back(int64_t(reads.size()));
    }
    const std::vector<ioc_pile_insert> sites = {{int32_t(site_row[0]), int32_t(site_row[0]) + 1, 0, 0, 0, 0, 0, 0}, {int32_t(site_row[1]), int32_t(site_row[1]) + 1, 0, 0, 0, 0, 0, 0}};

    std::vector<ioc_insert_window> win(S);
    std::vector<ioc_window_variant> want_var(S);
    std::vector<uint8_t> want_variant(n * S, 0xEE);
    std::vector<int32_t> want_agree(n * S * 2, 0);
    std::vector<uint64_t> want_key2(n), want_mask2(n);
    EXPECT(ioc_host_insert_window_variants(base.data(), qpos.data(), qlen.data(), int32_t(n), rlen, sites.data(), int32_t(S), keys.data(), reads.data(), read_off.data(), slack,
                                           max_win, 2, -2, 2, 1, rule.min_agree, rule.min_alt, rule.min_pct, win.data(), want_var.data(), want_variant.data(),
                                           want_agree.data(), nullptr, nullptr, 0, nullptr, nullptr, want_key2.data(), want_mask2.data()) == IOC_OK);
    std::vector<uint8_t> cls(n * S);
    std::vector<uint32_t> start(n * S), len(n * S);
    EXPECT(ioc_host_insert_windows(base.data(), qpos.data(), qlen.data(), int32_t(n), rlen, sites.data(), int32_t(S), keys.data(), slack, max_win, win.data(), cls.data(),
                                   start.data(), len.data()) == IOC_OK);
    auto window = [&](size_t i, size_t k) { return reads.substr(size_t(read_off[i]) + start[i * S + k], len[i * S + k]); };

    // the tables as the device holds them: an entry per (pair, site), the flags of both rounds behind one another
    const size_t E = n * S;
    std::vector<uint8_t> flag(2 * E, WINVAR_UNSEEN), variant(E, 0);
    std::vector<int32_t> agree(2 * E, INT32_MIN);
    std::vector<int> variant_writers(E, 0), flag_writers(2 * E, 0);
    std::vector<ioc_window_variant> var(S);
    auto run_round = [&](size_t k, size_t t, int which, const std::vector<size_t>& who) {  // k_win_agree over the items the host lists
        for (const size_t i : who) {
            const std::string q = window(i, k), tw = window(t, k);
            const int32_t a = lane_agreement(q, tw, 2, -2, 2);
            const size_t e = size_t(which) * E + i * S + k;
            agree[e] = a, flag[e] = winvar_near(a, uint32_t(q.size()), uint32_t(tw.size()), rule.min_agree) ? WINVAR_NEAR : WINVAR_FAR, ++flag_writers[e];
        }
    };
    for (size_t k = 0; k < S; ++k) {
        std::vector<size_t> voters, far;
        for (size_t i = 0; i < n; ++i)
            if (cls[i * S + k] == IOC_WIN_VOTER) voters.push_back(i);
        if (win[k].tlen > 0) run_round(k, size_t(win[k].template_pair), 0, voters);
        // k_win_template_far: a wave per site
        auto is_far = [&](size_t m) { return m < n && cls[m * S + k] == IOC_WIN_VOTER && flag[m * S + k] == WINVAR_FAR; };
        uint32_t n_far = 0;
        for (size_t m0 = 0; m0 < n; m0 += 64) {
            u64 ballot = 0;
            for (size_t lane = 0; lane < 64; ++lane) ballot |= u64(is_far(m0 + lane)) << lane;
            n_far += uint32_t(__builtin_popcountll(ballot));
        }
        const bool runs = winvar_round_b(rule, win[k].n_voters, n_far);
        int32_t t_pair = -1, t_len = 0, hits = 0;
        for (size_t a0 = 0; a0 < n && runs; a0 += 64)
            for (size_t lane = 0; lane < 64; ++lane) {
                if (!is_far(a0 + lane)) continue;
                uint32_t rank = 0;
                for (size_t b0 = 0; b0 < n; b0 += 64)
                    for (size_t r = 0; r < 64; ++r)  // (the far voters of a chunk, handed round one by one)
                        if (is_far(b0 + r)) rank += win_voter_less(len[(b0 + r) * S + k], uint32_t(b0 + r), len[(a0 + lane) * S + k], uint32_t(a0 + lane));
                if (rank == win_median_rank(n_far)) t_pair = int32_t(a0 + lane), t_len = int32_t(len[(a0 + lane) * S + k]), ++hits;
            }
        EXPECT(!runs || hits == 1);
        var[k] = ioc_window_variant{0, t_pair, t_len, 0, 0, 0, n_far, 0};
        if (t_pair >= 0) {
            for (const size_t i : voters)
                if (flag[i * S + k] == WINVAR_FAR) far.push_back(i);
            run_round(k, size_t(t_pair), 1, far);
            ++round_b_seen;
        }
        // k_win_decide: a wave per site
        uint32_t nv = 0, nf = 0, nb = 0;
        for (size_t m0 = 0; m0 < n; m0 += 64) {
            u64 b_v = 0, b_f = 0, b_b = 0;
            for (size_t lane = 0; lane < 64 && m0 + lane < n; ++lane) {
                const size_t e = (m0 + lane) * S + k;
                const bool votes = cls[e] == IOC_WIN_VOTER, farv = votes && flag[e] == WINVAR_FAR;
                b_v |= u64(votes) << lane, b_f |= u64(farv) << lane, b_b |= u64(farv && flag[E + e] == WINVAR_NEAR) << lane;
            }
            nv += uint32_t(__builtin_popcountll(b_v)), nf += uint32_t(__builtin_popcountll(b_f)), nb += uint32_t(__builtin_popcountll(b_b));
        }
        const bool ran = winvar_round_b(rule, nv, nf) && var[k].template_pair_b >= 0;
        if (!ran) nb = 0;
        const bool split = ran && winvar_splits(rule, nv, nf, nb);
        for (size_t m = 0; m < n; ++m) {
            const size_t e = m * S + k;
            variant[e] = winvar_variant(cls[e], split, flag[e], flag[E + e]), ++variant_writers[e];
            others_seen += variant[e] == IOC_WINVAR_OTHER;
        }
        var[k].split = split, var[k].n_a = split ? nv - nf : nv, var[k].n_b = nb, var[k].n_other = ran ? nf - nb : 0u, var[k].n_far = nf;
        EXPECT(memcmp(&var[k], &want_var[k], sizeof var[k]) == 0);
        splits_seen += split, ++sites_seen;
    }
    for (size_t e = 0; e < E; ++e) {
        EXPECT(variant_writers[e] == 1 && variant[e] == want_variant[e]);
        EXPECT(flag_writers[e] <= 1 && flag_writers[E + e] <= 1);
        EXPECT(agree[e] == want_agree[2 * e] && agree[E + e] == want_agree[2 * e + 1]);
    }
    // k_win_rekey: a wave per pair, a lane per site
    for (size_t i = 0; i < n; ++i) {
        u64 key = 0, mask = 0, mine = 0;
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            if (lane >= S) continue;
            const uint32_t st = winvar_state(uint32_t(keys[i] >> (2u * lane)) & 3u, cls[i * S + lane], var[lane].split != 0, variant[i * S + lane]);
            key |= u64(st) << (2u * lane), mask |= blocks_state_mask(lane, st), mine |= 3ull << (2u * lane);
        }
        EXPECT((key | (keys[i] & ~mine)) == want_key2[i] && mask == want_mask2[i]);
        ++reads_seen;
    }
}

}  // namespace

int main()
{
    std::mt19937 rng(11);
    const int params[3][3] = {{2, -2, 2}, {1, -1, 1}, {5, -4, 2}};
    const size_t lens[] = {1, 63, 64, 65, 128, 129, 512};
    for (const auto& p : params)
        for (size_t tl : lens) {
            const std::string t = random_bases(rng, tl);
            EXPECT(lane_agreement(t, t, p[0], p[1], p[2]) == int32_t(tl));
            lane_agreement(random_bases(rng, tl), t, p[0], p[1], p[2]);
            for (size_t ql : lens) {
                std::string q = mutate(rng, t, 0.08);
                while (q.size() < ql) q += mutate(rng, t, 0.08);
                lane_agreement(q.substr(0, ql), t, p[0], p[1], p[2]);
            }
        }
    lane_agreement("ACGTN", "ACGTN", 2, -2, 2), lane_agreement("A", "C", 2, -2, 2), lane_agreement("AAAA", "AAA", 2, -2, 2), lane_agreement("AAA", "AAAA", 2, -2, 2);
    // the segments: the shares of (lacks, family 1, family 2, family 3, short, long)
    const uint32_t shares[5][6] = {{2, 5, 5, 0, 1, 1}, {2, 9, 1, 0, 0, 0}, {2, 5, 3, 2, 1, 0}, {1, 1, 1, 1, 0, 0}, {4, 6, 0, 0, 0, 0}};
    const WinVarRule rules[3] = {{45, 3, 25}, {45, 1, 1}, {60, 2, 50}};
    for (const size_t n : {1, 2, 7, 20, 63, 64, 65, 130})
        for (const auto& sh : shares)
            for (const WinVarRule& rule : rules) segment(rng, n, sh, rule);
    printf("%s: %lld alignments, %lld sites (%lld with a round B, %lld split), %lld voters left over, %lld reads re-keyed, %d faults\n", faults ? "FAILED" : "ok",
           alignments_seen, sites_seen, round_b_seen, splits_seen, others_seen, reads_seen, faults);
    return faults || !splits_seen || !others_seen || round_b_seen == splits_seen ? 1 : 0;
}
