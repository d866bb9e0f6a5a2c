// insert_windows_check.cpp — the step and lane logic of the kernels of isonclust2_amd/csrc/ioc_insert_windows.hip, restated lane by lane
// on the CPU and compared with the definitions, ioc_host_ops_project_qpos, ioc_host_insert_windows and ioc_host_align_global_ops with
// ioc_host_ops_project / ioc_host_ops_project_ins (ioc_align.cpp):
//
//  * k_ops_project_qpos: the walk with PileAcc (ioc_ops_pileup.h), 64 bytes a step behind a head of 0 .. 3 bytes; the lane of a byte
//    that consumes a row stores the query bytes up to and including its own at the next row — runs of 'I' of 1 .. 300 across steps,
//    free ends, strings of 'D' alone;
//  * k_win_bounds, k_win_template: a lane per site, the class of every pair (win_class), the three counts and the rank of every voter
//    as the number of voters with a smaller (length, pair), over the members 64 at a time;
//  * k_win_align: the fill in strips of 64 columns with the rows skewed down the lanes — every lane reads its left neighbour's value
//    of the step before, lane 0 the edge buffer, lane 63 writes it in place —, two direction bits a cell packed 16 rows to a word,
//    and the walk back over the words of 64 columns held at a time, which writes the base plane and the six slot planes.
// Every buffer is a block of exactly its size, and every plane word, direction word, plane byte and record counts its writers: one
// each.  The inputs: strings of 1 .. 512 bases on either side (1, 15, 16, 17, 63, 64, 65, 128, 129, 512), identical, unrelated and
// mutated at 8 %, under four scoring sets one of which has a negative match.
//
// Host code only; meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/insert_windows_check tools/insert_windows_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/insert_windows_check
//
// Exit status 0 and "ok" when everything agrees.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ioc_insert_windows.h"
#include "ioc_ops_pileup.h"
#include "isonclust2_hip.h"

namespace {

typedef unsigned long long u64;
int faults = 0;
long long strings_seen = 0, alignments_seen = 0, strips_seen = 0, reloads_seen = 0, sites_seen = 0;

#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            if (++faults < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
        }                                                                   \
    } while (0)

// ---- k_ops_project_qpos ----
void project_qpos(const std::string& ops, uint32_t head, int32_t rlen)
{
    std::vector<uint32_t> want(size_t(rlen) + 1, 0xEEEEEEEEu), got(size_t(rlen) + 1, 0);
    std::vector<int> writers(size_t(rlen) + 1, 0);
    EXPECT(ioc_host_ops_project_qpos(ops.data(), int64_t(ops.size()), rlen, want.data()) == IOC_OK);
    const uint32_t span = head + uint32_t(ops.size()), nwords = (span + 3u) / 4u, nchunks = (nwords + 63u) / 64u;
    PileAcc acc;
    for (uint32_t c = 0; c < nchunks; ++c)
        for (uint32_t j = 0; j < 4u; ++j) {
            u64 m[6] = {0, 0, 0, 0, 0, 0};
            for (uint32_t lane = 0; lane < 64u; ++lane) {
                const uint32_t pos = c * 256u + j * 64u + lane;
                const char b = pos >= head && pos < span ? ops[pos - head] : 0;
                const char* at = b ? strchr("=XIDid", b) : nullptr;
                if (at) m[at - "=XIDid"] |= 1ull << lane;
            }
            acc.begin(m[0], m[1], m[2], m[3], m[4], m[5]);
            for (uint32_t lane = 0; lane < 64u; ++lane)
                if ((acc.m_ref >> lane) & 1ull) {
                    const uint64_t at_row = uint64_t(acc.row(lane)) + 1u;
                    EXPECT(at_row < got.size());
                    if (at_row < got.size()) got[at_row] = acc.qpos(lane) + uint32_t((acc.m_qry >> lane) & 1ull), ++writers[at_row];
                }
            acc.end();
        }
    EXPECT(got == want);
    EXPECT(writers[0] == 0);
    for (size_t r = 1; r < writers.size(); ++r) EXPECT(writers[r] == 1);
    ++strings_seen;
}

// ---- k_win_bounds, k_win_template: one segment, the members 64 at a time ----
void windows_of(const std::vector<uint8_t>& base, const std::vector<uint32_t>& qpos, const std::vector<int32_t>& qlen, int32_t rlen,
                const std::vector<ioc_pile_insert>& sites, const std::vector<uint64_t>& keys, int32_t slack, int32_t max_win)
{
    const size_t n = qlen.size(), S = sites.size(), rows = size_t(rlen) + 1;
    std::vector<ioc_insert_window> want(S), got(S);
    std::vector<uint8_t> cls(n * S);
    std::vector<uint32_t> start(n * S), len(n * S);
    EXPECT(ioc_host_insert_windows(base.data(), qpos.data(), qlen.data(), int32_t(n), rlen, sites.data(), int32_t(S), keys.data(), slack, max_win, want.data(),
                                   cls.data(), start.data(), len.data()) == IOC_OK);
    std::vector<IocWinSlot> slots(n * S);
    std::vector<int> writers(n * S, 0);
    for (size_t i = 0; i < n; ++i)          // k_win_bounds: a wave per pair, a lane per site
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            if (lane >= S) continue;
            const long long first = sites[lane].first, end = sites[lane].end;
            uint32_t c = IOC_WIN_NONE, st = 0, l = 0;
            const uint32_t state = uint32_t(keys[i] >> (2u * lane)) & 3u;
            if (win_site_ok(first, end, rlen) && state == uint32_t(IOC_INS_CARRY)) {
                const u64 po = i * rows, lo = u64(win_lo(first, slack)), hi = u64(win_hi(end, slack, rlen));
                EXPECT(po + hi < base.size() && lo >= 1);
                c = win_class(state, base[po + lo - 1], base[po + hi - 1], qpos[po + lo], qpos[po + hi], uint32_t(qlen[i]), max_win, &l);
                if (c == uint32_t(IOC_WIN_VOTER)) st = qpos[po + lo];
            }
            slots[i * S + lane] = IocWinSlot{st, win_slot_pack(c, l)}, ++writers[i * S + lane];
        }
    for (size_t x = 0; x < n * S; ++x) {
        EXPECT(writers[x] == 1 && win_slot_class(slots[x].cls_len) == cls[x]);
        if (cls[x] == IOC_WIN_VOTER) EXPECT(slots[x].start == start[x] && win_slot_len(slots[x].cls_len) == len[x]);
    }
    for (size_t k = 0; k < S; ++k) {        // k_win_template: a wave per site
        uint32_t nv = 0, nshort = 0, nlong = 0;
        for (size_t i = 0; i < n; ++i) {
            const uint32_t c = win_slot_class(slots[i * S + k].cls_len);
            nv += c == IOC_WIN_VOTER, nshort += c == IOC_WIN_SHORT, nlong += c == IOC_WIN_LONG;
        }
        int32_t t_pair = -1, t_len = 0, hits = 0;
        for (size_t a0 = 0; a0 < n && nv; a0 += 64)
            for (size_t lane = 0; lane < 64 && a0 + lane < n; ++lane) {
                const uint32_t a = slots[(a0 + lane) * S + k].cls_len;
                if (win_slot_class(a) != IOC_WIN_VOTER) continue;
                uint32_t rank = 0;
                for (size_t b = 0; b < n; ++b) {
                    const uint32_t v = slots[b * S + k].cls_len;
                    if (win_slot_class(v) == IOC_WIN_VOTER) rank += win_voter_less(win_slot_len(v), uint32_t(b), win_slot_len(a), uint32_t(a0 + lane));
                }
                if (rank == win_median_rank(nv)) t_pair = int32_t(a0 + lane), t_len = int32_t(win_slot_len(a)), ++hits;
            }
        EXPECT(nv == 0 || hits == 1);
        got[k] = ioc_insert_window{int32_t(win_lo(sites[k].first, slack)), int32_t(win_hi(sites[k].end, slack, rlen)), t_pair, t_len, nv, nshort, nlong, 0u};
        EXPECT(memcmp(&got[k], &want[k], sizeof got[k]) == 0);
        ++sites_seen;
    }
}

// ---- k_win_align: one wave ----
void align(const std::string& q, const std::string& t, int32_t match, int32_t mismatch, int32_t gap)
{
    const uint32_t qlen = uint32_t(q.size()), tlen = uint32_t(t.size());
    std::vector<char> ops(qlen + tlen + 1);
    const int64_t L = ioc_host_align_global_ops(q.data(), int32_t(qlen), t.data(), int32_t(tlen), match, mismatch, gap, ops.data(), qlen + tlen, nullptr);
    EXPECT(L >= 0);
    std::vector<uint8_t> want_base(tlen + 1), insf(tlen + 1), want_slots(size_t(IOC_PILE_INS_SLOTS) * (tlen + 1));
    EXPECT(ioc_host_ops_project(ops.data(), L, q.data(), int32_t(qlen), int32_t(tlen), want_base.data(), insf.data()) == IOC_OK);
    EXPECT(ioc_host_ops_project_ins(ops.data(), L, q.data(), int32_t(qlen), int32_t(tlen), want_slots.data()) == IOC_OK);

    const size_t P = size_t(tlen) + 1;
    std::vector<uint32_t> words(size_t(win_dir_words(qlen, tlen)), 0xDEADBEEFu);
    std::vector<int> word_writers(words.size(), 0), base_writers(P, 0), slot_writers(size_t(IOC_PILE_INS_SLOTS) * P, 0);
    std::vector<uint8_t> base(P, uint8_t(IOC_ALLELE_NONE)), slots(size_t(IOC_PILE_INS_SLOTS) * P, 0);
    std::vector<int32_t> edge(size_t(qlen) + 1);
    for (uint32_t a = 0; a <= qlen; ++a) edge[a] = -int32_t(a) * gap;
    for (uint32_t j0 = 0; j0 < tlen; j0 += 64u) {
        const uint32_t ncols = std::min(64u, tlen - j0);
        int32_t h[64], diag[64];
        uint32_t word[64];
        for (uint32_t lane = 0; lane < 64u; ++lane) h[lane] = -int32_t(j0 + lane + 1u) * gap, diag[lane] = -int32_t(j0 + lane) * gap, word[lane] = 0;
        for (uint32_t s = 0; s + 1u < qlen + ncols; ++s) {
            int32_t from_left[64];
            for (uint32_t lane = 0; lane < 64u; ++lane) from_left[lane] = lane ? h[lane - 1u] : h[0];  // (the shuffle, before any lane moves)
            for (uint32_t lane = 64u; lane-- > 0u;) {  // (lane 63 writes edge[i] of a row lane 0 read 63 steps ago: any order of the lanes does)
                const uint32_t j = j0 + lane + 1u, i = s + 1u - lane;
                if (!(j <= tlen && s >= lane && i <= qlen)) continue;
                int32_t left = from_left[lane];
                if (lane == 0u) left = edge[i];
                const int32_t dg = diag[lane] + (q[i - 1u] == t[j - 1u] ? match : mismatch), d = left - gap, in = h[lane] - gap;
                word[lane] |= win_dir(dg, d, in) << win_dir_shift(i);
                diag[lane] = left, h[lane] = win_max3(dg, d, in);
                if (lane == 63u) edge[i] = h[lane];
                if (i % uint32_t(IOC_WIN_ROWS_PER_WORD) == 0u || i == qlen) {
                    const uint64_t at = win_dir_word(i, j, tlen);
                    EXPECT(at < words.size());
                    if (at < words.size()) words[size_t(at)] = word[lane], ++word_writers[size_t(at)];
                    word[lane] = 0;
                }
            }
        }
        ++strips_seen;
    }
    for (int w : word_writers) EXPECT(w == 1);

    uint32_t i = qlen, j = tlen, run = 0, held[64], held_rb = 0xFFFFFFFFu, held_top = 0;
    auto close_run = [&]() {
        for (uint32_t lane = 0; lane < 64u; ++lane)
            if (lane < run && lane < uint32_t(IOC_PILE_INS_SLOTS) && i + lane < qlen) {
                const size_t at = size_t(lane) * P + j;
                EXPECT(j < P);
                slots[at] = uint8_t(1u + PileAcc::channel(uint8_t(q[i + lane]))), ++slot_writers[at];
            }
        run = 0;
    };
    while (i > 0u || j > 0u) {
        uint32_t d = i == 0u ? uint32_t(WIN_D) : uint32_t(WIN_I);
        if (i > 0u && j > 0u) {
            const uint32_t rb = (i - 1u) / uint32_t(IOC_WIN_ROWS_PER_WORD);
            if (rb != held_rb || j > held_top || j + 63u < held_top) {
                held_rb = rb, held_top = j, ++reloads_seen;
                for (uint32_t lane = 0; lane < 64u; ++lane) {
                    EXPECT(!(lane < j) || size_t(rb) * tlen + (j - lane - 1u) < words.size());
                    held[lane] = lane < j ? words[size_t(rb) * tlen + (j - lane - 1u)] : 0u;
                }
            }
            EXPECT(held_top - j < 64u);
            d = (held[held_top - j] >> win_dir_shift(i)) & 3u;
        }
        if (d != uint32_t(WIN_DIAG) && d != uint32_t(WIN_D)) {
            ++run, --i;
            continue;
        }
        close_run();
        EXPECT(j >= 1u && (d != uint32_t(WIN_DIAG) || i >= 1u));
        base[j - 1u] = d == uint32_t(WIN_DIAG) ? uint8_t(PileAcc::channel(uint8_t(q[i - 1u]))) : uint8_t(IOC_ALLELE_DEL), ++base_writers[j - 1u];
        if (d == uint32_t(WIN_DIAG)) --i;
        --j;
    }
    close_run();
    EXPECT(base == want_base && slots == want_slots);
    for (size_t r = 0; r < P; ++r) EXPECT(base_writers[r] == (r < tlen ? 1 : 0));
    for (size_t x = 0; x < slot_writers.size(); ++x) EXPECT(slot_writers[x] == (want_slots[x] ? 1 : 0));
    ++alignments_seen;
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

}  // namespace

int main()
{
    std::mt19937 rng(7);
    // the position plane
    for (uint32_t head = 0; head < 4u; ++head) {
        for (const char* s : {"", "====", "ii==dd", "dd==ii", "iiiii", "ddddd", "DDDDDDD", "III==", "==III", "iiIII=X=DD=IIIiiii", "dI=Id", "=iD"}) {
            const std::string ops(s);
            project_qpos(ops, head, int32_t(std::count_if(ops.begin(), ops.end(), [](char c) { return strchr("=XDd", c) != nullptr; })));
        }
        for (int run : {1, 63, 64, 65, 255, 256, 300})
            for (int before : {0, 1, 60, 200, 250, 255, 256}) {
                const std::string ops = std::string(size_t(before), '=') + std::string(size_t(run), 'I') + std::string(40, '=');
                project_qpos(ops, head, before + 40);
                project_qpos(std::string(size_t(before), '=') + std::string(size_t(run), 'I'), head, before);
            }
        for (int x = 0; x < 200; ++x) {
            std::string ops(size_t(rng() % 900u), '=');
            for (char& c : ops) c = "====XIIDid"[rng() % 8u];
            project_qpos(ops, head, int32_t(std::count_if(ops.begin(), ops.end(), [](char c) { return strchr("=XDd", c) != nullptr; })));
        }
    }
    // the windows: 0 .. 130 reads of a segment of 300 rows, three sites, classes at random
    for (int n : {0, 1, 3, 63, 64, 65, 130}) {
        const int32_t rlen = 300;
        std::vector<uint8_t> base(size_t(n) * 301);
        std::vector<uint32_t> qpos(size_t(n) * 301);
        std::vector<int32_t> qlen(static_cast<size_t>(n), 0);
        std::vector<uint64_t> keys(static_cast<size_t>(n), 0);
        for (int i = 0; i < n; ++i) {
            uint32_t q = 0;
            for (int r = 0; r <= rlen; ++r) {
                base[size_t(i) * 301 + size_t(r)] = uint8_t(rng() % 20u == 0 ? IOC_ALLELE_NONE : rng() % 6u);
                qpos[size_t(i) * 301 + size_t(r)] = q;
                q += rng() % 50u == 0 ? rng() % 60u : 1u;
            }
            qlen[size_t(i)] = int32_t(rng() % 8u == 0 ? q / 2u : q), keys[size_t(i)] = rng() & 0x3Fu;
        }
        const std::vector<ioc_pile_insert> sites = {{1, 3, 0, 0, 0, 0, 0, 0}, {100, 120, 0, 0, 0, 0, 0, 0}, {297, 300, 0, 0, 0, 0, 0, 0}};
        for (int32_t slack : {0, 8, 32})
            for (int32_t max_win : {1, 40, 512}) windows_of(base, qpos, qlen, rlen, sites, keys, slack, max_win);
    }
    // the alignments
    const int params[4][3] = {{2, -2, 2}, {1, -1, 1}, {5, -4, 2}, {-7, -8, 1}};
    const size_t lens[] = {1, 15, 16, 17, 63, 64, 65, 128, 129, 512};
    for (const auto& p : params) {
        align("AAAA", "AAA", p[0], p[1], p[2]), align("AAA", "AAAA", p[0], p[1], p[2]), align("A", "C", p[0], p[1], p[2]), align("ACGT", "TGCA", p[0], p[1], p[2]);
        for (size_t tl : lens) {
            const std::string t = random_bases(rng, tl);
            for (size_t ql : lens) {
                std::string q = mutate(rng, t, 0.08);
                while (q.size() < ql) q += mutate(rng, t, 0.08);
                align(q.substr(0, ql), t, p[0], p[1], p[2]);
            }
            align(t, t, p[0], p[1], p[2]);
            align(random_bases(rng, tl), t, p[0], p[1], p[2]);
        }
    }
    for (int x = 0; x < 300; ++x) {
        const std::string t = random_bases(rng, 1 + rng() % 200u);
        align(mutate(rng, t, 0.08), t, 2, -2, 2);
    }
    printf("%s: %lld strings, %lld sites, %lld alignments (%lld strips, %lld reloads of the walk), %d faults\n", faults ? "FAILED" : "ok", strings_seen, sites_seen,
           alignments_seen, strips_seen, reloads_seen, faults);
    return faults ? 1 : 0;
}
