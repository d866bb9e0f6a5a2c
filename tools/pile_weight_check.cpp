// pile_weight_check.cpp — the host-callable step logic behind the quality-weighted pileup and call, driven on the CPU as its kernels
// drive it and compared with the definitions in ioc_align.cpp:
//
//  * PileAcc with pile_qual_weight / del_weight (isonclust2_amd/csrc/ioc_ops_pileup.h), as the weighted variant of k_ops_pileup
//    uses it — 64-byte steps from the aligned-down address at every head offset 0 .. 3, one "lane" per byte, a base or 'I' lane
//    reading its own quality byte and a 'D' lane those of its one or two neighbours — against ioc_host_ops_pileup_weighted, over
//    quality bytes 0 .. 255: 'D' as the first and as the last byte of a step, 'D' in front of the first query base and behind the
//    last one (which no aligner's string puts in front of the kernel), runs of 'I' across step boundaries, random strings;
//  * pile_call_row with both gates (ioc_pile_call.h), as the weighted mode of k_pile_call uses it — a lane per row, the gates from
//    the table of counts, the decision from the tables of weights — against ioc_host_pileup_call_weighted over random tables,
//    counters up to 2^32 - 1 included.
//
// Host code only; meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/pile_weight_check tools/pile_weight_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/pile_weight_check
//
// Exit status 0 and "ok" when everything agrees.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ioc_pile_call.h"
#include "isonclust2_hip.h"

namespace {

constexpr uint32_t INS_WORDS = sizeof(ioc_pileup_ins) / 4, INS_LONGER = IOC_PILE_INS_SLOTS * 5;

// the weighted variant's loop over one string that stands `head` bytes behind a dword boundary.  The quality bytes are handed over
// in a block of exactly qlen bytes, so that a read outside them is the sanitizer's to find.
int drive(const std::string& ops, const std::string& query, const std::vector<uint8_t>& qual, uint32_t rlen, uint32_t head,
          std::vector<ioc_pileup_col>& wcols, std::vector<ioc_pileup_ins>& wins)
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
            if (!acc.is_base(l) && !acc.is_del(l) && !acc.is_ins(l)) continue;
            if (row > rlen) {
                ++faults;
                continue;
            }
            uint32_t* rec = reinterpret_cast<uint32_t*>(&wcols[row]);
            if (acc.is_base(l)) {
                if (at >= qlen) {
                    ++faults;
                    continue;
                }
                rec[PileAcc::channel(uint8_t(query[at]))] += pile_qual_weight(qual[at]);
            } else if (acc.is_del(l)) {
                rec[PILE_DEL] += acc.del_weight(l, qlen, qual.data());
            } else {
                if (at >= qlen) {
                    ++faults;
                    continue;
                }
                const uint32_t j = acc.ins_index(l);
                uint32_t* irec = reinterpret_cast<uint32_t*>(&wins[row]);
                irec[j < uint32_t(IOC_PILE_INS_SLOTS) ? j * 5u + PileAcc::channel(uint8_t(query[at])) : INS_LONGER] += pile_qual_weight(qual[at]);
            }
        }
        acc.end_len();
        acc.end();
    }
    return faults;
}

long g_strings = 0, g_tables = 0, g_del_first = 0, g_del_last = 0, g_del_q0 = 0, g_del_qn = 0;

bool check(const std::string& ops, std::mt19937& rng)
{
    uint32_t qlen = 0, rlen = 0;
    for (char b : ops) {
        qlen += b == '=' || b == 'X' || b == 'I' || b == 'i';
        rlen += b == '=' || b == 'X' || b == 'D' || b == 'd';
    }
    std::string query(qlen, 'A');
    for (char& ch : query) ch = "ACGTACGTACGTNacR"[rng() % 16u];
    std::vector<uint8_t> qual(qlen);
    const uint8_t edge[8] = {0, 33, 34, 35, 73, 126, 127, 255};
    for (uint8_t& b : qual) b = rng() % 3u ? uint8_t(rng() % 256u) : edge[rng() % 8u];
    std::vector<ioc_pileup_col> want_c(rlen + 1u, ioc_pileup_col{});
    std::vector<ioc_pileup_ins> want_i(rlen + 1u, ioc_pileup_ins{});
    if (ioc_host_ops_pileup_weighted(ops.data(), int64_t(ops.size()), query.data(), reinterpret_cast<const char*>(qual.data()), int32_t(qlen),
                                     int32_t(rlen), want_c.data(), want_i.data()) != IOC_OK) {
        fprintf(stderr, "the definition refused a string of %zu bytes\n", ops.size());
        return false;
    }
    for (uint32_t head = 0; head < 4u; ++head) {
        std::vector<ioc_pileup_col> got_c(rlen + 1u, ioc_pileup_col{});
        std::vector<ioc_pileup_ins> got_i(rlen + 1u, ioc_pileup_ins{});
        const int faults = drive(ops, query, qual, rlen, head, got_c, got_i);
        ++g_strings;
        if (faults || memcmp(got_c.data(), want_c.data(), want_c.size() * sizeof(ioc_pileup_col)) != 0 ||
            memcmp(got_i.data(), want_i.data(), want_i.size() * sizeof(ioc_pileup_ins)) != 0) {
            fprintf(stderr, "mismatch: %zu bytes, head %u, %d faults: %.120s\n", ops.size(), head, faults, ops.c_str());
            return false;
        }
        // what the cases covered: a 'D' on a step's first / last byte, in front of the first query base, behind the last one
        uint32_t q = 0;
        for (size_t x = 0; x < ops.size(); ++x) {
            if (ops[x] == 'D') {
                g_del_first += (head + x) % 64u == 0u, g_del_last += (head + x) % 64u == 63u;
                g_del_q0 += q == 0u, g_del_qn += q == qlen;
            }
            q += ops[x] == '=' || ops[x] == 'X' || ops[x] == 'I' || ops[x] == 'i';
        }
    }
    return true;
}

// one segment as the weighted mode of k_pile_call walks it, against the definition
bool check_call(int32_t rlen, int32_t min_depth, bool big, std::mt19937& rng)
{
    const uint32_t small[6] = {0u, 1u, 2u, 3u, 40u, 93u}, large[6] = {0u, 1u, 2u, 93u, 0x80000000u, 0xFFFFFFFFu};
    const uint32_t* vals = big ? large : small;
    auto draw = [&]() { return vals[rng() % 6u]; };
    auto count = [&]() { return big && rng() % 4u == 0 ? 0xFFFFFFFFu : uint32_t(rng() % 4u); };
    std::vector<ioc_pileup_col> cols(size_t(rlen) + 1u, ioc_pileup_col{}), wcols(size_t(rlen) + 1u, ioc_pileup_col{});
    std::vector<ioc_pileup_ins> wins(size_t(rlen) + 1u, ioc_pileup_ins{});
    for (auto& c : cols) c = rng() % 5u ? ioc_pileup_col{count(), count(), count(), count(), count(), count(), count(), count()} : ioc_pileup_col{};
    for (auto& c : wcols) c = rng() % 7u ? ioc_pileup_col{draw(), draw(), draw(), draw(), draw(), draw(), draw(), draw()} : ioc_pileup_col{};
    for (auto& x : wins) {
        const uint32_t used = rng() % 8u;  // (slots in use: the later ones stay empty in most rows)
        for (uint32_t s = 0; s < uint32_t(IOC_PILE_INS_SLOTS) && s < used; ++s)
            for (uint32_t ch = 0; ch < 5u; ++ch) x.slot[s][ch] = draw();
        x.longer = draw();
    }
    std::string frame(size_t(rlen), 'A');
    for (char& ch : frame) ch = "ACGTACGTACGTNacR"[rng() % 16u];
    const int64_t cap = int64_t(rlen) + IOC_PILE_INS_SLOTS * (int64_t(rlen) + 1);
    std::vector<char> want_s(size_t(cap), 0), want_q(size_t(cap), 0);
    ioc_polish_stats want{};
    const int64_t n = ioc_host_pileup_call_weighted(cols.data(), wcols.data(), wins.data(), frame.data(), rlen, min_depth, want_s.data(),
                                                    want_q.data(), cap, &want);
    if (n < 0 || n > cap || n != want.out_len) {
        fprintf(stderr, "the definition returned %lld for rlen %d\n", (long long)n, rlen);
        return false;
    }
    std::string got_s, got_q;
    ioc_polish_stats got{};
    for (int32_t p = 0; p <= rlen; ++p) {  // (as `decide` of ioc_pile_call.hip puts the row's arguments together)
        const bool has_base = p < rlen;
        const size_t at = size_t(p);
        const unsigned long long d_ins = has_base ? pile_depth(wcols[at]) : rlen > 0 ? pile_depth(wcols[at - 1u]) : 0ull;
        const unsigned long long c_ins = has_base ? pile_depth(cols[at]) : rlen > 0 ? pile_depth(cols[at - 1u]) : 0ull;
        const PileRowCall r = pile_call_row(wcols[at], wins[at], d_ins, has_base, has_base ? uint8_t(frame[at]) : uint8_t(0), min_depth, c_ins,
                                            has_base ? pile_depth(cols[at]) : 0ull);
        if (r.n > PILE_CALL_MAX_ROW) return false;
        for (uint32_t x = 0; x < r.n; ++x) got_s += char(r.seq >> (8u * x)), got_q += char(r.qual >> (8u * x));
        got.n_ins += int32_t(r.n_ins), got.n_sub += int32_t(r.n_sub), got.n_del += int32_t(r.n_del), got.n_low += int32_t(r.n_low);
    }
    got.out_len = int32_t(got_s.size());
    ++g_tables;
    if (int64_t(got_s.size()) != n || memcmp(got_s.data(), want_s.data(), size_t(n)) != 0 || memcmp(got_q.data(), want_q.data(), size_t(n)) != 0 ||
        memcmp(&got, &want, sizeof got) != 0) {
        fprintf(stderr, "call mismatch: rlen %d, min_depth %d\n", rlen, min_depth);
        return false;
    }
    for (char qv : got_q)
        if (qv < 33 || qv > 73) return false;
    return true;
}

}  // namespace

int main()
{
    static_assert(sizeof(ioc_pileup_ins) == INS_WORDS * 4 && INS_WORDS == 32, "record layout");
    std::mt19937 rng(8765);
    bool ok = true;
    for (int b = 0; b < 256; ++b) {
        const uint32_t w = b <= 34 ? 1u : b - 33 < 93 ? uint32_t(b - 33) : 93u;
        ok = ok && ioc_host_qual_weight(uint8_t(b)) == w && pile_qual_weight(uint8_t(b)) == w;
    }
    // 'D' in front of the first query base, behind the last one, with no query at all; free end gaps around it
    for (const char* s : {"", "D", "DD", "D=", "=D", "DD==", "==DD", "=D=", "dD=", "=Dd", "iD=", "=Di", "iDi", "dDd", "=ID=", "=DI=", "D=D", "IDI",
                          "iiII==DDdd", "=IDIDID=", "=IIDDDIIII=", "ddii=X=iidd", "IIIIIIII", "=IIIIIIIID="})
        ok = ok && check(s, rng);
    // a 'D' (alone, and a run of three) at every phase of a step — with the four heads the first and the last byte of a step at
    // every offset — between bases, and as the string's very first and very last byte
    for (uint32_t p = 0; p < 140u && ok; ++p)
        for (uint32_t G : {1u, 3u}) {
            ok = ok && check(std::string(p, '=') + std::string(G, 'D') + std::string(70u, '='), rng);
            ok = ok && check(std::string(G, 'D') + std::string(p, '='), rng) && check(std::string(p, '=') + std::string(G, 'D'), rng);
            ok = ok && check(std::string(p, 'i') + std::string(G, 'D') + std::string(5u, '='), rng);   // (q > 0 though no base was taken)
            ok = ok && check(std::string(p, 'd') + std::string(G, 'D') + std::string(5u, 'X'), rng);   // (q == 0 far into the string)
        }
    // one run of G 'I's at every phase of a step: across every step boundary at every offset; a 'D' directly behind it
    for (uint32_t G : {1u, 2u, 6u, 7u, 8u, 63u, 64u, 65u, 130u, 300u})
        for (uint32_t p = 0; p < 80u && ok; ++p)
            ok = ok && check(std::string(40u + p, '=') + std::string(G, 'I') + std::string(70u, '='), rng) &&
                 check(std::string(p, '=') + std::string(G, 'I') + "D" + std::string(G, 'I'), rng);
    // random strings over the six bytes, short runs and long ones
    for (int t = 0; t < 4000 && ok; ++t) {
        std::string s;
        const uint32_t runs = rng() % 60u;
        for (uint32_t x = 0; x < runs; ++x) {
            const uint32_t n = (rng() % 4u == 0) ? 1u + rng() % 150u : 1u + rng() % 8u;
            s.append(n, "=XIDidDI"[rng() % 8u]);
        }
        ok = check(s, rng);
    }
    if (!ok) return 1;
    if (!g_del_first || !g_del_last || !g_del_q0 || !g_del_qn) {
        fprintf(stderr, "a case the check is for did not occur\n");
        return 1;
    }
    for (int32_t rlen : {0, 1, 2, 63, 64, 65, 300})
        for (int32_t md : {1, 3})
            for (int big = 0; big < 2; ++big)
                for (int t = 0; t < 40 && ok; ++t) ok = check_call(rlen, md, big != 0, rng);
    if (!ok) return 1;
    printf("ok: %ld weighted tables agree with ioc_host_ops_pileup_weighted ('D' on a step's first byte %ld times, on its last %ld, in front of "
           "the first query base %ld, behind the last %ld), %ld calls with ioc_host_pileup_call_weighted\n",
           g_strings, g_del_first, g_del_last, g_del_q0, g_del_qn, g_tables);
    return 0;
}
