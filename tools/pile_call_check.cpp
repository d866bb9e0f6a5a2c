// pile_call_check.cpp — the two pieces of host-callable step logic behind the polished consensus, driven on the CPU as their kernels
// drive them and compared with the definitions in ioc_align.cpp:
//
//  * PileAcc with ins_index / end_len (isonclust2_amd/csrc/ioc_ops_pileup.h), as the ins variant of k_ops_pileup uses it — 64-byte
//    steps from the aligned-down address at every head offset 0 .. 3, one "lane" per byte — against ioc_host_ops_pileup_ins, on
//    random strings and on strings whose runs of 'I' cross step boundaries at every offset (lengths 1 .. 7, 63 .. 65, 130, 300);
//  * pile_call_row (ioc_pile_call.h), as k_pile_call uses it — a lane per row, the emitted bytes packed behind each other in row
//    order — against ioc_host_pileup_call over random tables, counts up to 2^32 - 1 included.
//
// Host code only; meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/pile_call_check tools/pile_call_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/pile_call_check
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

// the ins variant's loop over one string that stands `head` bytes behind a dword boundary
int drive(const std::string& ops, const std::string& query, uint32_t rlen, uint32_t head, std::vector<ioc_pileup_ins>& ins)
{
    int faults = 0;
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
            if (!acc.is_ins(l)) continue;
            const uint32_t row = acc.row(l), at = acc.qpos(l), j = acc.ins_index(l);
            if (row > rlen || at >= query.size()) {
                ++faults;
                continue;
            }
            uint32_t* rec = reinterpret_cast<uint32_t*>(&ins[row]);
            rec[j < uint32_t(IOC_PILE_INS_SLOTS) ? j * 5u + PileAcc::channel(uint8_t(query[at])) : INS_LONGER] += 1u;
        }
        acc.end_len();
        acc.end();
        if (acc.open_i != (acc.open_len != 0u)) ++faults;  // (open_len carries what open_i says)
    }
    return faults;
}

long g_strings = 0, g_tables = 0;

bool check(const std::string& ops, std::mt19937& rng)
{
    uint32_t qlen = 0, rlen = 0;
    for (char b : ops) {
        qlen += b == '=' || b == 'X' || b == 'I' || b == 'i';
        rlen += b == '=' || b == 'X' || b == 'D' || b == 'd';
    }
    std::string query(qlen, 'A');
    for (char& ch : query) ch = "ACGTACGTACGTNacR"[rng() % 16u];
    std::vector<ioc_pileup_ins> want(rlen + 1u, ioc_pileup_ins{});
    if (ioc_host_ops_pileup_ins(ops.data(), int64_t(ops.size()), query.data(), int32_t(qlen), int32_t(rlen), want.data()) != IOC_OK) {
        fprintf(stderr, "the definition refused a string of %zu bytes\n", ops.size());
        return false;
    }
    for (uint32_t head = 0; head < 4u; ++head) {
        std::vector<ioc_pileup_ins> got(rlen + 1u, ioc_pileup_ins{});
        const int faults = drive(ops, query, rlen, head, got);
        ++g_strings;
        if (faults || memcmp(got.data(), want.data(), want.size() * sizeof(ioc_pileup_ins)) != 0) {
            fprintf(stderr, "mismatch: %zu bytes, head %u, %d faults: %.120s\n", ops.size(), head, faults, ops.c_str());
            return false;
        }
    }
    return true;
}

// one segment as k_pile_call walks it, against the definition
bool check_call(int32_t rlen, int32_t min_depth, bool big, std::mt19937& rng)
{
    const uint32_t small[6] = {0u, 1u, 2u, 3u, 4u, 5u}, large[6] = {0u, 1u, 2u, 3u, 0x80000000u, 0xFFFFFFFFu};
    const uint32_t* vals = big ? large : small;
    auto draw = [&]() { return vals[rng() % 6u]; };
    std::vector<ioc_pileup_col> cols(size_t(rlen) + 1u, ioc_pileup_col{});
    std::vector<ioc_pileup_ins> ins(size_t(rlen) + 1u, ioc_pileup_ins{});
    for (auto& c : cols) c = ioc_pileup_col{draw(), draw(), draw(), draw(), draw(), draw(), draw(), draw()};
    for (auto& x : ins) {
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
    const int64_t n = ioc_host_pileup_call(cols.data(), ins.data(), frame.data(), rlen, min_depth, want_s.data(), want_q.data(), cap, &want);
    if (n < 0 || n > cap || n != want.out_len) {
        fprintf(stderr, "the definition returned %lld for rlen %d\n", (long long)n, rlen);
        return false;
    }
    std::string got_s, got_q;
    ioc_polish_stats got{};
    for (int32_t p = 0; p <= rlen; ++p) {
        const bool has_base = p < rlen;
        const unsigned long long d_ins = has_base ? pile_depth(cols[size_t(p)]) : rlen > 0 ? pile_depth(cols[size_t(p) - 1u]) : 0ull;
        const PileRowCall r = pile_call_row(cols[size_t(p)], ins[size_t(p)], d_ins, has_base, has_base ? uint8_t(frame[size_t(p)]) : uint8_t(0), min_depth);
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
    std::mt19937 rng(4321);
    bool ok = true;
    for (const char* s : {"", "I", "D", "=", "iiII==DDdd", "=IDIDID=", "=IIDDDIIII=", "ddii=X=iidd", "==II", "IIII", "IIIIIII", "=IIIIIIID="}) ok = ok && check(s, rng);
    for (uint32_t n : {63u, 64u, 65u, 127u, 128u, 129u, 255u, 256u, 257u, 1000u}) ok = ok && check(std::string(n, 'I'), rng);
    // one run of G 'I's at every phase of a step (and so, with the four heads, across every step boundary at every offset)
    for (uint32_t G : {1u, 2u, 3u, 4u, 5u, 6u, 7u, 63u, 64u, 65u, 130u, 300u})
        for (uint32_t p = 0; p < 80u && ok; ++p) ok = ok && check(std::string(40u + p, '=') + std::string(G, 'I') + std::string(70u, '='), rng);
    // two runs with one byte between them: the second starts at index 0 again, also at a step's first byte
    for (uint32_t p = 0; p < 80u && ok; ++p)
        for (char mid : {'=', 'D', 'X'}) ok = ok && check(std::string(30u + p, '=') + std::string(9u, 'I') + mid + std::string(70u, 'I') + "=", rng);
    // random strings over the six bytes, short runs and long ones
    for (int t = 0; t < 4000 && ok; ++t) {
        std::string s;
        const uint32_t runs = rng() % 60u;
        for (uint32_t x = 0; x < runs; ++x) {
            const uint32_t n = (rng() % 4u == 0) ? 1u + rng() % 150u : 1u + rng() % 8u;
            s.append(n, "=XIDidII"[rng() % 8u]);
        }
        ok = check(s, rng);
    }
    if (!ok) return 1;
    for (int32_t rlen : {0, 1, 2, 63, 64, 65, 300})
        for (int32_t md : {1, 3})
            for (int big = 0; big < 2; ++big)
                for (int t = 0; t < 40 && ok; ++t) ok = check_call(rlen, md, big != 0, rng);
    if (!ok) return 1;
    printf("ok: %ld insertion tables agree with ioc_host_ops_pileup_ins, %ld calls with ioc_host_pileup_call\n", g_strings, g_tables);
    return 0;
}
