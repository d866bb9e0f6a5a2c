// pileup_acc_check.cpp — PileAcc (isonclust2_amd/csrc/ioc_ops_pileup.h), the step logic of k_ops_pileup, driven on the CPU as the
// kernel drives it (64-byte steps over the dwords from the aligned-down address, bytes outside the string masked to 0, one "lane"
// per byte) and compared row for row with the definition, ioc_host_ops_pileup, on random strings and on strings shaped like an
// aligner's (long runs of '=', gaps of every length around the step sizes, end gaps).  Host code only; meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/pileup_acc_check tools/pileup_acc_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/pileup_acc_check
//
// Exit status 0 and "ok" when every table agrees.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ioc_ops_pileup.h"
#include "isonclust2_hip.h"

namespace {

// the kernel's loop over one string that stands `head` bytes behind a dword boundary; rows past rlen or bases past qlen are counted
// as faults (the kernel drops them)
int drive(const std::string& ops, const std::string& query, uint32_t rlen, uint32_t head, std::vector<ioc_pileup_col>& cols)
{
    int faults = 0;
    const uint32_t span = head + uint32_t(ops.size());
    const uint32_t nsteps = (((span + 3u) / 4u + 63u) / 64u) * 4u;  // (whole chunks of 64 dwords, four steps each)
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
            const uint32_t row = acc.row(l);
            if (row > rlen) {
                faults += acc.is_base(l) || acc.is_del(l) || acc.ins_piece(l);
                continue;
            }
            uint32_t* rec = reinterpret_cast<uint32_t*>(&cols[row]);
            if (acc.is_base(l)) {
                if (acc.qpos(l) < query.size())
                    rec[PileAcc::channel(uint8_t(query[acc.qpos(l)]))] += 1u;
                else
                    ++faults;
            } else if (acc.is_del(l)) {
                rec[PILE_DEL] += 1u;
            } else if (const uint32_t piece = acc.ins_piece(l)) {
                rec[PILE_INS_BASES] += piece;
                if (acc.run_start(l)) rec[PILE_INS_RUNS] += 1u;
            }
        }
        acc.end();
    }
    return faults;
}

long g_cases = 0;

bool check(const std::string& ops, std::mt19937& rng)
{
    uint32_t qlen = 0, rlen = 0;
    for (char b : ops) {
        qlen += b == '=' || b == 'X' || b == 'I' || b == 'i';
        rlen += b == '=' || b == 'X' || b == 'D' || b == 'd';
    }
    std::string query(qlen, 'A');
    for (char& ch : query) ch = "ACGTACGTACGTNacR"[rng() % 16u];
    std::vector<ioc_pileup_col> want(rlen + 1u, ioc_pileup_col{});
    if (ioc_host_ops_pileup(ops.data(), int64_t(ops.size()), query.data(), int32_t(qlen), int32_t(rlen), want.data()) != IOC_OK) {
        fprintf(stderr, "the definition refused a string of %zu bytes\n", ops.size());
        return false;
    }
    for (uint32_t head = 0; head < 4u; ++head) {
        std::vector<ioc_pileup_col> got(rlen + 1u, ioc_pileup_col{});
        const int faults = drive(ops, query, rlen, head, got);
        ++g_cases;
        if (faults || memcmp(got.data(), want.data(), want.size() * sizeof(ioc_pileup_col)) != 0) {
            fprintf(stderr, "mismatch: %zu bytes, head %u, %d faults: %.120s\n", ops.size(), head, faults, ops.c_str());
            return false;
        }
    }
    return true;
}

}  // namespace

int main()
{
    static_assert(sizeof(ioc_pileup_col) == PILE_WORDS * 4, "record layout");
    std::mt19937 rng(12345);
    bool ok = true;
    // hand-written: every rule once, runs across the step boundary, all of one byte
    for (const char* s : {"", "I", "D", "=", "iiII==DDdd", "=IDIDID=", "=IIDDDIIII=", "ddii=X=iidd", "==II", "IIII", "dddd"}) ok = ok && check(s, rng);
    for (uint32_t n : {63u, 64u, 65u, 127u, 128u, 129u, 255u, 256u, 257u, 1000u})
        for (char b : {'=', 'I', 'D', 'i', 'd', 'X'}) ok = ok && check(std::string(n, b), rng);
    // one gap of G bytes at every phase of a step
    for (uint32_t G : {1u, 2u, 63u, 64u, 65u, 130u, 200u})
        for (uint32_t p = 0; p < 80u && ok; ++p)
            for (char g : {'I', 'D'}) ok = ok && check(std::string(40u + p, '=') + std::string(G, g) + std::string(70u, '='), rng);
    // random strings over the six bytes, short runs and long ones
    for (int t = 0; t < 4000 && ok; ++t) {
        std::string s;
        const uint32_t runs = rng() % 60u;
        for (uint32_t x = 0; x < runs; ++x) {
            const uint32_t n = (rng() % 4u == 0) ? 1u + rng() % 150u : 1u + rng() % 4u;
            s.append(n, "=XIDid=="[rng() % 8u]);
        }
        ok = check(s, rng);
    }
    // aligner-shaped: end gaps, a walk of '=' with sparse 'X' and short gaps
    for (int t = 0; t < 1000 && ok; ++t) {
        std::string s(rng() % 300u, rng() % 2u ? 'i' : 'd');
        const uint32_t cols = 1u + rng() % 1500u;
        for (uint32_t x = 0; x < cols; ++x) {
            const uint32_t u = rng() % 100u;
            if (u < 88u)
                s += '=';
            else if (u < 94u)
                s += 'X';
            else
                s.append(1u + rng() % 5u, u < 97u ? 'I' : 'D');
        }
        if (s.back() == 'I' || s.back() == 'D') s += '=';
        s.append(rng() % 300u, rng() % 2u ? 'i' : 'd');
        ok = check(s, rng);
    }
    if (!ok) return 1;
    printf("ok: %ld tables agree with ioc_host_ops_pileup\n", g_cases);
    return 0;
}
