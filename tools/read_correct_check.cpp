// read_correct_check.cpp — the chunk loop of k_read_correct (isonclust2_amd/csrc/ioc_read_correct.hip), restated lane by lane on
// the CPU and compared with the definition, ioc_host_read_correct (ioc_align.cpp):
//
//  * the three-mask window — a wave walks a pair's rlen + 1 rows in chunks of 64, decides chunk c + 1 while it finishes chunk c,
//    and holds the "fill" and the "remove" masks of the chunks c - 1, c and c + 1 for read_run_exceeds (ioc_read_correct.h);
//  * the count pass (a pair's length and record), the scan over the pairs, and the write pass with its running carry: the output
//    buffers are blocks of exactly the counted size, and every byte must have exactly one writer;
//  * the bounds: tables, planes and frames are handed over in blocks of exactly their size, segments of 0, 1, 63, 64, 65, 127,
//    128, 129 and 300 bases, several pairs a segment, both frame directions;
//  * read_run_exceeds on its own, against a run measured end to end, for every lane, runs that start and end anywhere in three
//    chunks, and every max_run from 0 to 64.
// The inputs: random planes and tables with small counters (every branch of the rule is taken), with runs of deletions and of
// unsupported bases of 1 to 140 rows, and stretches of up to 150 uniform table rows under them, so that runs of one decision cross
// the chunk edges in the restated loop as well.
//
// Host code only; meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/read_correct_check tools/read_correct_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/read_correct_check
//
// Exit status 0 and "ok" when everything agrees.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ioc_read_correct.h"
#include "ioc_sink_plan.h"
#include "isonclust2_hip.h"

namespace {

constexpr uint32_t SLOTS = IOC_PILE_INS_SLOTS;
long guarded_at_64 = 0;  // rows the restated loop turned back at max_run 64: runs of more than a chunk were there

uint8_t comp_base(uint8_t ch) { return ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : ch; }

struct Call {  // what the kernel is launched over, every block exactly as large as it says
    std::vector<IocPileSeg> segs;
    std::vector<int32_t> seg_of_pair;
    std::vector<uint64_t> plane;
    std::vector<ioc_pileup_col> cols;
    std::vector<ioc_pileup_ins> ins;
    std::vector<uint8_t> frames, base_planes, slot_planes;  // (slot planes: SLOTS blocks of plane_bytes, one behind the other)
    uint64_t plane_bytes = 0;
};

// ReadPairView of the kernel (ioc_read_correct.h)
struct View {
    const Call& k;
    IocPileSeg s;
    uint64_t po;
    bool inside(uint32_t p) const
    {
        const uint32_t rlen = uint32_t(s.rlen);
        if (uint64_t(s.row0) + p >= k.cols.size() || po + p >= k.plane_bytes) return false;
        return p >= rlen || uint64_t(s.f_off) + (s.rc ? rlen - 1u - p : p) < k.frames.size();
    }
    uint32_t decide(uint32_t p, const ReadRule& r) const
    {
        const uint32_t rlen = uint32_t(s.rlen);
        if (p >= rlen || !inside(p)) return READ_NONE;
        const uint64_t at = uint64_t(s.f_off) + (s.rc ? rlen - 1u - p : p);
        const uint8_t fb = s.rc ? comp_base(k.frames.at(at)) : k.frames.at(at);
        return read_base_decide(k.cols.at(uint64_t(s.row0) + p), k.base_planes.at(po + p), fb, r);
    }
    ReadRowOut row(uint32_t p, uint32_t decision, bool guarded, const ReadRule& r) const
    {
        const uint32_t rlen = uint32_t(s.rlen);
        if (p > rlen || !inside(p)) return ReadRowOut{};
        const uint64_t rr = uint64_t(s.row0) + p, at = po + p;
        const bool has_base = p < rlen;
        const unsigned long long D = has_base ? pile_depth(k.cols.at(rr)) : rlen > 0u ? pile_depth(k.cols.at(rr - 1u)) : 0ull;
        const uint8_t own = k.base_planes.at(at);
        const uint8_t span = has_base ? own : rlen > 0u ? k.base_planes.at(at - 1u) : uint8_t(IOC_ALLELE_NONE);
        unsigned long long slots = 0;
        for (uint32_t j = 0; j < SLOTS; ++j) slots |= (unsigned long long)k.slot_planes.at(uint64_t(j) * k.plane_bytes + at) << (8u * j);
        return read_correct_row(k.cols.at(rr), k.ins.at(rr), D, read_covers(span), own, slots, decision, guarded, r);
    }
};

// one wave of k_read_correct<EMIT> over pair i: the count pass returns the record (out_len: the length), the write pass writes
// from `carry` on and counts the writers of every byte
ioc_correct_stats wave(const Call& k, uint32_t i, const ReadRule& rule, bool emit, unsigned long long carry, std::vector<uint8_t>& seq,
                       std::vector<uint8_t>& qual, std::vector<uint8_t>& writers)
{
    const View v{k, k.segs.at(size_t(k.seg_of_pair.at(i))), k.plane.at(i)};
    const uint32_t rows = uint32_t(v.s.rlen) + 1u, nchunks = (rows + 63u) / 64u;
    ioc_correct_stats st{};
    uint32_t dec[64], dec_next[64];
    auto ballot = [](const uint32_t* d, uint32_t kind) {
        unsigned long long m = 0;
        for (uint32_t l = 0; l < 64u; ++l)
            if (read_kind(d[l]) == kind) m |= 1ull << l;
        return m;
    };
    for (uint32_t l = 0; l < 64u; ++l) dec[l] = v.decide(l, rule);
    unsigned long long fill_prev = 0, rem_prev = 0, fill_cur = ballot(dec, READ_FILL), rem_cur = ballot(dec, READ_REMOVE);
    for (uint32_t c = 0; c < nchunks; ++c) {
        for (uint32_t l = 0; l < 64u; ++l) dec_next[l] = c + 1u < nchunks ? v.decide(c * 64u + l + 64u, rule) : uint32_t(READ_NONE);
        const unsigned long long fill_next = ballot(dec_next, READ_FILL), rem_next = ballot(dec_next, READ_REMOVE);
        uint32_t all = 0;  // (the wave scan: a lane's offset in the chunk is the sum over the lanes below it)
        for (uint32_t l = 0; l < 64u; ++l) {
            const uint32_t kind = read_kind(dec[l]);
            const bool guarded = kind == READ_FILL     ? read_run_exceeds(fill_prev, fill_cur, fill_next, l, rule.max_run)
                                 : kind == READ_REMOVE ? read_run_exceeds(rem_prev, rem_cur, rem_next, l, rule.max_run)
                                                       : false;
            const ReadRowOut r = v.row(c * 64u + l, dec[l], guarded, rule);
            if (!emit && rule.max_run == 64) guarded_at_64 += r.n_guarded;
            if (!emit) {
                st.out_len += int32_t(r.n), st.n_sub += int32_t(r.n_sub), st.n_fill += int32_t(r.n_fill), st.n_remove += int32_t(r.n_remove);
                st.n_ins_add += int32_t(r.n_ins_add), st.n_ins_drop += int32_t(r.n_ins_drop), st.n_low += int32_t(r.n_low), st.n_guarded += int32_t(r.n_guarded);
            } else {
                unsigned long long at = carry + all;
                for (uint32_t x = 0; x < r.n; ++x, ++at)
                    if (at < seq.size()) {
                        seq.at(at) = uint8_t(r.seq >> (8u * x)), qual.at(at) = uint8_t(r.qual >> (8u * x));
                        ++writers.at(at);
                    }
            }
            all += r.n;
        }
        carry += all;
        fill_prev = fill_cur, rem_prev = rem_cur, fill_cur = fill_next, rem_cur = rem_next;
        memcpy(dec, dec_next, sizeof dec);
    }
    return st;
}

// a run measured end to end, for the guard on its own
int check_guard(std::mt19937_64& rng)
{
    int faults = 0;
    for (int t = 0; t < 4000; ++t) {
        unsigned long long m[3];
        std::vector<uint8_t> bit(192, 0);
        const int shape = t % 4;
        if (shape == 0) {  // one run anywhere
            const uint32_t a = uint32_t(rng() % 192), b = a + uint32_t(rng() % (192 - a)) + 1u;
            for (uint32_t x = a; x < b; ++x) bit[x] = 1;
        } else {
            const unsigned thin = shape == 1 ? 2 : shape == 2 ? 8 : 40;  // (long runs with few gaps)
            for (auto& b : bit) b = rng() % thin != 0;
        }
        for (int w = 0; w < 3; ++w) {
            m[w] = 0;
            for (uint32_t l = 0; l < 64u; ++l) m[w] |= (unsigned long long)bit[size_t(w) * 64 + l] << l;
        }
        for (uint32_t l = 0; l < 64u; ++l) {
            if (!bit[64 + l]) continue;
            uint32_t a = 64 + l, b = 64 + l;
            while (a > 0 && bit[a - 1]) --a;
            while (b + 1 < 192 && bit[b + 1]) ++b;
            const uint32_t run = b - a + 1;  // (a run that touches either end of the window has at least 65 rows: too long at any max_run)
            for (int32_t max_run = 0; max_run <= 64; ++max_run)
                if (read_run_exceeds(m[0], m[1], m[2], l, max_run) != (run > uint32_t(max_run))) {
                    if (++faults < 5) fprintf(stderr, "guard: lane %u, run %u, max_run %d\n", l, run, max_run);
                }
        }
    }
    return faults;
}

int check_call(std::mt19937_64& rng, const ReadRule& rule)
{
    int faults = 0;
    const int32_t lens[] = {0, 1, 63, 64, 65, 127, 128, 129, 300};
    Call k;
    int64_t n_rows = 0, f_at = 0;
    for (int32_t rlen : lens) {
        k.segs.push_back(IocPileSeg{n_rows, f_at, rlen, int32_t(rng() % 2)});
        n_rows += rlen + 1, f_at += rlen;
    }
    const uint32_t small[] = {0, 0, 1, 2, 3, 5, 9, 20};
    k.cols.resize(size_t(n_rows)), k.ins.resize(size_t(n_rows)), k.frames.resize(size_t(f_at));
    for (auto& f : k.frames) f = uint8_t("ACGTN"[rng() % 5]);
    for (auto& c : k.cols) {
        uint32_t* w = reinterpret_cast<uint32_t*>(&c);
        for (int x = 0; x < 6; ++x) w[x] = small[rng() % 8];
    }
    for (auto& in : k.ins) {
        memset(&in, 0, sizeof in);
        for (uint32_t j = 0; j < SLOTS; ++j)
            for (uint32_t ch = 0; ch < 5u && rng() % 2; ++ch) in.slot[j][ch] = small[rng() % 8];
    }
    // stretches of one table row — the base 9 deep, or deleted by 9 of 10 — under which most pairs get one byte: runs of "fill" and of
    // "remove" of up to 150 rows, across the chunks of the loop below
    struct Stretch { int32_t a, e; bool fill; };
    std::vector<std::vector<Stretch>> stretches(k.segs.size());
    for (size_t g = 0; g < k.segs.size(); ++g)
        for (uint32_t x = 0, n = uint32_t(rng() % 3); x < n && k.segs[g].rlen > 0; ++x) {
            const int32_t a = int32_t(rng() % uint32_t(k.segs[g].rlen)), e = std::min<int32_t>(a + 5 + int32_t(rng() % 146), k.segs[g].rlen);
            const bool fill = rng() % 2;
            for (int32_t p = a; p < e; ++p) {
                ioc_pileup_col& c = k.cols[size_t(k.segs[g].row0 + p)];
                c = ioc_pileup_col{};
                c.a = fill ? 9u : 1u, c.del = fill ? 0u : 9u;
            }
            stretches[g].push_back(Stretch{a, e, fill});
        }
    for (size_t g = 0; g < k.segs.size(); ++g)
        for (uint32_t x = 0, n = uint32_t(rng() % 4); x < n; ++x) k.seg_of_pair.push_back(int32_t(g));
    for (size_t x = k.seg_of_pair.size(); x > 1; --x) std::swap(k.seg_of_pair[x - 1], k.seg_of_pair[rng() % x]);  // (the segments' pairs interleaved)
    for (int32_t g : k.seg_of_pair) k.plane.push_back(k.plane_bytes), k.plane_bytes += uint64_t(k.segs[size_t(g)].rlen) + 1u;
    k.base_planes.assign(size_t(k.plane_bytes), uint8_t(IOC_ALLELE_NONE)), k.slot_planes.assign(size_t(SLOTS * k.plane_bytes), 0);
    const size_t np = k.seg_of_pair.size();
    for (size_t i = 0; i < np; ++i) {
        const IocPileSeg& s = k.segs[size_t(k.seg_of_pair[i])];
        uint8_t* b = k.base_planes.data() + k.plane[i];
        for (int32_t p = 0; p < s.rlen;) {  // pieces of 1 to 140 rows: not covered, deleted, one base, random bases
            const int32_t n = int32_t(rng() % 8 ? rng() % 12 + 1 : rng() % 140 + 1), what = int32_t(rng() % 5);
            const uint8_t one = uint8_t(rng() % 5);
            for (int32_t x = p; x < p + n && x < s.rlen; ++x)
                b[x] = what == 0 ? uint8_t(IOC_ALLELE_NONE) : what == 1 ? uint8_t(IOC_ALLELE_DEL) : what == 2 ? one : uint8_t(rng() % 5);
            p += n;
        }
        for (const Stretch& t : stretches[size_t(k.seg_of_pair[i])])
            for (int32_t p = t.a; p < t.e && rng() % 64; ++p) b[p] = t.fill ? uint8_t(IOC_ALLELE_DEL) : uint8_t(0);  // (a few stop short)
        for (int32_t p = 0; p <= s.rlen; ++p) {
            if (rng() % 200 == 0) b[p] = uint8_t(rng() % 256);  // (bytes no projection writes)
            for (uint32_t j = 0; j < SLOTS; ++j)
                if (rng() % 3 == 0) k.slot_planes[size_t(j * k.plane_bytes + k.plane[i] + uint64_t(p))] = uint8_t(rng() % 40 == 0 ? rng() % 256 : rng() % 6);
        }
    }

    // the count pass, the scan, the write pass
    std::vector<ioc_correct_stats> recs(np);
    std::vector<unsigned long long> off(np + 1, 0);
    std::vector<uint8_t> none;
    for (size_t i = 0; i < np; ++i) recs[i] = wave(k, uint32_t(i), rule, false, 0, none, none, none), off[i + 1] = off[i] + uint64_t(recs[i].out_len);
    const size_t total = size_t(off[np]);
    std::vector<uint8_t> seq(total, 0xEE), qual(total, 0xEE), writers(total, 0);
    for (size_t i = 0; i < np; ++i) wave(k, uint32_t(i), rule, true, off[i], seq, qual, writers);
    for (uint8_t w : writers) faults += w != 1;

    // the definition, pair by pair
    for (size_t i = 0; i < np; ++i) {
        const IocPileSeg& s = k.segs[size_t(k.seg_of_pair[i])];
        const size_t rows = size_t(s.rlen) + 1;
        std::string frame(size_t(s.rlen), 'A');
        for (int32_t p = 0; p < s.rlen; ++p)
            frame[size_t(p)] = char(s.rc ? comp_base(k.frames[size_t(s.f_off + s.rlen - 1 - p)]) : k.frames[size_t(s.f_off + p)]);
        std::vector<uint8_t> base(k.base_planes.begin() + int64_t(k.plane[i]), k.base_planes.begin() + int64_t(k.plane[i] + rows)), slots(SLOTS * rows);
        for (uint32_t j = 0; j < SLOTS; ++j) memcpy(slots.data() + j * rows, k.slot_planes.data() + j * k.plane_bytes + k.plane[i], rows);
        const std::vector<ioc_pileup_col> cols(k.cols.begin() + s.row0, k.cols.begin() + s.row0 + int64_t(rows));
        const std::vector<ioc_pileup_ins> ins(k.ins.begin() + s.row0, k.ins.begin() + s.row0 + int64_t(rows));
        const int64_t cap = pile_call_most(s.rlen);
        std::vector<char> want_seq(size_t(cap) + 1), want_qual(size_t(cap) + 1);
        ioc_correct_stats want{};
        const int64_t n = ioc_host_read_correct(base.data(), slots.data(), s.rlen, cols.data(), ins.data(), frame.data(), rule.min_depth, rule.min_alt,
                                                rule.min_pct, rule.max_run, want_seq.data(), want_qual.data(), cap, &want);
        bool same = n == int64_t(recs[i].out_len) && memcmp(&want, &recs[i], sizeof want) == 0;
        same = same && (n <= 0 || (memcmp(want_seq.data(), seq.data() + off[i], size_t(n)) == 0 && memcmp(want_qual.data(), qual.data() + off[i], size_t(n)) == 0));
        if (!same && ++faults < 5) fprintf(stderr, "pair %zu of a segment of %d bases (rc %d), max_run %d: differs from the definition\n", i, s.rlen, s.rc, rule.max_run);
    }
    return faults;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20261019);
    int faults = check_guard(rng);
    long calls = 0;
    for (int t = 0; t < 120; ++t) {
        const int32_t runs[] = {0, 1, 3, 10, 63, 64};
        const ReadRule rule{int32_t(rng() % 4 + 1), int32_t(rng() % 4 + 1), int32_t(rng() % 50 + 1), runs[t % 6]};
        faults += check_call(rng, rule);
        ++calls;
    }
    if (guarded_at_64 == 0) fprintf(stderr, "no run of more than 64 rows in any call\n"), ++faults;
    if (faults) {
        fprintf(stderr, "%d faults\n", faults);
        return 1;
    }
    printf("ok (%ld calls, %ld rows guarded at max_run 64)\n", calls, guarded_at_64);
    return 0;
}
