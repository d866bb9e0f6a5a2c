// iso_correct_check.cpp — k_iso_correct_count and k_iso_correct_emit (isonclust2_amd/csrc/ioc_iso_correct.hip), restated lane by
// lane on the CPU and compared with the definition, ioc_host_read_correct_long (ioc_align.cpp):
//
//  * the chunk loop with its three-mask window, as tools/read_correct_check.cpp restates it for k_read_correct, over the tables of
//    the group-segment a per-pair table index names;
//  * the count pass — a pair's length, its record, and the OR of what makes it unresolved —, the scan over the pairs, and the write
//    pass: a lane's length is up to 254 + 1, the long runs of a chunk are copied run after run by all 64 lanes, a lane per byte,
//    and every lane then writes its row's own bytes behind its run.  The output buffers are blocks of exactly the counted size,
//    every byte must have exactly one writer, and an unresolved pair must have none;
//  * the bounds: tables, planes, frames and the pool are handed over in blocks of exactly their size and read with .at(); segments
//    of 0, 1, 63, 64, 65, 127, 128, 129 and 300 bases, several group-segments a segment, both frame directions;
//  * long rows of 7, 8 and 254 bases planted at rows 0, 63, 64 and rlen and two in one chunk, and among random pairs the plane's
//    cap, runs that leave the read, runs that together exceed it, long rows on rows that are not spanned, reads outside the pool.
//
// Host code only; meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/iso_correct_check tools/iso_correct_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/iso_correct_check
//
// Exit status 0 and "ok" when everything agrees.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ioc_iso_correct.h"
#include "ioc_sink_plan.h"
#include "isonclust2_hip.h"

namespace {

constexpr uint32_t SLOTS = IOC_PILE_INS_SLOTS;
long n_unresolved = 0, n_long_runs = 0, n_resolved_long = 0;

uint8_t comp_base(uint8_t ch) { return ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : ch; }

struct Call {  // what the kernels are launched over (IocIsoCorrectDev), every block exactly as large as it says
    std::vector<IocPileSeg> gsegs;
    uint32_t n_group_tables = 0;
    std::vector<uint32_t> table;
    std::vector<uint64_t> plane;
    std::vector<ioc_pileup_col> cols;
    std::vector<ioc_pileup_ins> ins;
    std::vector<uint8_t> frames, base_planes, slot_planes, ilen_planes, pool;  // (slot planes: SLOTS blocks of plane_bytes, one behind the other)
    std::vector<uint32_t> qpos_planes, q_len;
    std::vector<uint64_t> q_off;
    uint64_t plane_bytes = 0;
};

// IsoPairView of the kernels (ReadPairView's inside, decide and row_as, with .at() on every read)
struct View {
    const Call& k;
    IocPileSeg s;
    uint64_t po, q0;
    uint32_t qlen;
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
    IsoRowOut row(uint32_t p, uint32_t decision, bool guarded, const ReadRule& r) const
    {
        const uint32_t rlen = uint32_t(s.rlen);
        if (p > rlen || !inside(p)) return IsoRowOut{};
        const uint64_t rr = uint64_t(s.row0) + p, at = po + p;
        const bool has_base = p < rlen;
        const unsigned long long D = has_base ? pile_depth(k.cols.at(rr)) : rlen > 0u ? pile_depth(k.cols.at(rr - 1u)) : 0ull;
        const uint8_t own = k.base_planes.at(at);
        const uint8_t span = has_base ? own : rlen > 0u ? k.base_planes.at(at - 1u) : uint8_t(IOC_ALLELE_NONE);
        unsigned long long slots = 0;
        for (uint32_t j = 0; j < SLOTS; ++j) slots |= (unsigned long long)k.slot_planes.at(uint64_t(j) * k.plane_bytes + at) << (8u * j);
        return iso_correct_row(k.cols.at(rr), k.ins.at(rr), D, read_covers(span), own, slots, k.ilen_planes.at(at), k.qpos_planes.at(at), qlen, decision, guarded, r);
    }
};

// one wave of k_iso_correct_count (emit false: returns the record, out_len the pair's length) or of k_iso_correct_emit (writes
// from `carry` on and counts the writers of every byte) over pair i
ioc_iso_correct_stats wave(const Call& k, uint32_t i, const ReadRule& rule, bool emit, unsigned long long carry, std::vector<uint8_t>& seq,
                           std::vector<uint8_t>& qual, std::vector<uint8_t>& writers)
{
    const uint32_t tab = k.table.at(i);
    const uint64_t q0 = k.q_off.at(i);
    const uint32_t ql = k.q_len.at(i);
    const View v{k, k.gsegs.at(tab), k.plane.at(i), q0, q0 <= k.pool.size() && ql <= k.pool.size() - q0 ? ql : 0u};
    const uint32_t rows = uint32_t(v.s.rlen) + 1u, nchunks = (rows + 63u) / 64u;
    ioc_iso_correct_stats st{};
    unsigned long long n = 0, bases = 0;
    bool unresolved = false;
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
        IsoRowOut r[64];
        uint32_t before[64], all = 0;  // (the wave scan: a lane's offset in the chunk is the sum over the lanes below it)
        for (uint32_t l = 0; l < 64u; ++l) {
            const uint32_t kind = read_kind(dec[l]);
            const bool guarded = kind == READ_FILL     ? read_run_exceeds(fill_prev, fill_cur, fill_next, l, rule.max_run)
                                 : kind == READ_REMOVE ? read_run_exceeds(rem_prev, rem_cur, rem_next, l, rule.max_run)
                                                       : false;
            r[l] = v.row(c * 64u + l, dec[l], guarded, rule);
            before[l] = all, all += r[l].bytes();
        }
        if (!emit) {
            for (uint32_t l = 0; l < 64u; ++l) {
                n += r[l].row.n, bases += r[l].long_len, unresolved = unresolved || r[l].unresolved;
                st.n_sub += int32_t(r[l].row.n_sub), st.n_fill += int32_t(r[l].row.n_fill), st.n_remove += int32_t(r[l].row.n_remove);
                st.n_ins_add += int32_t(r[l].row.n_ins_add), st.n_ins_drop += int32_t(r[l].row.n_ins_drop), st.n_low += int32_t(r[l].row.n_low);
                st.n_guarded += int32_t(r[l].row.n_guarded), st.n_long_runs += r[l].long_len > 0u;
            }
        } else {
            for (uint32_t src = 0; src < 64u; ++src) {  // the ballot of the long-row lanes, run after run; 64 lanes, a byte each, step after step
                if (r[src].long_len == 0u) continue;
                const unsigned long long to = carry + before[src];
                for (uint32_t lane = 0; lane < 64u; ++lane)
                    for (uint32_t x = lane; x < r[src].long_len; x += 64u) {
                        const uint64_t q = v.q0 + r[src].long_from + x;
                        if (to + x < seq.size() && q < k.pool.size()) {
                            seq.at(size_t(to + x)) = k.pool.at(size_t(q)), qual.at(size_t(to + x)) = uint8_t('!');
                            ++writers.at(size_t(to + x));
                        }
                    }
            }
            for (uint32_t l = 0; l < 64u; ++l) {
                unsigned long long at = carry + before[l] + r[l].long_len;
                for (uint32_t x = 0; x < r[l].row.n; ++x, ++at)
                    if (at < seq.size()) {
                        seq.at(size_t(at)) = uint8_t(r[l].row.seq >> (8u * x)), qual.at(size_t(at)) = uint8_t(r[l].row.qual >> (8u * x));
                        ++writers.at(size_t(at));
                    }
            }
        }
        carry += all;
        fill_prev = fill_cur, rem_prev = rem_cur, fill_cur = fill_next, rem_cur = rem_next;
        memcpy(dec, dec_next, sizeof dec);
    }
    if (emit) return st;
    const int32_t table = iso_table_name(tab, k.n_group_tables);
    if (unresolved || bases > v.qlen) {
        st = ioc_iso_correct_stats{};
        st.flags = IOC_ISOC_UNRESOLVED;
    } else {
        st.out_len = int32_t(n + bases), st.n_long_bases = int32_t(bases);
    }
    st.table = table;
    return st;
}

int check_call(std::mt19937_64& rng, const ReadRule& rule, bool planted)
{
    int faults = 0;
    const int32_t lens[] = {0, 1, 63, 64, 65, 127, 128, 129, 300};
    Call k;
    // two or three group-segments a segment (its groups', then its own), each with rows of its own
    int64_t n_rows = 0, f_at = 0;
    std::vector<std::vector<uint32_t>> tables_of(sizeof lens / sizeof *lens);
    std::vector<IocPileSeg> own;
    for (size_t g = 0; g < tables_of.size(); ++g) {
        const int32_t rc = int32_t(rng() % 2);
        for (uint32_t h = 0, n = uint32_t(rng() % 3); h < n; ++h) {
            tables_of[g].push_back(uint32_t(k.gsegs.size()));
            k.gsegs.push_back(IocPileSeg{n_rows, f_at, lens[g], rc});
            n_rows += lens[g] + 1;
        }
        own.push_back(IocPileSeg{0, f_at, lens[g], rc});
        f_at += lens[g];
    }
    k.n_group_tables = uint32_t(k.gsegs.size());
    for (size_t g = 0; g < own.size(); ++g) {
        tables_of[g].push_back(uint32_t(k.gsegs.size()));
        own[g].row0 = n_rows, n_rows += own[g].rlen + 1;
        k.gsegs.push_back(own[g]);
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
    for (const IocPileSeg& s : k.gsegs)  // a stretch of one table row in some: runs of "fill" and of "remove" across the chunks
        if (s.rlen > 0 && rng() % 2) {
            const int32_t a = int32_t(rng() % uint32_t(s.rlen)), e = std::min<int32_t>(a + 5 + int32_t(rng() % 146), s.rlen);
            const bool fill = rng() % 2;
            for (int32_t p = a; p < e; ++p) {
                ioc_pileup_col& c = k.cols[size_t(s.row0 + p)];
                c = ioc_pileup_col{};
                c.a = fill ? 9u : 1u, c.del = fill ? 0u : 9u;
            }
        }
    std::vector<size_t> seg_of_pair;
    for (size_t g = 0; g < own.size(); ++g)
        for (uint32_t x = 0, n = uint32_t(rng() % 4); x < n; ++x) seg_of_pair.push_back(g);
    for (size_t x = seg_of_pair.size(); x > 1; --x) std::swap(seg_of_pair[x - 1], seg_of_pair[rng() % x]);  // (the segments' pairs interleaved)
    const size_t np = seg_of_pair.size();
    for (size_t g : seg_of_pair) {
        k.table.push_back(tables_of[g][rng() % tables_of[g].size()]);
        k.plane.push_back(k.plane_bytes), k.plane_bytes += uint64_t(own[g].rlen) + 1u;
    }
    k.base_planes.assign(size_t(k.plane_bytes), uint8_t(IOC_ALLELE_NONE)), k.slot_planes.assign(size_t(SLOTS * k.plane_bytes), 0);
    k.ilen_planes.assign(size_t(k.plane_bytes), 0), k.qpos_planes.assign(size_t(k.plane_bytes), 0);
    for (size_t i = 0; i < np; ++i) {
        const IocPileSeg& s = own[seg_of_pair[i]];
        uint8_t* b = k.base_planes.data() + k.plane[i];
        for (int32_t p = 0; p < s.rlen;) {  // pieces of 1 to 140 rows: not covered (seldom), deleted, one base, random bases
            const int32_t n = int32_t(rng() % 8 ? rng() % 12 + 1 : rng() % 140 + 1), what = int32_t(rng() % 9);
            const uint8_t one = uint8_t(rng() % 5);
            for (int32_t x = p; x < p + n && x < s.rlen; ++x)
                b[x] = what == 0 ? uint8_t(IOC_ALLELE_NONE) : what <= 2 ? uint8_t(IOC_ALLELE_DEL) : what <= 4 ? one : uint8_t(rng() % 5);
            p += n;
        }
        // the read: as many bytes as its rows and its runs need, in the pool behind the reads before it (a few lie outside it)
        const uint32_t qlen = uint32_t(s.rlen) + uint32_t(rng() % 600);
        k.q_off.push_back(rng() % 40 == 0 ? k.pool.size() + 5 : k.pool.size()), k.q_len.push_back(qlen);
        for (uint32_t x = 0; x < qlen; ++x) k.pool.push_back(uint8_t("ACGTN"[rng() % 5]));
        uint32_t q = 0;
        for (int32_t p = 0; p <= s.rlen; ++p) {
            const uint64_t at = k.plane[i] + uint64_t(p);
            if (rng() % 300 == 0) b[p] = uint8_t(rng() % 256);  // (bytes no projection writes)
            for (uint32_t j = 0; j < SLOTS; ++j)
                if (rng() % 3 == 0) k.slot_planes[size_t(j * k.plane_bytes + at)] = uint8_t(rng() % 40 == 0 ? rng() % 256 : rng() % 6);
            uint32_t len = rng() % 4 ? 0u : uint32_t(rng() % 7);
            if (planted) {
                const int32_t at_rows[] = {0, 63, 64, s.rlen, 70, 75};
                const uint32_t of[] = {7, 8, 254, 254, 8, 7};
                for (int x = 0; x < 6; ++x)
                    if (p == at_rows[x] && rng() % 3 == 0) len = of[x];
            } else if (rng() % 40 == 0) {
                len = 7u + uint32_t(rng() % 248);
            }
            if (rng() % 3000 == 0) len = 255u;  // (the plane's cap)
            k.ilen_planes[size_t(at)] = uint8_t(len);
            k.qpos_planes[size_t(at)] = rng() % 500 == 0 ? uint32_t(rng()) : q;  // (now and then a word of another read's plane)
            q += len + (p < s.rlen && b[p] <= 4);
        }
    }

    // the count pass, the scan, the write pass
    std::vector<ioc_iso_correct_stats> recs(np);
    std::vector<unsigned long long> off(np + 1, 0);
    std::vector<uint8_t> none;
    for (size_t i = 0; i < np; ++i) recs[i] = wave(k, uint32_t(i), rule, false, 0, none, none, none), off[i + 1] = off[i] + uint64_t(recs[i].out_len);
    const size_t total = size_t(off[np]);
    std::vector<uint8_t> seq(total, 0xEE), qual(total, 0xEE), writers(total, 0);
    for (size_t i = 0; i < np; ++i)
        if (recs[i].out_len > 0) wave(k, uint32_t(i), rule, true, off[i], seq, qual, writers);  // (the write pass leaves a pair of length 0 at once)
    for (uint8_t w : writers) faults += w != 1;

    // the definition, pair by pair, over the rows of the pair's table
    for (size_t i = 0; i < np; ++i) {
        const IocPileSeg& s = k.gsegs[k.table[i]];
        const size_t rows = size_t(s.rlen) + 1;
        std::string frame(size_t(s.rlen), 'A');
        for (int32_t p = 0; p < s.rlen; ++p)
            frame[size_t(p)] = char(s.rc ? comp_base(k.frames[size_t(s.f_off + s.rlen - 1 - p)]) : k.frames[size_t(s.f_off + p)]);
        const auto from = [&](const auto& plane, size_t at) { return std::vector<typename std::decay<decltype(plane[0])>::type>(plane.begin() + int64_t(at), plane.begin() + int64_t(at + rows)); };
        const std::vector<uint8_t> base = from(k.base_planes, size_t(k.plane[i])), ilen = from(k.ilen_planes, size_t(k.plane[i]));
        const std::vector<uint32_t> qpos = from(k.qpos_planes, size_t(k.plane[i]));
        std::vector<uint8_t> slots(SLOTS * rows);
        for (uint32_t j = 0; j < SLOTS; ++j) memcpy(slots.data() + j * rows, k.slot_planes.data() + j * k.plane_bytes + k.plane[i], rows);
        const std::vector<ioc_pileup_col> cols(k.cols.begin() + s.row0, k.cols.begin() + s.row0 + int64_t(rows));
        const std::vector<ioc_pileup_ins> ins(k.ins.begin() + s.row0, k.ins.begin() + s.row0 + int64_t(rows));
        const bool in_pool = k.q_off[i] + k.q_len[i] <= k.pool.size();  // (a read outside the pool: the kernels take it as empty)
        const std::vector<char> query(k.pool.begin() + int64_t(in_pool ? k.q_off[i] : 0), k.pool.begin() + int64_t(in_pool ? k.q_off[i] + k.q_len[i] : 0));
        const int64_t cap = pile_call_most(s.rlen) + int64_t(query.size());
        std::vector<char> want_seq(size_t(cap) + 1), want_qual(size_t(cap) + 1);
        ioc_iso_correct_stats want{};
        const char nothing = 0;
        const int64_t n = ioc_host_read_correct_long(base.data(), slots.data(), ilen.data(), qpos.data(), s.rlen, cols.data(), ins.data(), frame.data(),
                                                     query.empty() ? &nothing : query.data(), int32_t(query.size()), rule.min_depth, rule.min_alt, rule.min_pct,
                                                     rule.max_run, want_seq.data(), want_qual.data(), cap, &want);
        want.table = iso_table_name(k.table[i], k.n_group_tables);
        bool same = n == int64_t(recs[i].out_len) && memcmp(&want, &recs[i], sizeof want) == 0;
        same = same && (n <= 0 || (memcmp(want_seq.data(), seq.data() + off[i], size_t(n)) == 0 && memcmp(want_qual.data(), qual.data() + off[i], size_t(n)) == 0));
        if (!same && ++faults < 5)
            fprintf(stderr, "pair %zu of a segment of %d bases (rc %d), max_run %d: differs from the definition (%lld / %d bytes, flags %d / %d)\n", i, s.rlen, s.rc,
                    rule.max_run, (long long)n, recs[i].out_len, want.flags, recs[i].flags);
        n_unresolved += recs[i].flags != 0, n_long_runs += recs[i].n_long_runs, n_resolved_long += recs[i].flags == 0 && recs[i].n_long_runs > 0;
    }
    return faults;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20261021);
    int faults = 0;
    long calls = 0;
    for (int t = 0; t < 160; ++t) {
        const int32_t runs[] = {0, 1, 3, 10, 63, 64};
        const ReadRule rule{int32_t(rng() % 4 + 1), int32_t(rng() % 4 + 1), int32_t(rng() % 50 + 1), runs[t % 6]};
        faults += check_call(rng, rule, t % 2 == 0);
        ++calls;
    }
    if (n_unresolved == 0 || n_resolved_long == 0) fprintf(stderr, "no unresolved pair, or no resolved pair with a long row, in any call\n"), ++faults;
    if (faults) {
        fprintf(stderr, "%d faults\n", faults);
        return 1;
    }
    printf("ok (%ld calls, %ld long runs carried through, %ld pairs with long rows resolved, %ld pairs unresolved)\n", calls, n_long_runs, n_resolved_long, n_unresolved);
    return 0;
}
