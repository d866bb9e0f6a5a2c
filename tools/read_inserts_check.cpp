// read_inserts_check.cpp — the step, chunk and word logic of the kernels of isonclust2_amd/csrc/ioc_read_inserts.hip, restated lane
// by lane on the CPU and compared with the definitions, ioc_host_ops_project_ilen and ioc_host_planes_inserts (ioc_align.cpp):
//
//  * k_ops_project_ilen: the walk with PileAcc (ioc_ops_pileup.h), 64 bytes a step behind a head of 0 .. 3 bytes; the lane of the byte
//    behind a run stores its length, lane 0 the run that ends with the last byte of the last chunk — runs of 1 .. 300, runs across
//    steps and chunks, runs beside 'i', strings that end in a run at every phase of a chunk;
//  * k_ins_bits: a chunk of 64 base bytes becomes a span word (covered AND covered-shifted-by-one, the bit carried from chunk to
//    chunk), and W comes from two prefix sums over 64 lanes, the chunk's bytes and a halo of 32 either side (window_sums), at chunk
//    starts that are multiples of 64 and, as k_ins_lens has them, any junction;
//  * k_ins_rows: span and in_ins bit by bit from the members' words, the variable word;
//  * k_ins_list: the k-th start and the k-th end of the runs of variable junctions, a run going on across a word by its
//    neighbour's edge bit and across a batch of 64 words by a carried bit and a word read ahead;
//  * k_ins_states, k_ins_lens: masked popcounts of the words a site spans, a carrier's largest W into its place of a table of 16-bit
//    entries, and the smallest and largest of a site's entries over the members 64 at a time;
//  * k_ins_support, k_ins_isoforms, k_ins_record: counts over the members with UNSIGNED compares of two-word keys, major word first.
// Every buffer is a block of exactly its size, and every plane byte, word, row and record counts its writers: one each.  The inputs:
// segments of 0, 1, 2, 63, 64, 65, 127, 128, 129, 600, 4200 and 9000 rows with 0 to 130 reads, length bytes of 1 .. 255 shared by
// groups of reads so that sites form, windows across 63 | 64 and 4095 | 4096, reads that stop early or start late, bytes no
// projection writes, 35 sites under max_sites 32, block words with bit 63 — under rules of slack 0, 8 and 32.
//
// Host code only; meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/read_inserts_check tools/read_inserts_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/read_inserts_check
//
// Exit status 0 and "ok" when everything agrees.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ioc_ops_pileup.h"
#include "ioc_read_inserts.h"
#include "isonclust2_hip.h"

namespace {

typedef unsigned long long u64;
int faults = 0;
long long runs_seen = 0, tail_runs = 0, sites_seen = 0, batches_crossed = 0, windows_seen = 0, hows_seen[4] = {0, 0, 0, 0}, states_seen[4] = {0, 0, 0, 0};

#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            if (++faults < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
        }                                                                   \
    } while (0)

// ---- k_ops_project_ilen ----
void project_ilen(const std::string& ops, uint32_t head, int32_t rlen)
{
    std::vector<uint8_t> want(size_t(rlen) + 1, 0xEE), got(size_t(rlen) + 1, 0);
    std::vector<int> writers(size_t(rlen) + 1, 0);
    EXPECT(ioc_host_ops_project_ilen(ops.data(), int64_t(ops.size()), rlen, want.data()) == IOC_OK);
    const uint32_t span = head + uint32_t(ops.size()), nwords = (span + 3u) / 4u, nchunks = (nwords + 63u) / 64u;
    PileAcc acc;
    for (uint32_t c = 0; c < nchunks; ++c)
        for (uint32_t j = 0; j < 4u; ++j) {
            u64 m[6] = {0, 0, 0, 0, 0, 0};
            for (uint32_t l = 0; l < 64u; ++l) {
                const uint32_t pos = c * 256u + j * 64u + l;
                const char b = pos >= head && pos < span ? ops.at(pos - head) : char(0);
                const char* at = b ? strchr("=XIDid", b) : nullptr;
                if (at) m[at - "=XIDid"] |= 1ull << l;
            }
            acc.begin(m[0], m[1], m[2], m[3], m[4], m[5]);
            for (uint32_t l = 0; l < 64u; ++l) {
                const bool behind = !acc.is_ins(l) && (l ? acc.is_ins(l - 1u) : acc.open_len != 0u);
                if (!behind) continue;
                got.at(acc.row(l)) = inserts_len_byte(acc.ins_index(l)), ++writers.at(acc.row(l)), ++runs_seen;
            }
            acc.end_len();
            acc.end();
        }
    if (acc.open_len != 0u) got.at(acc.r) = inserts_len_byte(acc.open_len), ++writers.at(acc.r), ++tail_runs;
    EXPECT(got == want);
    for (size_t r = 0; r < writers.size(); ++r) EXPECT(writers[r] == (want[r] ? 1 : 0));
}

std::string random_ops(std::mt19937& rng, uint32_t len, int32_t& rlen)
{
    std::string s;
    while (s.size() < len) {
        const uint32_t x = rng() % 100u;
        if (x < 8) {
            const uint32_t runs[] = {1, 2, 19, 63, 64, 65, 254, 255, 256, 300};
            s.append(runs[rng() % 10u], 'I');
            s += "=XD"[rng() % 3u];  // (two runs are separated by a byte that consumes a reference base)
        } else {
            s += x < 12 ? 'D' : x < 20 ? 'X' : '=';
        }
    }
    s.resize(len);
    if (len && rng() % 3u == 0) s = std::string(rng() % 5u, 'i') + s + std::string(rng() % 5u, 'i');
    if (rng() % 4u == 0) s = std::string(rng() % 4u, 'd') + s;
    for (size_t a = 0; a + 1 < s.size(); ++a)
        if (s[a] == 'I' && s[a + 1] == 'i') s[a + 1] = '=';  // (keep the string one the aligner could write: no 'I' run is cut by 'i' alone)
    rlen = 0;
    for (char c : s) rlen += c == '=' || c == 'X' || c == 'D' || c == 'd';
    return s;
}

// ---- the kernels of the stage ----
struct Segment {
    int32_t rlen = 0;
    std::vector<std::vector<uint8_t>> base, ilen;  // per read, rlen + 1 bytes
    std::vector<uint64_t> pre_key, pre_mask;
    uint64_t pre_full = 0;
    bool with_pre = false;
};

uint32_t scan_incl(const uint32_t* v, uint32_t lane)
{
    uint32_t s = 0;
    for (uint32_t l = 0; l <= lane; ++l) s += v[l];
    return s;
}

// window_sums: W(p0 + lane) for the 64 lanes, and the lanes' own bytes
void window_sums(const std::vector<uint8_t>& plane, int32_t rlen, long long p0, uint32_t slack, uint32_t* win, uint32_t* own)
{
    auto at = [&](long long q) -> uint32_t { return q >= 0 && q <= rlen ? plane.at(size_t(q)) : 0u; };
    uint32_t halo[64], sV[64], sH[64];
    for (uint32_t l = 0; l < 64u; ++l) own[l] = at(p0 + l), halo[l] = at(l < 32u ? p0 - 32 + l : p0 + 32 + l);
    for (uint32_t l = 0; l < 64u; ++l) sV[l] = scan_incl(own, l), sH[l] = scan_incl(halo, l);
    const uint32_t left = sH[31], mid = sV[63];
    auto prefix = [&](int idx) -> uint32_t {
        const uint32_t fromH = sH[uint32_t(idx < 32 ? idx : idx - 64) & 63u], fromV = sV[uint32_t(idx - 32) & 63u];
        return idx < 0 ? 0u : idx < 32 ? fromH : idx < 96 ? left + fromV : mid + fromH;
    };
    for (uint32_t l = 0; l < 64u; ++l) win[l] = prefix(int(32u + l + slack)) - prefix(int(32u + l) - int(slack) - 1);
    ++windows_seen;
}

void check_segment(const Segment& s, const InsertsRule& rule)
{
    const uint32_t n = uint32_t(s.base.size()), rlen = uint32_t(s.rlen), W = rlen / 64u + 1u, rows = rlen + 1u;
    const uint32_t slots = uint32_t(inserts_sites_most(s.rlen, rule.max_sites));
    // the definition
    std::vector<uint8_t> fb, fl;
    for (uint32_t i = 0; i < n; ++i) fb.insert(fb.end(), s.base[i].begin(), s.base[i].end()), fl.insert(fl.end(), s.ilen[i].begin(), s.ilen[i].end());
    std::vector<ioc_insert_row> want_rows(rows);
    std::vector<ioc_pile_insert> want_sites(std::max(slots, 1u));
    std::vector<ioc_read_inserts> want_reads(n);
    ioc_inserts_seg want_seg{};
    EXPECT(ioc_host_planes_inserts(n ? fb.data() : nullptr, n ? fl.data() : nullptr, int32_t(n), s.rlen, rule.min_ins, rule.slack, rule.min_depth, rule.min_alt,
                                   rule.min_pct, rule.max_sites, s.with_pre && n ? s.pre_key.data() : nullptr, s.with_pre && n ? s.pre_mask.data() : nullptr, s.pre_full,
                                   want_rows.data(), want_sites.data(), n ? want_reads.data() : nullptr, &want_seg) == IOC_OK);
    auto pre_key = [&](uint32_t i) -> u64 { return s.with_pre ? u64(s.pre_key.at(i)) : 0ull; };
    auto pre_mask = [&](uint32_t i) -> u64 { return s.with_pre ? u64(s.pre_mask.at(i)) : 0ull; };
    const u64 pre_full = s.with_pre ? s.pre_full : 0ull;

    // k_ins_bits
    std::vector<std::vector<u64>> span(n, std::vector<u64>(W, 0)), near(n, std::vector<u64>(W, 0));
    std::vector<std::vector<int>> word_writers(n, std::vector<int>(W, 0));
    std::vector<ioc_read_inserts> reads(n, ioc_read_inserts{});
    for (uint32_t i = 0; i < n; ++i) {
        u64 carry = 0;
        uint32_t n_near = 0, bases = 0;
        for (uint32_t b0 = 0; b0 < W; b0 += 64u) {
            u64 mine_s[64] = {0}, mine_n[64] = {0};
            for (uint32_t c = b0; c < std::min(b0 + 64u, W); ++c) {
                u64 cw = 0;
                for (uint32_t l = 0; l < 64u; ++l) {
                    const u64 p = u64(c) * 64u + l;
                    const uint8_t b = p < rlen ? s.base[i].at(size_t(p)) : uint8_t(IOC_ALLELE_NONE);
                    cw |= u64(blocks_covers(b)) << l;
                }
                const u64 sw = cw & (cw << 1 | carry);
                carry = cw >> 63;
                uint32_t win[64], own[64];
                window_sums(s.ilen[i], s.rlen, (long long)c * 64, uint32_t(rule.slack), win, own);
                u64 nw = 0;
                for (uint32_t l = 0; l < 64u; ++l) {
                    const bool spans = (sw >> l) & 1ull;
                    nw |= u64(spans && win[l] >= uint32_t(rule.min_ins)) << l;
                    if (spans) bases += own[l];
                }
                n_near += uint32_t(__builtin_popcountll(nw));
                mine_s[c - b0] = sw, mine_n[c - b0] = nw;  // (lane c - b0 keeps them)
            }
            for (uint32_t l = 0; l < 64u && b0 + l < W; ++l) span[i].at(b0 + l) = mine_s[l], near[i].at(b0 + l) = mine_n[l], ++word_writers[i].at(b0 + l);
            if (b0 + 64u < W) ++batches_crossed;
        }
        reads[i].n_near = int32_t(n_near), reads[i].ins_bases = int32_t(bases);
        for (int w : word_writers[i]) EXPECT(w == 1);
    }

    // k_ins_rows
    std::vector<ioc_insert_row> got_rows(rows, ioc_insert_row{0xEEEEEEEEu, 0xEEEEEEEEu});
    std::vector<int> row_writers(rows, 0);
    std::vector<u64> var(W, 0);
    for (uint32_t c = 0; c < W; ++c) {
        uint32_t spanned[64] = {0}, in[64] = {0};
        for (uint32_t m0 = 0; m0 < n; m0 += 64u)
            for (uint32_t r = 0; r < 64u; ++r)
                for (uint32_t l = 0; l < 64u && m0 + l < n; ++l) spanned[r] += uint32_t((span[m0 + l][c] >> r) & 1ull), in[r] += uint32_t((near[m0 + l][c] >> r) & 1ull);
        for (uint32_t l = 0; l < 64u; ++l) {
            const u64 p = u64(c) * 64u + l;
            if (p <= rlen) got_rows.at(size_t(p)) = ioc_insert_row{spanned[l], in[l]}, ++row_writers.at(size_t(p));
            if (p >= 1u && p + 1u <= rlen && rule.variable(spanned[l], in[l])) var[c] |= 1ull << l;
        }
    }
    for (int w : row_writers) EXPECT(w == 1);
    EXPECT(memcmp(got_rows.data(), want_rows.data(), rows * sizeof(ioc_insert_row)) == 0);

    // k_ins_list
    std::vector<ioc_pile_insert> sites(slots, ioc_pile_insert{});
    std::vector<int> first_writers(slots, 0), end_writers(slots, 0);
    auto load = [&](uint32_t i) -> u64 { return i < W ? var.at(i) : 0ull; };
    uint32_t base_s = 0, base_e = 0;
    u64 top = 0;
    for (uint32_t b0 = 0; b0 < W; b0 += 64u) {
        u64 w[64];
        uint32_t ns[64], ne[64];
        u64 st[64], en[64];
        for (uint32_t l = 0; l < 64u; ++l) w[l] = load(b0 + l);
        for (uint32_t l = 0; l < 64u; ++l) {
            const u64 dn = w[(l + 63u) & 63u], up = w[(l + 1u) & 63u];
            const uint32_t left = uint32_t(l ? dn >> 63 : top), right = uint32_t((l < 63u ? up : load(b0 + 64u)) & 1ull);
            st[l] = run_starts(w[l], left), en[l] = run_ends(w[l], right);
            ns[l] = uint32_t(__builtin_popcountll(st[l])), ne[l] = uint32_t(__builtin_popcountll(en[l]));
        }
        for (uint32_t l = 0; l < 64u; ++l) {
            const uint32_t is = scan_incl(ns, l), ie = scan_incl(ne, l), row = (b0 + l) * 64u;
            u64 a = st[l], e = en[l];
            for (uint32_t k = base_s + is - ns[l]; a && k < slots; ++k, a &= a - 1ull) sites.at(k).first = int32_t(row + uint32_t(__builtin_ctzll(a))), ++first_writers.at(k);
            for (uint32_t k = base_e + ie - ne[l]; e && k < slots; ++k, e &= e - 1ull) sites.at(k).end = int32_t(row + uint32_t(__builtin_ctzll(e)) + 1u), ++end_writers.at(k);
        }
        base_s += scan_incl(ns, 63), base_e += scan_incl(ne, 63);
        top = w[63] >> 63;
    }
    EXPECT(base_s == base_e);
    const uint32_t n_sites = std::min(base_s, slots);
    EXPECT(int32_t(n_sites) == want_seg.n_sites && int32_t(base_s) == want_seg.n_found);
    for (uint32_t k = 0; k < slots; ++k) EXPECT(first_writers[k] == (k < n_sites ? 1 : 0) && end_writers[k] == (k < n_sites ? 1 : 0));
    sites_seen += n_sites;

    // k_ins_states
    std::vector<u64> mask(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        u64 key = 0;
        for (uint32_t lane = 0; lane < n_sites && lane < uint32_t(IOC_INSERTS_MAX); ++lane) {
            const long long first = sites[lane].first, end = sites[lane].end;
            uint32_t c = 0, t = 0;
            for (long long w = first / 64; w * 64 < end && w < (long long)W; ++w) {
                const u64 m = run_row_mask(w * 64, first, end);
                c += uint32_t(__builtin_popcountll(span[i].at(size_t(w)) & m)), t += uint32_t(__builtin_popcountll(near[i].at(size_t(w)) & m));
            }
            const uint32_t st = inserts_state(uint32_t(end - first), c, t);
            key |= u64(st) << (2u * lane), mask[i] |= blocks_state_mask(lane, st);
            ++states_seen[st];
        }
        reads[i].key = key;
    }

    // k_ins_states, second half: site by site where the pair carries, its largest W into its place of the scratch table
    const uint32_t S = uint32_t(rule.max_sites);
    std::vector<uint16_t> wmax(size_t(n) * S, uint16_t(0xEEEE));
    std::vector<int> wmax_writers(size_t(n) * S, 0);
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t k = 0; k < n_sites && k < uint32_t(IOC_INSERTS_MAX); ++k) {
            if (((reads[i].key >> (2u * k)) & 3ull) != u64(IOC_INS_CARRY)) continue;
            uint32_t longest = 0;
            for (long long p0 = sites[k].first; p0 < sites[k].end; p0 += 64) {
                uint32_t win[64], own[64];
                window_sums(s.ilen[i], s.rlen, p0, uint32_t(rule.slack), win, own);
                for (uint32_t l = 0; l < 64u; ++l)
                    if (p0 + l < sites[k].end) longest = std::max(longest, win[l]);
            }
            EXPECT(longest <= 0xFFFFu && k < S);
            wmax.at(size_t(i) * S + k) = uint16_t(longest), ++wmax_writers.at(size_t(i) * S + k);
        }
    for (int w : wmax_writers) EXPECT(w <= 1);

    // k_ins_lens: the members 64 at a time, a lane each
    for (uint32_t k = 0; k < n_sites; ++k) {
        uint32_t lane_min[64], lane_max[64];
        for (uint32_t l = 0; l < 64u; ++l) lane_min[l] = 0xFFFFFFFFu, lane_max[l] = 0;
        for (uint32_t m0 = 0; m0 < n; m0 += 64u)
            for (uint32_t l = 0; l < 64u && m0 + l < n; ++l) {
                const uint32_t i = m0 + l;
                if (((reads[i].key >> (2u * k)) & 3ull) != u64(IOC_INS_CARRY)) continue;
                EXPECT(wmax_writers.at(size_t(i) * S + k) == 1);
                const uint32_t longest = wmax.at(size_t(i) * S + k);
                lane_min[l] = std::min(lane_min[l], longest), lane_max[l] = std::max(lane_max[l], longest);
            }
        const uint32_t len_min = *std::min_element(lane_min, lane_min + 64), len_max = *std::max_element(lane_max, lane_max + 64);
        sites[k].len_min = len_max ? len_min : 0u, sites[k].len_max = len_max;
    }

    // k_ins_support, k_ins_isoforms, k_ins_record
    const u64 full = blocks_full_mask(n_sites);
    enum : uint32_t { SUPPORTED = 1, FIRST = 2 };
    std::vector<uint8_t> flags(n, 0);
    auto complete = [&](uint32_t i) { return mask[i] == full && pre_mask(i) == pre_full; };
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t same = 0, earlier = 0;
        for (uint32_t x = 0; x < n; ++x) {
            const bool hit = complete(x) && reads[x].key == reads[i].key && pre_key(x) == pre_key(i);
            same += hit, earlier += hit && x < i;
        }
        flags[i] = uint8_t(complete(i) && same >= uint32_t(rule.min_alt) ? SUPPORTED | (earlier == 0u ? FIRST : 0u) : 0u);
    }
    auto rank = [&](u64 pre, u64 key) {
        uint32_t r = 0;
        for (uint32_t x = 0; x < n; ++x) r += (flags[x] & FIRST) && inserts_key_less(pre_key(x), reads[x].key, pre, key);
        return r;
    };
    ioc_inserts_seg seg{int32_t(n_sites), int32_t(base_s), 0, int32_t(n), 0, 0, 0, 0};
    for (uint32_t i = 0; i < n; ++i) {
        int32_t group = -1, how;
        if (complete(i)) {
            how = (flags[i] & SUPPORTED) ? IOC_ISO_DIRECT : IOC_ISO_RARE;
            if (how == IOC_ISO_DIRECT) group = int32_t(rank(pre_key(i), reads[i].key));
        } else {
            uint32_t agreeing = 0;
            u64 which_pre = 0, which_key = 0;
            for (uint32_t x = 0; x < n && (mask[i] | pre_mask(i)) != 0ull; ++x)
                if ((flags[x] & FIRST) && inserts_key_agrees(pre_key(i), reads[i].key, pre_key(x), reads[x].key, pre_mask(i), mask[i])) {
                    if (agreeing == 0u) which_pre = pre_key(x), which_key = reads[x].key;
                    ++agreeing;
                }
            how = agreeing == 1u ? IOC_ISO_ASSIGNED : IOC_ISO_AMBIGUOUS;
            if (agreeing == 1u) group = int32_t(rank(which_pre, which_key));
        }
        reads[i].group = group, reads[i].how = how;
        ++hows_seen[how];
        seg.n_groups += (flags[i] & FIRST) != 0;
        ++(how == IOC_ISO_DIRECT ? seg.n_direct : how == IOC_ISO_ASSIGNED ? seg.n_assigned : how == IOC_ISO_RARE ? seg.n_rare : seg.n_ambiguous);
        for (uint32_t b = 0; b < n_sites; ++b) {
            const uint32_t st = uint32_t(reads[i].key >> (2u * b)) & 3u;
            ++(st == IOC_INS_CARRY ? sites[b].n_carry : st == IOC_INS_LACK ? sites[b].n_lack : sites[b].n_none);
            EXPECT(st != 2u);
        }
    }
    EXPECT(memcmp(&seg, &want_seg, sizeof seg) == 0);
    EXPECT(n_sites == 0 || memcmp(sites.data(), want_sites.data(), n_sites * sizeof(ioc_pile_insert)) == 0);
    EXPECT(n == 0 || memcmp(reads.data(), want_reads.data(), n * sizeof(ioc_read_inserts)) == 0);
}

Segment make_segment(std::mt19937& rng, int32_t rlen, uint32_t n, uint32_t n_sites, bool with_pre)
{
    Segment s;
    s.rlen = rlen;
    s.with_pre = with_pre;
    s.pre_full = rng() % 2u ? ~0ull : 0xFull;
    const u64 words[] = {0ull, 1ull, 4ull, 5ull, (1ull << 63) | 1ull};
    for (uint32_t i = 0; i < n; ++i) {
        std::vector<uint8_t> b(size_t(rlen) + 1), l(size_t(rlen) + 1, 0);
        for (auto& x : b) x = uint8_t(rng() % 6u);
        b[size_t(rlen)] = uint8_t(IOC_ALLELE_NONE);
        if (rlen > 4 && rng() % 5u == 0) std::fill(b.begin(), b.begin() + rng() % uint32_t(rlen), uint8_t(IOC_ALLELE_NONE));           // starts late
        if (rlen > 4 && rng() % 5u == 0) std::fill(b.begin() + rng() % uint32_t(rlen), b.end(), uint8_t(IOC_ALLELE_NONE));             // stops early
        if (rlen > 0 && rng() % 4u == 0) b[rng() % uint32_t(rlen)] = rng() % 2u ? uint8_t(6) : uint8_t(0xEE);
        for (uint32_t k = 0; k < 3u && rlen > 0; ++k)
            if (rng() % 2u) l[rng() % (uint32_t(rlen) + 1u)] = uint8_t(1u + rng() % 60u);                                              // noise, rows 0 and rlen included
        s.base.push_back(b), s.ilen.push_back(l);
        s.pre_key.push_back(words[rng() % 5u] & s.pre_full), s.pre_mask.push_back(rng() % 5u ? s.pre_full : s.pre_full & 3ull);
    }
    for (uint32_t k = 0; k < n_sites && rlen > 2; ++k) {  // a site: a group of reads shares an insertion, whole or in two runs
        const uint32_t at = n_sites > 8 ? 25u + 50u * k : rng() % 4u == 0 ? (rng() % 2u ? 62u : 4094u) % uint32_t(rlen) : rng() % uint32_t(rlen);
        const uint32_t group = rng() % 3u;
        for (uint32_t i = 0; i < n; ++i) {
            if (i % 3u != group && rng() % 8u) continue;
            const uint32_t len = rng() % 6u == 0 ? 255u : 15u + rng() % 40u;
            if (rng() % 2u && at + 6u <= uint32_t(rlen)) s.ilen[i][at] = uint8_t(len / 2u), s.ilen[i][at + 6u] = uint8_t(len - len / 2u);
            else s.ilen[i][std::min(at + uint32_t(rng() % 2u), uint32_t(rlen))] = uint8_t(len);
        }
    }
    return s;
}

}  // namespace

int main()
{
    std::mt19937 rng(12345);
    for (uint32_t len : {0u, 1u, 3u, 63u, 64u, 65u, 250u, 251u, 252u, 253u, 254u, 255u, 256u, 257u, 511u, 512u, 513u, 1000u, 3000u})
        for (uint32_t head = 0; head < 4u; ++head)
            for (int rep = 0; rep < 6; ++rep) {
                int32_t rlen;
                const std::string ops = random_ops(rng, len, rlen);
                project_ilen(ops, head, rlen);
            }
    for (uint32_t total : {256u, 512u, 768u})  // a string that ends in a run with the last byte of the last chunk: nobody stands behind it
        for (uint32_t head = 0; head < 4u; ++head)
            for (uint32_t run : {1u, 63u, 64u, 65u, 200u}) {
                const uint32_t len = total - head;
                project_ilen(std::string(len - run, '=') + std::string(run, 'I'), head, int32_t(len - run));
            }
    project_ilen(std::string(300, 'I'), 0, 0), project_ilen(std::string(256, 'I'), 0, 0), project_ilen("iI==Ii", 1, 2);

    const InsertsRule rules[] = {{20, 8, 3, 3, 25, 32}, {20, 0, 2, 2, 10, 32}, {30, 32, 3, 2, 25, 4}, {1, 31, 1, 1, 1, 32}, {255, 8, 2, 2, 25, 1}};
    const int32_t lens[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 600, 4200, 9000};
    const uint32_t counts[] = {0, 1, 3, 64, 65, 130};
    for (const InsertsRule& rule : rules)
        for (int32_t rlen : lens)
            for (uint32_t n : counts) {
                if (rlen >= 4200 && n > 65) continue;  // (the plain definition is quadratic in the window)
                check_segment(make_segment(rng, rlen, n, rlen >= 600 ? 6u : 2u, n % 2u == 0), rule);
            }
    for (const InsertsRule& rule : rules) check_segment(make_segment(rng, 2000, 64, 35, true), rule);  // 35 sites under max_sites 32
    Segment all = make_segment(rng, 64, 64, 0, false);  // 255 throughout every window: the largest sum
    for (uint32_t i = 0; i < 20; ++i) std::fill(all.ilen[i].begin(), all.ilen[i].end(), uint8_t(255)), std::fill(all.base[i].begin(), all.base[i].end() - 1, uint8_t(0));
    check_segment(all, InsertsRule{255, 32, 3, 3, 25, 32});

    printf("%lld runs behind a byte, %lld at a chunk's end, %lld windows, %lld sites, %lld batches crossed, states %lld %lld %lld, hows %lld %lld %lld %lld\n", runs_seen,
           tail_runs, windows_seen, sites_seen, batches_crossed, states_seen[0], states_seen[1], states_seen[3], hows_seen[0], hows_seen[1], hows_seen[2], hows_seen[3]);
    if (faults || !runs_seen || !tail_runs || !sites_seen || !batches_crossed || !states_seen[0] || !states_seen[1] || !states_seen[3] || !hows_seen[0] ||
        !hows_seen[1] || !hows_seen[2] || !hows_seen[3]) {
        fprintf(stderr, "%d faults\n", faults);
        return 1;
    }
    puts("ok");
    return 0;
}
