// read_blocks_check.cpp — the chunk and word logic of the kernels of isonclust2_amd/csrc/ioc_read_blocks.hip, restated lane by
// lane on the CPU and compared with the definition, ioc_host_planes_blocks (ioc_align.cpp):
//
//  * k_plane_bits: a chunk of 64 plane bytes becomes a covered word and a deleted word (the ballot is a loop over 64 lanes);
//  * the run sweep of k_gap_words and k_block_list: lane w holds word w of a batch of 64, the ballot of "has a clear bit" gives
//    every lane the nearest such word on either side, a saturated carry comes in from the batch below and the read-ahead from the
//    batches above, and run_long_bits (ioc_read_blocks.h) marks the bits of long runs — runs that cross words, whole words, whole
//    batches and two batch edges are there;
//  * k_block_rows: depth and in_gap bit by bit from the members' words, the variable-row word;
//  * k_block_list: the k-th start and the k-th end of the long runs paired by a prefix sum over the lanes and a running base;
//  * k_read_states: masked popcounts of the words a block spans; k_key_support, k_read_isoforms, k_blocks_record: counts over the
//    members with UNSIGNED key compares.
// Every buffer is a block of exactly its size.  The inputs: the planted shapes — segments of 0, 1, 19, 20, 63, 64, 65, 127, 128,
// 129, 600, 4200 and 9000 rows with 0 to 130 reads, runs of deletions of 1 to 300 rows placed at random, shared by groups of
// reads so that blocks form, one of 4100 and one of 8500 rows, reads that stop early or start late, bytes no projection writes, 35
// blocks under max_blocks 32 with keys that differ in bit 63 — under three rules.
//
// Host code only; meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/read_blocks_check tools/read_blocks_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/read_blocks_check
//
// Exit status 0 and "ok" when everything agrees.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "ioc_read_blocks.h"
#include "isonclust2_hip.h"

namespace {

typedef unsigned long long u64;
int faults = 0;
long long long_runs_seen = 0, batches_crossed = 0, blocks_seen = 0, hows_seen[4] = {0, 0, 0, 0};

#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            if (++faults < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
        }                                                                   \
    } while (0)

// RunSweep of the kernels: one batch of 64 lanes at b0 of a plane of W words; what the lanes hold afterwards
struct Sweep {
    const std::vector<u64>& words;
    uint32_t W, least;
    uint32_t carry = 0;
    u64 w[64], q[64];
    uint32_t left[64], right[64];
    u64 load(uint32_t i) const { return i < W ? words.at(i) : 0ull; }
    void next(uint32_t b0)
    {
        u64 nonfull = 0;
        for (uint32_t l = 0; l < 64; ++l) w[l] = load(b0 + l), nonfull |= u64(~w[l] != 0ull) << l;
        uint32_t ahead = 0;
        for (uint32_t nb = b0 + 64u; nb < W; nb += 64u) {
            u64 nf = 0;
            for (uint32_t l = 0; l < 64; ++l) nf |= u64(~load(nb + l) != 0ull) << l;
            if (nf) {
                const uint32_t j = uint32_t(__builtin_ctzll(nf));
                ahead = run_sat(u64(ahead) + 64ull * j + run_lead(load(nb + j)), least);
                break;
            }
            ahead = run_sat(u64(ahead) + 4096ull, least);
            ++batches_crossed;
            if (ahead >= least) break;
        }
        for (uint32_t l = 0; l < 64; ++l) {
            const uint32_t below = run_src_below(nonfull, l), above = run_src_above(nonfull, l);
            left[l] = run_left_in(l, below, run_trail(w[below & 63u]), carry, least);
            right[l] = run_right_in(l, above, run_lead(w[above & 63u]), ahead, least);
            q[l] = run_long_bits(w[l], left[l], right[l], least);
        }
        if (nonfull) {
            const uint32_t j = 63u - uint32_t(__builtin_clzll(nonfull));
            carry = run_sat(64ull * (63u - j) + run_trail(w[j]), least);
        } else {
            carry = run_sat(4096ull + carry, least);
        }
    }
};

// one segment through the restated kernels
struct Result {
    std::vector<ioc_block_row> rows;
    std::vector<ioc_pile_block> blocks;
    std::vector<ioc_read_blocks> reads;
    ioc_blocks_seg seg;
};

Result restated(const std::vector<uint8_t>& base, uint32_t n, uint32_t rlen, const BlocksRule& rule)
{
    const uint32_t W = rlen / 64u + 1u, rows = rlen + 1u;
    std::vector<std::vector<u64>> cov(n, std::vector<u64>(W, 0)), del(n, std::vector<u64>(W, 0)), gap(n, std::vector<u64>(W, 0));
    Result r{std::vector<ioc_block_row>(rows, ioc_block_row{0, 0}), {}, std::vector<ioc_read_blocks>(n, ioc_read_blocks{}), ioc_blocks_seg{}};
    // k_plane_bits
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t c = 0; c < W; ++c)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const u64 p = u64(c) * 64u + lane;
                const uint8_t b = p < rlen ? base.at(size_t(i) * rows + p) : uint8_t(IOC_ALLELE_NONE);
                cov[i][c] |= u64(blocks_covers(b)) << lane, del[i][c] |= u64(b == uint8_t(IOC_ALLELE_DEL)) << lane;
            }
    // k_gap_words
    for (uint32_t i = 0; i < n; ++i) {
        Sweep sw{del[i], W, uint32_t(rule.min_gap)};
        uint32_t n_gaps = 0, gap_rows = 0, first = 0xFFFFFFFFu, end = 0;
        for (uint32_t b0 = 0; b0 < W; b0 += 64u) {
            sw.next(b0);
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t w = b0 + lane;
                if (w < W) {
                    gap[i].at(w) = sw.q[lane];
                    const u64 cw = cov[i][w];
                    if (cw) first = std::min(first, w * 64u + uint32_t(__builtin_ctzll(cw))), end = std::max(end, w * 64u + 64u - uint32_t(__builtin_clzll(cw)));
                } else {
                    EXPECT(sw.q[lane] == 0ull);
                }
                n_gaps += uint32_t(__builtin_popcountll(run_starts(sw.q[lane], sw.left[lane])));
                gap_rows += uint32_t(__builtin_popcountll(sw.q[lane]));
            }
        }
        r.reads[i].first_row = end ? int32_t(first) : 0, r.reads[i].end_row = int32_t(end), r.reads[i].n_gaps = int32_t(n_gaps), r.reads[i].gap_rows = int32_t(gap_rows);
        long_runs_seen += n_gaps;
    }
    // k_block_rows
    std::vector<u64> var(W, 0);
    for (uint32_t c = 0; c < W; ++c)
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const u64 p = u64(c) * 64u + lane;
            uint32_t depth = 0, in = 0;
            for (uint32_t i = 0; i < n; ++i) depth += uint32_t(cov[i][c] >> lane) & 1u, in += uint32_t(gap[i][c] >> lane) & 1u;
            if (p <= rlen) r.rows.at(size_t(p)) = ioc_block_row{depth, in};
            var[c] |= u64(p < rlen && blocks_row_variable(rule, depth, in)) << lane;
        }
    // k_block_list
    const uint32_t most = uint32_t(rule.max_blocks), slots = std::min(most, rlen);
    r.blocks.assign(slots, ioc_pile_block{});
    std::vector<int> first_writers(slots, 0), end_writers(slots, 0);
    {
        Sweep sw{var, W, uint32_t(rule.min_block)};
        uint32_t base_s = 0, base_e = 0;
        for (uint32_t b0 = 0; b0 < W; b0 += 64u) {
            sw.next(b0);
            uint32_t is = 0, ie = 0;  // (the inclusive scan, lane by lane)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                u64 st = run_starts(sw.q[lane], sw.left[lane]), en = run_ends(sw.q[lane], sw.right[lane]);
                const uint32_t ns = uint32_t(__builtin_popcountll(st)), ne = uint32_t(__builtin_popcountll(en));
                is += ns, ie += ne;
                const uint32_t row = (b0 + lane) * 64u;
                for (uint32_t k = base_s + is - ns; st && k < most; ++k, st &= st - 1ull) r.blocks.at(k).first = int32_t(row + uint32_t(__builtin_ctzll(st))), ++first_writers.at(k);
                for (uint32_t k = base_e + ie - ne; en && k < most; ++k, en &= en - 1ull)
                    r.blocks.at(k).end = int32_t(row + uint32_t(__builtin_ctzll(en)) + 1u), ++end_writers.at(k);
            }
            base_s += is, base_e += ie;
        }
        EXPECT(base_s == base_e);
        r.seg.n_blocks = int32_t(std::min(base_s, most)), r.seg.n_found = int32_t(base_s);
    }
    const uint32_t nb = uint32_t(r.seg.n_blocks);
    for (uint32_t k = 0; k < slots; ++k) EXPECT(first_writers[k] == (k < nb) && end_writers[k] == (k < nb));
    r.blocks.resize(nb);
    blocks_seen += nb;
    // k_read_states
    std::vector<u64> mask(n, 0);
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t lane = 0; lane < nb; ++lane) {
            const long long first = r.blocks[lane].first, end = r.blocks[lane].end;
            uint32_t c = 0, s = 0;
            for (long long w = first / 64; w * 64 < end && w < (long long)W; ++w) {
                const u64 m = run_row_mask(w * 64, first, end);
                c += uint32_t(__builtin_popcountll(cov[i].at(size_t(w)) & m)), s += uint32_t(__builtin_popcountll(del[i].at(size_t(w)) & m));
            }
            const uint32_t st = blocks_state(uint32_t(end - first), c, s);
            r.reads[i].key |= u64(st) << (2u * lane), mask[i] |= blocks_state_mask(lane, st);
        }
    // k_key_support
    const u64 full = blocks_full_mask(nb);
    std::vector<uint8_t> flags(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t same = 0, earlier = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const bool hit = mask[j] == full && r.reads[j].key == r.reads[i].key;
            same += hit, earlier += hit && j < i;
        }
        flags[i] = uint8_t(mask[i] == full && same >= uint32_t(rule.min_alt) ? 1u | (earlier == 0u ? 2u : 0u) : 0u);
    }
    // k_read_isoforms
    auto rank = [&](u64 key) {
        uint32_t k = 0;
        for (uint32_t j = 0; j < n; ++j) k += (flags[j] & 2u) && u64(r.reads[j].key) < key;
        return k;
    };
    for (uint32_t i = 0; i < n; ++i) {
        const u64 key = r.reads[i].key;
        int32_t group = -1, how;
        if (mask[i] == full) {
            how = (flags[i] & 1u) ? IOC_ISO_DIRECT : IOC_ISO_RARE;
            if (how == IOC_ISO_DIRECT) group = int32_t(rank(key));
        } else {
            uint32_t agreeing = 0;
            u64 which = 0;
            for (uint32_t j = 0; j < n && mask[i] != 0ull; ++j)
                if ((flags[j] & 2u) && blocks_key_agrees(key, r.reads[j].key, mask[i])) {
                    if (agreeing == 0u) which = r.reads[j].key;
                    ++agreeing;
                }
            how = agreeing == 1u ? IOC_ISO_ASSIGNED : IOC_ISO_AMBIGUOUS;
            if (agreeing == 1u) group = int32_t(rank(which));
        }
        r.reads[i].group = group, r.reads[i].how = how;
        ++hows_seen[how];
    }
    // k_blocks_record
    r.seg.n_reads = int32_t(n);
    for (uint32_t i = 0; i < n; ++i) {
        r.seg.n_groups += (flags[i] & 2u) != 0;
        const int32_t how = r.reads[i].how;
        ++(how == IOC_ISO_DIRECT ? r.seg.n_direct : how == IOC_ISO_ASSIGNED ? r.seg.n_assigned : how == IOC_ISO_RARE ? r.seg.n_rare : r.seg.n_ambiguous);
        for (uint32_t lane = 0; lane < nb; ++lane) {
            const uint32_t st = uint32_t(u64(r.reads[i].key) >> (2u * lane)) & 3u;
            ++(st == 0u ? r.blocks[lane].n_keep : st == 1u ? r.blocks[lane].n_skip : st == 2u ? r.blocks[lane].n_part : r.blocks[lane].n_none);
        }
    }
    return r;
}

void compare(const std::vector<uint8_t>& base, uint32_t n, uint32_t rlen, const BlocksRule& k)
{
    const Result got = restated(base, n, rlen, k);
    std::vector<ioc_block_row> rows(rlen + 1u);
    std::vector<ioc_pile_block> blocks(std::min(uint32_t(k.max_blocks), rlen));
    std::vector<ioc_read_blocks> reads(n);
    ioc_blocks_seg seg;
    const int rc = ioc_host_planes_blocks(base.data(), int32_t(n), int32_t(rlen), k.min_gap, k.min_depth, k.min_alt, k.min_pct, k.min_block, k.max_blocks, rows.data(),
                                          blocks.data(), reads.data(), &seg);
    EXPECT(rc == IOC_OK);
    EXPECT(memcmp(&seg, &got.seg, sizeof seg) == 0);
    EXPECT(memcmp(rows.data(), got.rows.data(), rows.size() * sizeof(ioc_block_row)) == 0);
    EXPECT(got.blocks.size() == size_t(seg.n_blocks) && (got.blocks.empty() || memcmp(blocks.data(), got.blocks.data(), got.blocks.size() * sizeof(ioc_pile_block)) == 0));
    EXPECT(n == 0 || memcmp(reads.data(), got.reads.data(), n * sizeof(ioc_read_blocks)) == 0);
}

std::vector<uint8_t> planes(std::mt19937& rng, uint32_t n, uint32_t rlen, bool shared)
{
    const uint32_t rows = rlen + 1u;
    std::vector<uint8_t> b(size_t(n) * rows);
    for (uint8_t& x : b) x = uint8_t(rng() % 5u);
    auto del = [&](uint32_t i, uint32_t a, uint32_t len) {
        for (uint32_t p = a; p < std::min(a + len, rlen); ++p) b[size_t(i) * rows + p] = uint8_t(IOC_ALLELE_DEL);
    };
    for (int g = 0; shared && rlen > 0 && g < 6; ++g) {  // a third of the reads share a run: a block
        const uint32_t a = rng() % rlen, len = 1u + rng() % 300u, from = rng() % 3u;
        for (uint32_t i = from; i < n; i += 3u) del(i, a + rng() % 3u, len);
    }
    for (uint32_t i = 0; i < n && rlen > 0; ++i) {
        for (int x = rng() % 3u; x > 0; --x) del(i, rng() % rlen, 1u + rng() % 140u);
        if (rng() % 8u == 0) std::fill(b.begin() + size_t(i) * rows, b.begin() + size_t(i) * rows + rng() % rows, uint8_t(IOC_ALLELE_NONE));
        if (rng() % 8u == 0) std::fill(b.begin() + size_t(i) * rows + rng() % rows, b.begin() + size_t(i + 1) * rows, uint8_t(IOC_ALLELE_NONE));
        if (rng() % 6u == 0) b[size_t(i) * rows + rng() % rlen] = rng() % 2u ? 6 : 0xEE;
    }
    for (uint32_t i = 0; i < n; ++i) b[size_t(i) * rows + rlen] = rng() % 4u ? uint8_t(IOC_ALLELE_NONE) : uint8_t(IOC_ALLELE_DEL);  // (row rlen takes part in nothing)
    return b;
}

}  // namespace

int main()
{
    std::mt19937 rng(7);
    const BlocksRule rules[3] = {{20, 3, 3, 25, 10, 32}, {5, 2, 2, 10, 3, 4}, {1, 1, 1, 50, 1, 1}};
    const uint32_t lens[] = {0, 1, 19, 20, 63, 64, 65, 127, 128, 129, 600}, counts[] = {0, 1, 2, 3, 5, 64, 65, 130};
    for (uint32_t rlen : lens)
        for (uint32_t n : counts)
            for (const BlocksRule& k : rules) compare(planes(rng, n, rlen, true), n, rlen, k), compare(planes(rng, n, rlen, false), n, rlen, k);
    {  // a gap and a block of 4100 rows across a batch edge; of 8500 rows across two; whole words and whole batches of set bits
        for (uint32_t rlen : {4200u, 9000u}) {
            const uint32_t n = 12, rows = rlen + 1u, len = rlen == 4200u ? 4100u : 8500u;
            std::vector<uint8_t> b = planes(rng, n, rlen, false);
            for (uint32_t i = 0; i < 5; ++i) std::fill(b.begin() + size_t(i) * rows + 50, b.begin() + size_t(i) * rows + 50 + len, uint8_t(IOC_ALLELE_DEL));
            std::fill(b.begin() + 6 * size_t(rows) + 4096, b.begin() + 6 * size_t(rows) + 4160, uint8_t(IOC_ALLELE_DEL));
            for (const BlocksRule& k : rules) compare(b, n, rlen, k);
            compare(b, n, rlen, BlocksRule{4100, 3, 3, 25, 4100, 32});
            compare(b, n, rlen, BlocksRule{8500, 3, 3, 25, 8500, 32});
            compare(b, n, rlen, BlocksRule{8501, 3, 3, 25, 10, 32});
            compare(b, n, rlen, BlocksRule{INT32_MAX, 3, 3, 25, INT32_MAX, 32});
        }
    }
    {  // 35 blocks under max_blocks 32; the keys of two groups of reads differ at block 31 alone, skip and part: bit 63
        const uint32_t n = 64, rlen = 2000, rows = rlen + 1u;
        std::vector<uint8_t> b(size_t(n) * rows, 0);
        for (uint32_t i = 0; i < n; ++i) b[size_t(i) * rows + rlen] = uint8_t(IOC_ALLELE_NONE);
        for (uint32_t k = 0; k < 35; ++k)
            for (uint32_t i = 0; i < 40; ++i)
                std::fill(b.begin() + size_t(i) * rows + 50 * k + 10, b.begin() + size_t(i) * rows + 50 * k + 10 + (i >= 20 && k == 31 ? 12 : 25), uint8_t(IOC_ALLELE_DEL));
        compare(b, n, rlen, rules[0]);
        const Result r = restated(b, n, rlen, rules[0]);
        EXPECT(r.seg.n_found == 35 && r.seg.n_blocks == 32 && r.seg.n_groups == 3);
        EXPECT(r.reads[40].group == 0 && r.reads[0].group == 1 && r.reads[20].group == 2 && (r.reads[20].key >> 63) == 1);
        compare(b, n, rlen, BlocksRule{20, 3, 3, 25, 10, 1});
    }
    EXPECT(long_runs_seen > 1000 && batches_crossed > 0 && blocks_seen > 100);
    EXPECT(hows_seen[0] > 0 && hows_seen[1] > 0 && hows_seen[2] > 0 && hows_seen[3] > 0);
    if (faults) {
        fprintf(stderr, "%d checks failed\n", faults);
        return 1;
    }
    printf("ok (%lld long gaps, %lld blocks, %lld whole batches read ahead; direct %lld assigned %lld rare %lld ambiguous %lld)\n", long_runs_seen, blocks_seen,
           batches_crossed, hows_seen[0], hows_seen[1], hows_seen[2], hows_seen[3]);
    return 0;
}
