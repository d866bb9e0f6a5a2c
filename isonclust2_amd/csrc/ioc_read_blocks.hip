// ioc_read_blocks.hip — the exon blocks of every segment of a call and every read's isoform, from the reads' base planes where they
// lie (ioc_planes_blocks, ioc_align_pairs_blocks; the definition is ioc_host_planes_blocks, ioc_align.cpp).
//
// Eight kernels in a row on one stream, a wave per item, IOC_READ_BLOCKS_WAVES items per workgroup; nothing is shared between the
// waves of a workgroup, so there is no barrier and a wave either runs whole or returns.  What one kernel hands to the next goes
// through global memory between two launches; inside a kernel no word passes from lane to lane except by ballot and shuffle.
//   k_plane_bits     a wave per pair, a lane per row in chunks of 64: __ballot turns a chunk of the byte plane into a covered word and a
//                    deleted word; lane w keeps word w of 64 and the wave writes 64 words at a time.  From here on nobody reads a byte.
//   k_gap_words      a wave per pair, lane w holds deleted word w of a batch of 64 (4096 rows): the long-gap word (run_long_bits,
//                    ioc_read_blocks.h) needs the run's length across any number of words — the nearest word with a clear bit on
//                    either side, found in the ballot of "has a clear bit", says how far the run reaches inside the batch; beyond the
//                    batch a saturated carry comes in from the left, and from the right by reading ahead until a clear bit or min_gap
//                    rows.  Also the read's extent and its gap counters.
//   k_block_rows     a wave per 64 rows of a segment, a lane per row: the segment's members 64 at a time — lane j fetches member j's
//                    two words, and row by row a ballot counts the members that have the row's bit, which lane r keeps — depth,
//                    in_gap and, by ballot, the word of variable rows.
//   k_block_list     a wave per segment sweeps the variable-row words with the same run logic at min_block: the k-th start and the
//                    k-th end of the long runs are block k; ranks by a wave scan and a running base; the first max_blocks are written.
//   k_read_states    a wave per pair, a lane per kept block: masked popcounts of the covered and the deleted words, the state, and
//                    the key and its mask by an OR over the wave.
//   k_key_support    a wave per read, lanes over the segment's reads: how many complete reads carry its key, and whether it is the
//                    first of them.
//   k_read_isoforms  a wave per read: its key's rank among the first occurrences of supported keys (unsigned compares) or, incomplete,
//                    the supported keys that agree with it under its mask and the rank of the single one.
//   k_blocks_record  a wave per segment: the counts of the record and, a lane per block, the four state counts of every kept block.
// No atomics and no LDS: every output byte has one writer and is a function of the inputs alone.  Every plane byte, word, table row
// and record is held against the sizes passed.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ioc_internal.h"
#include "ioc_read_blocks.h"

namespace {

constexpr uint32_t WAVES = IOC_READ_BLOCKS_WAVES;
typedef unsigned long long u64;

__device__ __forceinline__ u64 shfl64(u64 v, uint32_t src)
{
    const uint32_t lo = uint32_t(__shfl(int(uint32_t(v)), int(src), 64)), hi = uint32_t(__shfl(int(uint32_t(v >> 32)), int(src), 64));
    return u64(hi) << 32 | lo;
}
__device__ __forceinline__ uint32_t shfl32(uint32_t v, uint32_t src) { return uint32_t(__shfl(int(v), int(src), 64)); }

__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t up = uint32_t(__shfl_up(int(v), d, 64));
        if (lane >= d) v += up;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) v += uint32_t(__shfl_xor(int(v), int(d), 64));
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) v = min(v, uint32_t(__shfl_xor(int(v), int(d), 64)));
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) v = max(v, uint32_t(__shfl_xor(int(v), int(d), 64)));
    return v;
}
__device__ __forceinline__ u64 wave_or64(u64 v)
{
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) {
        const uint32_t lo = uint32_t(__shfl_xor(int(uint32_t(v)), int(d), 64)), hi = uint32_t(__shfl_xor(int(uint32_t(v >> 32)), int(d), 64));
        v |= u64(hi) << 32 | lo;
    }
    return v;
}

__device__ __forceinline__ uint32_t seg_words(const IocPileSeg& s) { return uint32_t(s.rlen) / 64u + 1u; }  // ceil((rlen + 1) / 64)

// The sweep of one plane of W words from `words` on (n_words: what the buffer holds) for its runs of at least `least` set bits, 64
// words a batch, lane w word w.  next() loads the batch at b0 and works out what the run logic needs; every lane of the wave takes
// every step: there are ballots and shuffles in it.
struct RunSweep {
    const u64* __restrict__ words;
    u64 at, n_words;
    uint32_t W, least, lane;
    uint32_t carry = 0;  // the set bits that end right below the batch, saturated
    u64 w = 0, q = 0;    // lane's word and its bits that stand in long runs
    uint32_t left = 0, right = 0;

    __device__ __forceinline__ u64 load(uint32_t i) const { return i < W && at + i < n_words ? words[at + i] : 0ull; }
    __device__ __forceinline__ void next(uint32_t b0)
    {
        w = load(b0 + lane);
        const u64 nonfull = __ballot(~w != 0ull);
        uint32_t ahead = 0;  // the set bits that begin right above the batch, read as far as `least` asks
        for (uint32_t nb = b0 + 64u; nb < W; nb += 64u) {
            const u64 x = load(nb + lane);
            const u64 nf = __ballot(~x != 0ull);
            if (nf) {
                const uint32_t j = uint32_t(__builtin_ctzll(nf));
                ahead = run_sat(u64(ahead) + 64ull * j + shfl32(run_lead(x), j), least);
                break;
            }
            ahead = run_sat(u64(ahead) + 4096ull, least);
            if (ahead >= least) break;
        }
        const uint32_t below = run_src_below(nonfull, lane), above = run_src_above(nonfull, lane);
        const uint32_t t_below = shfl32(run_trail(w), below & 63u), l_above = shfl32(run_lead(w), above & 63u);
        left = run_left_in(lane, below, t_below, carry, least);
        right = run_right_in(lane, above, l_above, ahead, least);
        q = run_long_bits(w, left, right, least);
        if (nonfull) {
            const uint32_t j = 63u - uint32_t(__builtin_clzll(nonfull));
            carry = run_sat(64ull * (63u - j) + shfl32(run_trail(w), j), least);
        } else {
            carry = run_sat(4096ull + carry, least);
        }
    }
};

__global__ void __launch_bounds__(64 * WAVES)
k_plane_bits(IocReadBlocksDev v)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;  // (whole waves: there is no barrier below)
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;  // (the entry points refuse such a pair)
    const IocPileSeg s = v.segs[g];
    const uint32_t rlen = uint32_t(s.rlen), W = seg_words(s);
    const u64 po = v.plane[i], w0 = v.pair_word[i];
    for (uint32_t b0 = 0; b0 < W; b0 += 64u) {
        u64 mine_c = 0, mine_d = 0;
        const uint32_t stop = min(b0 + 64u, W);
        for (uint32_t c = b0; c < stop; ++c) {
            const u64 p = u64(c) * 64u + lane;
            const uint8_t b = p < rlen && po + p < v.plane_bytes ? v.base_planes[po + p] : uint8_t(IOC_ALLELE_NONE);
            const u64 cw = __ballot(blocks_covers(b)), dw = __ballot(b == uint8_t(IOC_ALLELE_DEL));
            if (lane == c - b0) mine_c = cw, mine_d = dw;
        }
        const uint32_t w = b0 + lane;
        if (w < W && w0 + w < v.n_pair_words) v.cov[w0 + w] = mine_c, v.del[w0 + w] = mine_d;
    }
}

__global__ void __launch_bounds__(64 * WAVES)
k_gap_words(IocReadBlocksDev v, BlocksRule rule)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;
    const uint32_t W = seg_words(v.segs[g]);
    const u64 w0 = v.pair_word[i];
    RunSweep sw{v.del, w0, v.n_pair_words, W, uint32_t(rule.min_gap), lane};
    uint32_t n_gaps = 0, gap_rows = 0, first = 0xFFFFFFFFu, end = 0;
    for (uint32_t b0 = 0; b0 < W; b0 += 64u) {
        sw.next(b0);
        const uint32_t w = b0 + lane;
        if (w < W && w0 + w < v.n_pair_words) {
            v.gap[w0 + w] = sw.q;
            const u64 cw = v.cov[w0 + w];
            if (cw) first = min(first, w * 64u + uint32_t(__builtin_ctzll(cw))), end = max(end, w * 64u + 64u - uint32_t(__builtin_clzll(cw)));
        }
        n_gaps += uint32_t(__popcll(run_starts(sw.q, sw.left)));
        gap_rows += uint32_t(__popcll(sw.q));
    }
    n_gaps = wave_sum(n_gaps), gap_rows = wave_sum(gap_rows), first = wave_min(first), end = wave_max(end);
    if (lane == 0) {
        ioc_read_blocks* r = v.reads + i;
        r->first_row = end ? int32_t(first) : 0, r->end_row = int32_t(end), r->n_gaps = int32_t(n_gaps), r->gap_rows = int32_t(gap_rows);
    }
}

__global__ void __launch_bounds__(64 * WAVES)
k_block_rows(IocReadBlocksDev v, BlocksRule rule)
{
    const uint32_t lane = threadIdx.x & 63u;
    const u64 t = u64(blockIdx.x) * WAVES + (threadIdx.x >> 6);
    if (t >= v.n_seg_words) return;
    const uint32_t g = uint32_t(v.word_seg[t]);
    if (g >= v.n_segs) return;
    const IocPileSeg s = v.segs[g];
    const u64 c = t - v.seg_word[g];
    const u64 p = c * 64u + lane;
    uint32_t depth = 0, in = 0;
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u];
    for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
        u64 cw = 0, gw = 0;
        if (m0 + lane < me) {
            const uint32_t i = v.members[m0 + lane];
            const u64 w = i < v.n_pairs ? v.pair_word[i] + c : v.n_pair_words;
            if (w < v.n_pair_words) cw = v.cov[w], gw = v.gap[w];
        }
        for (uint32_t r = 0; r < 64u; ++r) {  // (row r of the chunk: how many of the 64 members have its bit; lane r keeps the sum)
            const uint32_t d = uint32_t(__popcll(__ballot((cw >> r) & 1ull))), gp = uint32_t(__popcll(__ballot((gw >> r) & 1ull)));
            if (lane == r) depth += d, in += gp;
        }
    }
    const bool has_base = p < u64(uint32_t(s.rlen));
    if (p <= u64(uint32_t(s.rlen)) && u64(s.row0) + p < v.n_rows) v.rows[u64(s.row0) + p] = ioc_block_row{depth, in};
    const u64 var = __ballot(has_base && blocks_row_variable(rule, depth, in));
    if (lane == 0) v.var[t] = var;
}

__global__ void __launch_bounds__(64 * WAVES)
k_block_list(IocReadBlocksDev v, BlocksRule rule)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (g >= v.n_segs) return;
    const uint32_t W = seg_words(v.segs[g]), most = uint32_t(rule.max_blocks);
    const u64 bb = u64(v.block_base[g]);
    RunSweep sw{v.var, v.seg_word[g], v.n_seg_words, W, uint32_t(rule.min_block), lane};
    uint32_t base_s = 0, base_e = 0;  // the starts and the ends of long runs below the batch
    for (uint32_t b0 = 0; b0 < W; b0 += 64u) {
        sw.next(b0);
        u64 st = run_starts(sw.q, sw.left), en = run_ends(sw.q, sw.right);
        const uint32_t ns = uint32_t(__popcll(st)), ne = uint32_t(__popcll(en));
        const uint32_t is = wave_scan_incl(ns, lane), ie = wave_scan_incl(ne, lane);
        const uint32_t row = (b0 + lane) * 64u;
        for (uint32_t k = base_s + is - ns; st && k < most; ++k, st &= st - 1ull)
            if (bb + k < v.n_block_slots) v.blocks[bb + k].first = int32_t(row + uint32_t(__builtin_ctzll(st)));
        for (uint32_t k = base_e + ie - ne; en && k < most; ++k, en &= en - 1ull)
            if (bb + k < v.n_block_slots) v.blocks[bb + k].end = int32_t(row + uint32_t(__builtin_ctzll(en)) + 1u);
        base_s += shfl32(is, 63), base_e += shfl32(ie, 63);
    }
    if (lane == 0) v.seg_out[g].n_blocks = int32_t(min(base_s, most)), v.seg_out[g].n_found = int32_t(base_s);
}

__global__ void __launch_bounds__(64 * WAVES)
k_read_states(IocReadBlocksDev v)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;
    const uint32_t W = seg_words(v.segs[g]), nb = uint32_t(v.seg_out[g].n_blocks);
    const u64 bb = u64(v.block_base[g]), w0 = v.pair_word[i];
    u64 key = 0, mask = 0;
    if (lane < nb && lane < uint32_t(IOC_BLOCKS_MAX) && bb + lane < v.n_block_slots) {
        const long long first = v.blocks[bb + lane].first, end = v.blocks[bb + lane].end;
        uint32_t c = 0, s = 0;
        for (long long w = first / 64; w * 64 < end && w < (long long)W; ++w) {
            const u64 m = run_row_mask(w * 64, first, end);
            if (w0 + u64(w) < v.n_pair_words) c += uint32_t(__popcll(v.cov[w0 + u64(w)] & m)), s += uint32_t(__popcll(v.del[w0 + u64(w)] & m));
        }
        const uint32_t st = blocks_state(uint32_t(end - first), c, s);
        key = u64(st) << (2u * lane), mask = blocks_state_mask(lane, st);
    }
    key = wave_or64(key), mask = wave_or64(mask);
    if (lane == 0) v.reads[i].key = key, v.mask[i] = mask;
}

// what a wave reads of member m of its segment (lane's member of a chunk): the pair, its key and mask, its flags
struct Member {
    uint32_t pair = 0xFFFFFFFFu;
    u64 key = 0, mask = 0;
    uint32_t flags = 0;
    bool there = false;
};
__device__ __forceinline__ Member member_at(const IocReadBlocksDev& v, uint32_t m, uint32_t me, bool with_flags)
{
    Member x;
    if (m >= me) return x;
    x.pair = v.members[m];
    if (x.pair >= v.n_pairs) return x;
    x.there = true, x.key = v.reads[x.pair].key, x.mask = v.mask[x.pair];
    if (with_flags) x.flags = v.flags[x.pair];
    return x;
}

enum : uint32_t { KEY_SUPPORTED = 1, KEY_FIRST = 2 };

__global__ void __launch_bounds__(64 * WAVES)
k_key_support(IocReadBlocksDev v, BlocksRule rule)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;
    const u64 full = blocks_full_mask(uint32_t(v.seg_out[g].n_blocks)), key = v.reads[i].key;
    const bool complete = v.mask[i] == full;
    uint32_t same = 0, earlier = 0;
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u];
    for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
        const Member x = member_at(v, m0 + lane, me, false);
        const bool hit = x.there && x.mask == full && x.key == key;
        same += uint32_t(__popcll(__ballot(hit)));
        earlier += uint32_t(__popcll(__ballot(hit && x.pair < i)));  // (a segment's reads are its pairs in ascending order)
    }
    if (lane == 0) v.flags[i] = uint8_t(complete && same >= uint32_t(rule.min_alt) ? KEY_SUPPORTED | (earlier == 0u ? KEY_FIRST : 0u) : 0u);
}

// the rank of `key` among the first occurrences of the supported keys of the segment: the isoform's number
__device__ __forceinline__ uint32_t key_rank(const IocReadBlocksDev& v, uint32_t mb, uint32_t me, u64 key, uint32_t lane)
{
    uint32_t rank = 0;
    for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
        const Member x = member_at(v, m0 + lane, me, true);
        rank += uint32_t(__popcll(__ballot(x.there && (x.flags & KEY_FIRST) && x.key < key)));  // (unsigned)
    }
    return rank;
}

__global__ void __launch_bounds__(64 * WAVES)
k_read_isoforms(IocReadBlocksDev v)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;
    const u64 full = blocks_full_mask(uint32_t(v.seg_out[g].n_blocks)), key = v.reads[i].key, mask = v.mask[i];
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u];
    int32_t group = -1, how;
    if (mask == full) {  // (uniform over the wave, like everything it branches on below)
        how = (v.flags[i] & KEY_SUPPORTED) ? IOC_ISO_DIRECT : IOC_ISO_RARE;
        if (how == IOC_ISO_DIRECT) group = int32_t(key_rank(v, mb, me, key, lane));
    } else {
        uint32_t agreeing = 0;
        u64 which = 0;
        for (uint32_t m0 = mb; m0 < me && mask != 0ull; m0 += 64u) {
            const Member x = member_at(v, m0 + lane, me, true);
            const u64 hits = __ballot(x.there && (x.flags & KEY_FIRST) && blocks_key_agrees(key, x.key, mask));
            if (hits && agreeing == 0u) which = shfl64(x.key, uint32_t(__builtin_ctzll(hits)));
            agreeing += uint32_t(__popcll(hits));
        }
        how = agreeing == 1u ? IOC_ISO_ASSIGNED : IOC_ISO_AMBIGUOUS;
        if (agreeing == 1u) group = int32_t(key_rank(v, mb, me, which, lane));
    }
    if (lane == 0) v.reads[i].group = group, v.reads[i].how = how;
}

__global__ void __launch_bounds__(64 * WAVES)
k_blocks_record(IocReadBlocksDev v)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (g >= v.n_segs) return;
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u], nb = uint32_t(v.seg_out[g].n_blocks);
    const u64 bb = u64(v.block_base[g]);
    uint32_t groups = 0, how_n[4] = {0, 0, 0, 0}, state_n[4] = {0, 0, 0, 0};
    for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
        const Member x = member_at(v, m0 + lane, me, true);
        const uint32_t how = x.there ? uint32_t(v.reads[x.pair].how) : 4u;
        groups += uint32_t(__popcll(__ballot(x.there && (x.flags & KEY_FIRST))));
#pragma unroll
        for (uint32_t h = 0; h < 4u; ++h) how_n[h] += uint32_t(__popcll(__ballot(how == h)));
        for (uint32_t b = 0; b < nb && b < uint32_t(IOC_BLOCKS_MAX); ++b) {  // (block b: how many of the 64 members are in each state; lane b keeps the sums)
            const uint32_t st = uint32_t(x.key >> (2u * b)) & 3u;
#pragma unroll
            for (uint32_t h = 0; h < 4u; ++h) {
                const uint32_t n = uint32_t(__popcll(__ballot(x.there && st == h)));
                if (lane == b) state_n[h] += n;
            }
        }
    }
    if (lane == 0) {
        ioc_blocks_seg* r = v.seg_out + g;
        r->n_groups = int32_t(groups), r->n_reads = int32_t(me - mb), r->n_direct = int32_t(how_n[IOC_ISO_DIRECT]), r->n_assigned = int32_t(how_n[IOC_ISO_ASSIGNED]),
        r->n_rare = int32_t(how_n[IOC_ISO_RARE]), r->n_ambiguous = int32_t(how_n[IOC_ISO_AMBIGUOUS]);
    }
    if (lane < nb && lane < uint32_t(IOC_BLOCKS_MAX) && bb + lane < v.n_block_slots) {
        ioc_pile_block* b = v.blocks + bb + lane;
        b->n_keep = state_n[IOC_BLOCK_KEEP], b->n_skip = state_n[IOC_BLOCK_SKIP], b->n_part = state_n[IOC_BLOCK_PART], b->n_none = state_n[IOC_BLOCK_NONE];
        b->reserved[0] = 0, b->reserved[1] = 0;
    }
}

}  // namespace

static_assert(sizeof(ioc_block_row) == 8 && sizeof(ioc_pile_block) == 32 && sizeof(ioc_read_blocks) == 32 && sizeof(ioc_blocks_seg) == 32,
              "the records are laid out as the public ones");

// The eight kernels over the view, in a row on `st`.  The caller has set v.reads and v.seg_out to 0.
hipError_t iock_read_blocks(hipStream_t st, const IocReadBlocksDev& v, int32_t min_gap, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                            int32_t min_block, int32_t max_blocks)
{
    const BlocksRule rule{min_gap, min_depth, min_alt, min_pct, min_block, max_blocks};
    if (v.n_segs == 0) return hipSuccess;
    auto grid = [](uint64_t items) { return dim3(uint32_t((items + WAVES - 1u) / WAVES)); };
    const dim3 block(64 * WAVES);
    if (v.n_pairs) hipLaunchKernelGGL(k_plane_bits, grid(v.n_pairs), block, 0, st, v);
    if (v.n_pairs) hipLaunchKernelGGL(k_gap_words, grid(v.n_pairs), block, 0, st, v, rule);
    if (v.n_seg_words) hipLaunchKernelGGL(k_block_rows, grid(v.n_seg_words), block, 0, st, v, rule);
    hipLaunchKernelGGL(k_block_list, grid(v.n_segs), block, 0, st, v, rule);
    if (v.n_pairs) hipLaunchKernelGGL(k_read_states, grid(v.n_pairs), block, 0, st, v);
    if (v.n_pairs) hipLaunchKernelGGL(k_key_support, grid(v.n_pairs), block, 0, st, v, rule);
    if (v.n_pairs) hipLaunchKernelGGL(k_read_isoforms, grid(v.n_pairs), block, 0, st, v);
    hipLaunchKernelGGL(k_blocks_record, grid(v.n_segs), block, 0, st, v);
    return hipGetLastError();
}
