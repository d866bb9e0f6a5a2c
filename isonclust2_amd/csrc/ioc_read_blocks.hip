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
//   k_block_rows     a wave per 64 rows of a segment, a lane per row: the segment's members 64 at a time (member_row_counts,
//                    ioc_read_stage.h) — depth, in_gap and, by ballot, the word of variable rows.
//   k_block_list     a wave per segment sweeps the variable-row words with the same run logic at min_block (RunSweep, below): the
//                    k-th start and the k-th end of the long runs are block k (run_slots_put); the first max_blocks are written.
//   k_read_states    a wave per pair, a lane per kept block: masked popcounts of the covered and the deleted words
//                    (masked_counts), the state, and the key and its mask by an OR over the wave.
//   k_key_support    a wave per read, lanes over the segment's reads: how many complete reads carry its key, and whether it is the
//                    first of them (key_support).
//   k_read_isoforms  a wave per read: its key's rank among the first occurrences of supported keys (unsigned compares) or, incomplete,
//                    the supported keys that agree with it under its mask and the rank of the single one (key_isoform).
//   k_blocks_record  a wave per segment: the counts of the record and, a lane per block, the four state counts of every kept block
//                    (key_tallies).
// The last three are the one-word case of ioc_read_stage.h's two-word keys: the major word is absent and compiled away.
// No atomics and no LDS: every output byte has one writer and is a function of the inputs alone.  Every plane byte, word, table row
// and record is held against the sizes passed.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ioc_internal.h"
#include "ioc_read_blocks.h"
#include "ioc_read_stage.h"

namespace {

constexpr uint32_t WAVES = IOC_READ_BLOCKS_WAVES;
typedef unsigned long long u64;

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
    const uint2 n = member_row_counts(v, g, c, v.cov, v.gap, lane);
    const uint32_t depth = n.x, in = n.y;
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
        run_slots_put(run_starts(sw.q, sw.left), run_ends(sw.q, sw.right), (b0 + lane) * 64u, lane, base_s, base_e, v.blocks, bb, v.n_block_slots, most);
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
        const uint2 n = masked_counts(v.cov, v.del, w0, v.n_pair_words, W, first, end);
        const uint32_t st = blocks_state(uint32_t(end - first), n.x, n.y);
        key = u64(st) << (2u * lane), mask = blocks_state_mask(lane, st);
    }
    key = wave_or64(key), mask = wave_or64(mask);
    if (lane == 0) v.reads[i].key = key, v.mask[i] = mask;
}

__global__ void __launch_bounds__(64 * WAVES)
k_key_support(IocReadBlocksDev v, BlocksRule rule)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;
    const uint8_t flags = key_support(v, i, g, blocks_full_mask(uint32_t(v.seg_out[g].n_blocks)), uint32_t(rule.min_alt), lane);
    if (lane == 0) v.flags[i] = flags;
}

__global__ void __launch_bounds__(64 * WAVES)
k_read_isoforms(IocReadBlocksDev v)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;
    const KeyIsoform r = key_isoform(v, i, g, blocks_full_mask(uint32_t(v.seg_out[g].n_blocks)), lane);
    if (lane == 0) v.reads[i].group = r.group, v.reads[i].how = r.how;
}

__global__ void __launch_bounds__(64 * WAVES)
k_blocks_record(IocReadBlocksDev v)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (g >= v.n_segs) return;
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u], nb = min(uint32_t(v.seg_out[g].n_blocks), uint32_t(IOC_BLOCKS_MAX));
    const u64 bb = u64(v.block_base[g]);
    const KeyTallies t = key_tallies(v, mb, me, nb, lane);
    if (lane == 0) {
        ioc_blocks_seg* r = v.seg_out + g;
        r->n_groups = int32_t(t.groups), r->n_reads = int32_t(me - mb), r->n_direct = int32_t(t.how_n[IOC_ISO_DIRECT]), r->n_assigned = int32_t(t.how_n[IOC_ISO_ASSIGNED]),
        r->n_rare = int32_t(t.how_n[IOC_ISO_RARE]), r->n_ambiguous = int32_t(t.how_n[IOC_ISO_AMBIGUOUS]);
    }
    if (lane < nb && bb + lane < v.n_block_slots) {
        ioc_pile_block* b = v.blocks + bb + lane;
        b->n_keep = t.state_n[IOC_BLOCK_KEEP], b->n_skip = t.state_n[IOC_BLOCK_SKIP], b->n_part = t.state_n[IOC_BLOCK_PART], b->n_none = t.state_n[IOC_BLOCK_NONE];
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
