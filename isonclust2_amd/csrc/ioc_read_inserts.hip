// ioc_read_inserts.hip — the insertion sites of every segment of a call and every read's combined isoform, from the reads' base and
// length planes where they lie (ioc_planes_inserts, ioc_align_pairs_blocks_inserts; the definitions are ioc_host_ops_project_ilen
// and ioc_host_planes_inserts, ioc_align.cpp).
//
//   k_ops_project_ilen  beside k_ops_project_ins (ioc_plane_pile.hip), over the same bytes of a slice: one wave per pair repeats that
//                       kernel's walk with PileAcc.  The lane of the byte BEHIND a run of 'I' — the first byte that is no 'I', be it
//                       a byte of the string or the 0 behind its end — stores min(run, 255) at the run's row: ins_index of that lane
//                       is the run's length, open_len carries it across steps.  A run that ends with the last byte of the last chunk
//                       has no byte behind it: lane 0 stores it after the walk.  A row takes one run, so every byte has one writer:
//                       plain byte stores, no atomics, and a re-run rewrites what it wrote.
// Eight kernels in a row on one stream behind it, a wave per item, IOC_READ_INSERTS_WAVES items per workgroup; nothing is shared
// between the waves of a workgroup, so there is no barrier and a wave either runs whole or returns.
//   k_ins_bits       a wave per pair, a lane per junction in chunks of 64: the span word is covered AND covered-shifted-by-one, the
//                    shifted-in bit carried from chunk to chunk; W(p) comes from two wave prefix sums, over the chunk's 64 length
//                    bytes and over a halo of 32 on either side (window_sums): two byte loads a lane and chunk, not 2 slack + 1.  The
//                    near word is the ballot of "spans and W >= min_ins".  Lane w keeps word w of 64, the wave writes 64 words at a
//                    time; also the read's n_near and ins_bases.
//   k_ins_rows       a wave per 64 junctions of a segment, the members 64 at a time as k_block_rows has it: span, in_ins and, by
//                    ballot, the word of variable junctions.
//   k_ins_list       a wave per segment sweeps the variable words for runs of any length: a run goes on across a word where the
//                    neighbour's edge bit is set (run_starts / run_ends, ioc_read_blocks.h), across a batch by a carried bit and one
//                    word read ahead; ranks by a wave scan and a running base; the first max_sites are written.
//   k_ins_states     a wave per pair, a lane per kept site: masked popcounts of the span and the near words, the state, and the key
//                    and its mask by an OR over the wave.  Then site by site where the pair carries: its largest W over the site's
//                    junctions (window_sums again, the only plane bytes read after k_ins_bits), which lane k keeps and stores as 16
//                    bits (at most 65 x 255) at the pair's place of a scratch table, max_sites entries a pair.
//   k_ins_lens       a wave per kept site over the segment's members, 64 at a time: the smallest and the largest of the carriers'
//                    entries.  (A first form computed W here, a wave per site walking its carriers one after the other: 0.83 ms for
//                    600 carriers of two sites, against 0.02 ms of everything else the two kernels do.)
//   k_ins_support, k_ins_isoforms, k_ins_record
//                    k_key_support, k_read_isoforms and k_blocks_record on two-word keys (the block stage's word, read where that
//                    stage left it, and this stage's): unsigned compares, major word first.
// No atomics and no LDS: every output byte has one writer and is a function of the inputs alone.  Every plane byte, word, table row
// and record is held against the sizes passed.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ioc_internal.h"
#include "ioc_ops_pileup.h"
#include "ioc_read_inserts.h"

namespace {

constexpr uint32_t WAVES = IOC_READ_INSERTS_WAVES;
constexpr int OP_WAVES = 4;  // pairs per workgroup of k_ops_project_ilen (nothing is shared between them)
typedef unsigned long long u64;

__global__ void __launch_bounds__(64 * OP_WAVES)
k_ops_project_ilen(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ end, const uint32_t* __restrict__ len,
                   const uint32_t* __restrict__ room, const uint32_t* __restrict__ ord, uint32_t cnt, const int64_t* __restrict__ row_base,
                   const uint64_t* __restrict__ plane, uint8_t* __restrict__ ilen_planes, uint64_t plane_bytes)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t x = blockIdx.x * OP_WAVES + (threadIdx.x >> 6);
    if (x >= cnt) return;  // (whole waves: there is no barrier below)
    const uint32_t pid = ord[x];
    const uint64_t L = len[pid], e = end[pid];
    if (L == 0 || L > room[pid] || L > e) return;  // came back without an answer: left to its re-run (as k_ops_project has it)
    if (row_base[pid] < 0) return;                 // (piled and projected by an earlier run of this call already)
    const uint64_t po = plane[pid];

    const uint8_t* first = buf + (e - L);
    const uint32_t head = uint32_t(reinterpret_cast<uintptr_t>(first) & 3u);
    const uint32_t* words = reinterpret_cast<const uint32_t*>(first - head);
    const uint32_t span = head + uint32_t(L);
    const uint32_t nwords = (span + 3u) / 4u, nchunks = (nwords + 63u) / 64u;

    PileAcc acc;
    uint32_t w = lane < nwords ? words[lane] : 0u;
    for (uint32_t c = 0; c < nchunks; ++c) {
        const uint32_t nx = (c + 1u) * 64u + lane;
        const uint32_t w_next = nx < nwords ? words[nx] : 0u;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t pos = c * 256u + j * 64u + lane;
            const uint32_t v = uint32_t(__shfl(int(w), int(16u * j + (lane >> 2)), 64));
            const uint32_t b = (pos >= head && pos < span) ? (v >> (8u * (lane & 3u))) & 0xFFu : 0u;
            acc.begin(__ballot(b == uint32_t('=')), __ballot(b == uint32_t('X')), __ballot(b == uint32_t('I')), __ballot(b == uint32_t('D')),
                      __ballot(b == uint32_t('i')), __ballot(b == uint32_t('d')));
            // the byte behind a run: no 'I' itself, the byte below it one (below lane 0: the step before ended in one)
            const bool behind = !acc.is_ins(lane) && (lane ? acc.is_ins(lane - 1u) : acc.open_len != 0u);
            if (behind) {
                const uint64_t at_row = po + acc.row(lane);
                if (at_row < plane_bytes) ilen_planes[at_row] = inserts_len_byte(acc.ins_index(lane));
            }
            acc.end_len();
            acc.end();
        }
        w = w_next;
    }
    if (lane == 0u && acc.open_len != 0u && po + acc.r < plane_bytes) ilen_planes[po + acc.r] = inserts_len_byte(acc.open_len);
}

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

// W(p0 + lane) of the pair whose length plane begins at byte po, and own = its byte at p0 + lane.  Every lane of the wave takes
// part.  A[0 .. 128) = the 32 bytes below p0, the 64 from p0 on, the 32 behind them (0 outside rows 0 .. rlen, so the window needs
// no clamping); sV and sH are the inclusive prefix sums of the middle and of the halo (lanes 0 .. 31 the left half), and the
// inclusive prefix of A at idx is sH[idx], sH[31] + sV[idx - 32] or sV[63] + sH[idx - 64].  W = prefix(32 + lane + slack) -
// prefix(32 + lane - slack - 1); slack <= 32 keeps both inside -1 .. 127.  A sum is at most 128 x 255.
__device__ __forceinline__ uint32_t window_sums(const IocReadInsertsDev& v, u64 po, uint32_t rlen, long long p0, uint32_t slack, uint32_t lane, uint32_t& own)
{
    auto at = [&](long long q) -> uint32_t { return q >= 0 && q <= (long long)rlen && po + u64(q) < v.plane_bytes ? uint32_t(v.ilen_planes[po + u64(q)]) : 0u; };
    own = at(p0 + lane);
    const uint32_t halo = at(lane < 32u ? p0 - 32 + lane : p0 + 32 + lane);
    const uint32_t sV = wave_scan_incl(own, lane), sH = wave_scan_incl(halo, lane);
    const uint32_t left = shfl32(sH, 31u), mid = shfl32(sV, 63u);
    auto prefix = [&](int idx) -> uint32_t {
        const uint32_t fromH = shfl32(sH, uint32_t(idx < 32 ? idx : idx - 64) & 63u), fromV = shfl32(sV, uint32_t(idx - 32) & 63u);
        return idx < 0 ? 0u : idx < 32 ? fromH : idx < 96 ? left + fromV : mid + fromH;
    };
    const uint32_t hi = prefix(int(32u + lane + slack)), lo = prefix(int(32u + lane) - int(slack) - 1);
    return hi - lo;
}

__global__ void __launch_bounds__(64 * WAVES)
k_ins_bits(IocReadInsertsDev v, InsertsRule rule)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;  // (whole waves: there is no barrier below)
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;  // (the entry points refuse such a pair)
    const IocPileSeg s = v.segs[g];
    const uint32_t rlen = uint32_t(s.rlen), W = seg_words(s);
    const u64 po = v.plane[i], w0 = v.pair_word[i];
    u64 carry = 0;  // whether the row below the chunk is covered
    uint32_t n_near = 0, bases = 0;
    for (uint32_t b0 = 0; b0 < W; b0 += 64u) {
        u64 mine_s = 0, mine_n = 0;
        const uint32_t stop = min(b0 + 64u, W);
        for (uint32_t c = b0; c < stop; ++c) {
            const u64 p = u64(c) * 64u + lane;
            const uint8_t b = p < rlen && po + p < v.plane_bytes ? v.base_planes[po + p] : uint8_t(IOC_ALLELE_NONE);
            const u64 cw = __ballot(blocks_covers(b));
            const u64 sw = cw & (cw << 1 | carry);  // (junction 0 has carry 0 below it; junction rlen and beyond no covered row)
            carry = cw >> 63;
            uint32_t own;
            const uint32_t win = window_sums(v, po, rlen, (long long)c * 64, uint32_t(rule.slack), lane, own);
            const bool spans = (sw >> lane) & 1ull;
            const u64 nw = __ballot(spans && win >= uint32_t(rule.min_ins));
            n_near += uint32_t(__popcll(nw));
            if (spans) bases += own;
            if (lane == c - b0) mine_s = sw, mine_n = nw;
        }
        const uint32_t w = b0 + lane;
        if (w < W && w0 + w < v.n_pair_words) v.span[w0 + w] = mine_s, v.near[w0 + w] = mine_n;
    }
    bases = wave_sum(bases);
    if (lane == 0) v.reads[i].n_near = int32_t(n_near), v.reads[i].ins_bases = int32_t(bases);
}

__global__ void __launch_bounds__(64 * WAVES)
k_ins_rows(IocReadInsertsDev v, InsertsRule rule)
{
    const uint32_t lane = threadIdx.x & 63u;
    const u64 t = u64(blockIdx.x) * WAVES + (threadIdx.x >> 6);
    if (t >= v.n_seg_words) return;
    const uint32_t g = uint32_t(v.word_seg[t]);
    if (g >= v.n_segs) return;
    const IocPileSeg s = v.segs[g];
    const u64 c = t - v.seg_word[g];
    const u64 p = c * 64u + lane;
    uint32_t spanned = 0, in = 0;
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u];
    for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
        u64 sw = 0, nw = 0;
        if (m0 + lane < me) {
            const uint32_t i = v.members[m0 + lane];
            const u64 w = i < v.n_pairs ? v.pair_word[i] + c : v.n_pair_words;
            if (w < v.n_pair_words) sw = v.span[w], nw = v.near[w];
        }
        for (uint32_t r = 0; r < 64u; ++r) {  // (junction r of the chunk: how many of the 64 members have its bit; lane r keeps the sum)
            const uint32_t d = uint32_t(__popcll(__ballot((sw >> r) & 1ull))), np = uint32_t(__popcll(__ballot((nw >> r) & 1ull)));
            if (lane == r) spanned += d, in += np;
        }
    }
    const bool junction = p >= 1u && p + 1u <= u64(uint32_t(s.rlen));
    if (p <= u64(uint32_t(s.rlen)) && u64(s.row0) + p < v.n_rows) v.rows[u64(s.row0) + p] = ioc_insert_row{spanned, in};
    const u64 var = __ballot(junction && rule.variable(spanned, in));
    if (lane == 0) v.var[t] = var;
}

__global__ void __launch_bounds__(64 * WAVES)
k_ins_list(IocReadInsertsDev v)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (g >= v.n_segs) return;
    const uint32_t W = seg_words(v.segs[g]);
    const u64 sb = u64(v.site_base[g]), at = v.seg_word[g];
    const uint32_t most = uint32_t(u64(v.site_base[g + 1u]) - sb);  // min(max_sites, junctions)
    auto load = [&](uint32_t i) -> u64 { return i < W && at + i < v.n_seg_words ? v.var[at + i] : 0ull; };
    uint32_t base_s = 0, base_e = 0;  // the starts and the ends of runs below the batch
    u64 top = 0;                      // whether the junction right below the batch is variable
    for (uint32_t b0 = 0; b0 < W; b0 += 64u) {
        const u64 w = load(b0 + lane);
        const u64 dn = shfl64(w, (lane + 63u) & 63u), up = shfl64(w, (lane + 1u) & 63u);
        const uint32_t left = uint32_t(lane ? dn >> 63 : top), right = uint32_t((lane < 63u ? up : load(b0 + 64u)) & 1ull);
        u64 st = run_starts(w, left), en = run_ends(w, right);
        const uint32_t ns = uint32_t(__popcll(st)), ne = uint32_t(__popcll(en));
        const uint32_t is = wave_scan_incl(ns, lane), ie = wave_scan_incl(ne, lane);
        const uint32_t row = (b0 + lane) * 64u;
        for (uint32_t k = base_s + is - ns; st && k < most; ++k, st &= st - 1ull)
            if (sb + k < v.n_site_slots) v.sites[sb + k].first = int32_t(row + uint32_t(__builtin_ctzll(st)));
        for (uint32_t k = base_e + ie - ne; en && k < most; ++k, en &= en - 1ull)
            if (sb + k < v.n_site_slots) v.sites[sb + k].end = int32_t(row + uint32_t(__builtin_ctzll(en)) + 1u);
        base_s += shfl32(is, 63), base_e += shfl32(ie, 63);
        top = shfl64(w, 63u) >> 63;
    }
    if (lane == 0) v.seg_out[g].n_sites = int32_t(min(base_s, most)), v.seg_out[g].n_found = int32_t(base_s);
}

__global__ void __launch_bounds__(64 * WAVES)
k_ins_states(IocReadInsertsDev v, InsertsRule rule)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;
    const uint32_t W = seg_words(v.segs[g]), ns = uint32_t(v.seg_out[g].n_sites);
    const u64 sb = u64(v.site_base[g]), w0 = v.pair_word[i];
    u64 key = 0, mask = 0;
    if (lane < ns && lane < uint32_t(IOC_INSERTS_MAX) && sb + lane < v.n_site_slots) {
        const long long first = v.sites[sb + lane].first, end = v.sites[sb + lane].end;
        uint32_t c = 0, s = 0;
        for (long long w = first / 64; w * 64 < end && w < (long long)W; ++w) {
            const u64 m = run_row_mask(w * 64, first, end);
            if (w0 + u64(w) < v.n_pair_words) c += uint32_t(__popcll(v.span[w0 + u64(w)] & m)), s += uint32_t(__popcll(v.near[w0 + u64(w)] & m));
        }
        const uint32_t st = inserts_state(uint32_t(end - first), c, s);
        key = u64(st) << (2u * lane), mask = blocks_state_mask(lane, st);
    }
    // (here key is the lane's own state: a carried site is worked through by the whole wave, lane k keeps what comes out)
    const uint32_t rlen = uint32_t(v.segs[g].rlen);
    const u64 carried = __ballot(lane < ns && lane < uint32_t(IOC_INSERTS_MAX) && ((key >> (2u * lane)) & 3ull) == u64(IOC_INS_CARRY));
    long long my_first = 0, my_end = 0;
    if (lane < ns && lane < uint32_t(IOC_INSERTS_MAX) && sb + lane < v.n_site_slots) my_first = v.sites[sb + lane].first, my_end = v.sites[sb + lane].end;
    uint32_t mine = 0;
    for (u64 left = carried; left; left &= left - 1ull) {
        const uint32_t k = uint32_t(__builtin_ctzll(left));
        const long long first = (long long)shfl32(uint32_t(my_first), k), end = (long long)shfl32(uint32_t(my_end), k);
        uint32_t longest = 0, own;
        for (long long p0 = first; p0 < end; p0 += 64) {
            const uint32_t win = window_sums(v, v.plane[i], rlen, p0, uint32_t(rule.slack), lane, own);
            if (p0 + lane < end) longest = max(longest, win);
        }
        longest = wave_max(longest);
        if (lane == k) mine = longest;
    }
    if ((carried >> lane) & 1ull) {
        const u64 at = u64(i) * v.wmax_stride + lane;
        if (lane < v.wmax_stride && at < v.n_wmax) v.wmax[at] = uint16_t(mine);
    }
    key = wave_or64(key), mask = wave_or64(mask);
    if (lane == 0) v.reads[i].key = key, v.mask[i] = mask;
}

__global__ void __launch_bounds__(64 * WAVES)
k_ins_lens(IocReadInsertsDev v)
{
    const uint32_t lane = threadIdx.x & 63u;
    const u64 x = u64(blockIdx.x) * WAVES + (threadIdx.x >> 6);
    if (x >= v.n_site_slots) return;
    const uint32_t g = uint32_t(v.slot_seg[x]);
    if (g >= v.n_segs) return;
    const uint32_t k = uint32_t(x - u64(v.site_base[g]));
    if (k >= uint32_t(v.seg_out[g].n_sites) || k >= uint32_t(IOC_INSERTS_MAX)) return;
    uint32_t len_min = 0xFFFFFFFFu, len_max = 0;
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u];
    for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
        if (m0 + lane >= me) continue;  // (no ballot or shuffle inside the loop)
        const uint32_t i = v.members[m0 + lane];
        if (i >= v.n_pairs || ((v.reads[i].key >> (2u * k)) & 3ull) != u64(IOC_INS_CARRY)) continue;
        const u64 at = u64(i) * v.wmax_stride + k;
        if (k >= v.wmax_stride || at >= v.n_wmax) continue;
        const uint32_t longest = v.wmax[at];
        len_min = min(len_min, longest), len_max = max(len_max, longest);
    }
    len_min = wave_min(len_min), len_max = wave_max(len_max);
    if (lane == 0) v.sites[x].len_min = len_max ? len_min : 0u, v.sites[x].len_max = len_max;
}

// what a wave reads of member m of its segment (lane's member of a chunk): the pair, both words of its key and of its mask, its flags
struct Member {
    uint32_t pair = 0xFFFFFFFFu;
    u64 pre = 0, key = 0, pre_mask = 0, mask = 0;
    uint32_t flags = 0;
    bool there = false;
};
__device__ __forceinline__ u64 pre_key_of(const IocReadInsertsDev& v, uint32_t i) { return v.pre_key ? v.pre_key[u64(i) * v.pre_key_stride] : 0ull; }
__device__ __forceinline__ u64 pre_mask_of(const IocReadInsertsDev& v, uint32_t i) { return v.pre_mask ? v.pre_mask[u64(i) * v.pre_mask_stride] : 0ull; }
__device__ __forceinline__ u64 pre_full_of(const IocReadInsertsDev& v, uint32_t g) { return v.pre_full ? v.pre_full[g] : 0ull; }
__device__ __forceinline__ Member member_at(const IocReadInsertsDev& v, uint32_t m, uint32_t me, bool with_flags)
{
    Member x;
    if (m >= me) return x;
    x.pair = v.members[m];
    if (x.pair >= v.n_pairs) return x;
    x.there = true, x.key = v.reads[x.pair].key, x.mask = v.mask[x.pair], x.pre = pre_key_of(v, x.pair), x.pre_mask = pre_mask_of(v, x.pair);
    if (with_flags) x.flags = v.flags[x.pair];
    return x;
}

enum : uint32_t { KEY_SUPPORTED = 1, KEY_FIRST = 2 };

__global__ void __launch_bounds__(64 * WAVES)
k_ins_support(IocReadInsertsDev v, InsertsRule rule)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;
    const u64 full = blocks_full_mask(uint32_t(v.seg_out[g].n_sites)), pre_full = pre_full_of(v, g), key = v.reads[i].key, pre = pre_key_of(v, i);
    const bool complete = v.mask[i] == full && pre_mask_of(v, i) == pre_full;
    uint32_t same = 0, earlier = 0;
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u];
    for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
        const Member x = member_at(v, m0 + lane, me, false);
        const bool hit = x.there && x.mask == full && x.pre_mask == pre_full && x.key == key && x.pre == pre;
        same += uint32_t(__popcll(__ballot(hit)));
        earlier += uint32_t(__popcll(__ballot(hit && x.pair < i)));  // (a segment's reads are its pairs in ascending order)
    }
    if (lane == 0) v.flags[i] = uint8_t(complete && same >= uint32_t(rule.min_alt) ? KEY_SUPPORTED | (earlier == 0u ? KEY_FIRST : 0u) : 0u);
}

// the rank of (pre, key) among the first occurrences of the supported pairs of the segment: the isoform's number
__device__ __forceinline__ uint32_t key_rank(const IocReadInsertsDev& v, uint32_t mb, uint32_t me, u64 pre, u64 key, uint32_t lane)
{
    uint32_t rank = 0;
    for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
        const Member x = member_at(v, m0 + lane, me, true);
        rank += uint32_t(__popcll(__ballot(x.there && (x.flags & KEY_FIRST) && inserts_key_less(x.pre, x.key, pre, key))));  // (unsigned)
    }
    return rank;
}

__global__ void __launch_bounds__(64 * WAVES)
k_ins_isoforms(IocReadInsertsDev v)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;
    const u64 full = blocks_full_mask(uint32_t(v.seg_out[g].n_sites)), key = v.reads[i].key, mask = v.mask[i];
    const u64 pre = pre_key_of(v, i), pre_mask = pre_mask_of(v, i);
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u];
    int32_t group = -1, how;
    if (mask == full && pre_mask == pre_full_of(v, g)) {  // (uniform over the wave, like everything it branches on below)
        how = (v.flags[i] & KEY_SUPPORTED) ? IOC_ISO_DIRECT : IOC_ISO_RARE;
        if (how == IOC_ISO_DIRECT) group = int32_t(key_rank(v, mb, me, pre, key, lane));
    } else {
        uint32_t agreeing = 0;
        u64 which_pre = 0, which_key = 0;
        for (uint32_t m0 = mb; m0 < me && (mask | pre_mask) != 0ull; m0 += 64u) {
            const Member x = member_at(v, m0 + lane, me, true);
            const u64 hits = __ballot(x.there && (x.flags & KEY_FIRST) && inserts_key_agrees(pre, key, x.pre, x.key, pre_mask, mask));
            if (hits && agreeing == 0u) which_pre = shfl64(x.pre, uint32_t(__builtin_ctzll(hits))), which_key = shfl64(x.key, uint32_t(__builtin_ctzll(hits)));
            agreeing += uint32_t(__popcll(hits));
        }
        how = agreeing == 1u ? IOC_ISO_ASSIGNED : IOC_ISO_AMBIGUOUS;
        if (agreeing == 1u) group = int32_t(key_rank(v, mb, me, which_pre, which_key, lane));
    }
    if (lane == 0) v.reads[i].group = group, v.reads[i].how = how;
}

__global__ void __launch_bounds__(64 * WAVES)
k_ins_record(IocReadInsertsDev v)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (g >= v.n_segs) return;
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u], ns = uint32_t(v.seg_out[g].n_sites);
    const u64 sb = u64(v.site_base[g]);
    uint32_t groups = 0, how_n[4] = {0, 0, 0, 0}, state_n[4] = {0, 0, 0, 0};
    for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
        const Member x = member_at(v, m0 + lane, me, true);
        const uint32_t how = x.there ? uint32_t(v.reads[x.pair].how) : 4u;
        groups += uint32_t(__popcll(__ballot(x.there && (x.flags & KEY_FIRST))));
#pragma unroll
        for (uint32_t h = 0; h < 4u; ++h) how_n[h] += uint32_t(__popcll(__ballot(how == h)));
        for (uint32_t b = 0; b < ns && b < uint32_t(IOC_INSERTS_MAX); ++b) {  // (site b: how many of the 64 members are in each state; lane b keeps the sums)
            const uint32_t st = uint32_t(x.key >> (2u * b)) & 3u;
#pragma unroll
            for (uint32_t h = 0; h < 4u; ++h) {
                const uint32_t n = uint32_t(__popcll(__ballot(x.there && st == h)));
                if (lane == b) state_n[h] += n;
            }
        }
    }
    if (lane == 0) {
        ioc_inserts_seg* r = v.seg_out + g;
        r->n_groups = int32_t(groups), r->n_reads = int32_t(me - mb), r->n_direct = int32_t(how_n[IOC_ISO_DIRECT]), r->n_assigned = int32_t(how_n[IOC_ISO_ASSIGNED]),
        r->n_rare = int32_t(how_n[IOC_ISO_RARE]), r->n_ambiguous = int32_t(how_n[IOC_ISO_AMBIGUOUS]);
    }
    if (lane < ns && lane < uint32_t(IOC_INSERTS_MAX) && sb + lane < v.n_site_slots) {
        ioc_pile_insert* b = v.sites + sb + lane;
        b->n_carry = state_n[IOC_INS_CARRY], b->n_lack = state_n[IOC_INS_LACK], b->n_none = state_n[IOC_INS_NONE];
        b->reserved = 0;
    }
}

}  // namespace

static_assert(sizeof(ioc_insert_row) == 8 && sizeof(ioc_pile_insert) == 32 && sizeof(ioc_read_inserts) == 32 && sizeof(ioc_inserts_seg) == 32,
              "the records are laid out as the public ones");

// The bytes of a slice's operation strings in [buf, ..): pair pid's length plane is ilen_planes + plane[pid] .. + its reference
// length, set to 0 by the caller.  The arguments of iock_ops_project_ins, without the pool.
hipError_t iock_ops_project_ilen(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room, const uint32_t* ord,
                                 uint32_t cnt, const int64_t* row_base, const uint64_t* plane, uint8_t* ilen_planes, uint64_t plane_bytes)
{
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ops_project_ilen, dim3((cnt + OP_WAVES - 1) / OP_WAVES), dim3(64 * OP_WAVES), 0, st, buf, end, len, room, ord, cnt, row_base, plane,
                       ilen_planes, plane_bytes);
    return hipGetLastError();
}

// The eight kernels over the view, in a row on `st`.  The caller has set v.sites, v.reads and v.seg_out to 0.  `each` (9 events,
// or NULL): one is recorded in front of every kernel and one behind the last, so that every kernel can be timed on its own.
hipError_t iock_read_inserts(hipStream_t st, const IocReadInsertsDev& v, int32_t min_ins, int32_t slack, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                             int32_t max_sites, hipEvent_t* each)
{
    const InsertsRule rule{min_ins, slack, min_depth, min_alt, min_pct, max_sites};
    if (v.n_segs == 0) return hipSuccess;
    auto grid = [](uint64_t items) { return dim3(uint32_t((items + WAVES - 1u) / WAVES)); };
    const dim3 block(64 * WAVES);
    int step = 0;
    auto mark = [&]() { if (each) (void)hipEventRecord(each[step++], st); };
    mark();
    if (v.n_pairs) hipLaunchKernelGGL(k_ins_bits, grid(v.n_pairs), block, 0, st, v, rule);
    mark();
    if (v.n_seg_words) hipLaunchKernelGGL(k_ins_rows, grid(v.n_seg_words), block, 0, st, v, rule);
    mark();
    hipLaunchKernelGGL(k_ins_list, grid(v.n_segs), block, 0, st, v);
    mark();
    if (v.n_pairs) hipLaunchKernelGGL(k_ins_states, grid(v.n_pairs), block, 0, st, v, rule);
    mark();
    if (v.n_site_slots) hipLaunchKernelGGL(k_ins_lens, grid(v.n_site_slots), block, 0, st, v);
    mark();
    if (v.n_pairs) hipLaunchKernelGGL(k_ins_support, grid(v.n_pairs), block, 0, st, v, rule);
    mark();
    if (v.n_pairs) hipLaunchKernelGGL(k_ins_isoforms, grid(v.n_pairs), block, 0, st, v);
    mark();
    hipLaunchKernelGGL(k_ins_record, grid(v.n_segs), block, 0, st, v);
    mark();
    return hipGetLastError();
}
