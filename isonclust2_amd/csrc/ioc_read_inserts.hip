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
//                    bytes and over a halo of 32 on either side (ilen_window loads them, window_sums of ioc_read_stage.h adds them
//                    up): two byte loads a lane and chunk, not 2 slack + 1.  The
//                    near word is the ballot of "spans and W >= min_ins".  Lane w keeps word w of 64, the wave writes 64 words at a
//                    time; also the read's n_near and ins_bases.
//   k_ins_rows       a wave per 64 junctions of a segment, the members 64 at a time (member_row_counts, ioc_read_stage.h): span,
//                    in_ins and, by ballot, the word of variable junctions.
//   k_ins_list       a wave per segment sweeps the variable words for runs of any length (run_list_any, ioc_read_stage.h); the first
//                    max_sites are written.
//   k_ins_states     a wave per pair, a lane per kept site: masked popcounts of the span and the near words (masked_counts), the
//                    state, and the key and its mask by an OR over the wave.  Then site by site where the pair carries: its largest
//                    W over the site's junctions (ilen_window again, the only plane bytes read after k_ins_bits), which lane k keeps
//                    and stores as 16 bits (at most 65 x 255) at the pair's place of a scratch table, max_sites entries a pair.
//   k_ins_lens       a wave per kept site over the segment's members, 64 at a time: the smallest and the largest of the carriers'
//                    entries.  (A first form computed W here, a wave per site walking its carriers one after the other: 0.83 ms for
//                    600 carriers of two sites, against 0.02 ms of everything else the two kernels do.)
//   k_ins_support, k_ins_isoforms, k_ins_record
//                    key_support, key_isoform and key_tallies (ioc_read_stage.h) on two-word keys (the block stage's word, read
//                    where that stage left it, and this stage's): unsigned compares, major word first.
// No atomics and no LDS: every output byte has one writer and is a function of the inputs alone.  Every plane byte, word, table row
// and record is held against the sizes passed.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ioc_internal.h"
#include "ioc_ops_pileup.h"
#include "ioc_read_inserts.h"
#include "ioc_read_stage.h"

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

// W(p0 + lane) of the pair whose length plane begins at byte po (window_sums, ioc_read_stage.h), and own = its byte at p0 + lane:
// two byte loads a lane, 0 outside rows 0 .. rlen.  Every lane of the wave takes part.
__device__ __forceinline__ uint32_t ilen_window(const IocReadInsertsDev& v, u64 po, uint32_t rlen, long long p0, uint32_t slack, uint32_t lane, uint32_t& own)
{
    auto at = [&](long long q) -> uint32_t { return q >= 0 && q <= (long long)rlen && po + u64(q) < v.plane_bytes ? uint32_t(v.ilen_planes[po + u64(q)]) : 0u; };
    own = at(p0 + lane);
    return window_sums(own, at(lane < 32u ? p0 - 32 + lane : p0 + 32 + lane), slack, lane);
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
            const uint32_t win = ilen_window(v, po, rlen, (long long)c * 64, uint32_t(rule.slack), lane, own);
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
    const uint2 n = member_row_counts(v, g, c, v.span, v.near, lane);
    const uint32_t spanned = n.x, in = n.y;
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
    const uint32_t base_s = run_list_any(v.var, at, v.n_seg_words, W, lane, v.sites, sb, v.n_site_slots, most);
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
        const uint2 n = masked_counts(v.span, v.near, w0, v.n_pair_words, W, first, end);
        const uint32_t st = inserts_state(uint32_t(end - first), n.x, n.y);
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
            const uint32_t win = ilen_window(v, v.plane[i], rlen, p0, uint32_t(rule.slack), lane, own);
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

__global__ void __launch_bounds__(64 * WAVES)
k_ins_support(IocReadInsertsDev v, InsertsRule rule)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;
    const uint8_t flags = key_support(v, i, g, blocks_full_mask(uint32_t(v.seg_out[g].n_sites)), uint32_t(rule.min_alt), lane);
    if (lane == 0) v.flags[i] = flags;
}

__global__ void __launch_bounds__(64 * WAVES)
k_ins_isoforms(IocReadInsertsDev v)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;
    const KeyIsoform r = key_isoform(v, i, g, blocks_full_mask(uint32_t(v.seg_out[g].n_sites)), lane);
    if (lane == 0) v.reads[i].group = r.group, v.reads[i].how = r.how;
}

__global__ void __launch_bounds__(64 * WAVES)
k_ins_record(IocReadInsertsDev v)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (g >= v.n_segs) return;
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u], ns = min(uint32_t(v.seg_out[g].n_sites), uint32_t(IOC_INSERTS_MAX));
    const u64 sb = u64(v.site_base[g]);
    const KeyTallies t = key_tallies(v, mb, me, ns, lane);
    if (lane == 0) {
        ioc_inserts_seg* r = v.seg_out + g;
        r->n_groups = int32_t(t.groups), r->n_reads = int32_t(me - mb), r->n_direct = int32_t(t.how_n[IOC_ISO_DIRECT]), r->n_assigned = int32_t(t.how_n[IOC_ISO_ASSIGNED]),
        r->n_rare = int32_t(t.how_n[IOC_ISO_RARE]), r->n_ambiguous = int32_t(t.how_n[IOC_ISO_AMBIGUOUS]);
    }
    if (lane < ns && sb + lane < v.n_site_slots) {
        ioc_pile_insert* b = v.sites + sb + lane;
        b->n_carry = t.state_n[IOC_INS_CARRY], b->n_lack = t.state_n[IOC_INS_LACK], b->n_none = t.state_n[IOC_INS_NONE];
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
