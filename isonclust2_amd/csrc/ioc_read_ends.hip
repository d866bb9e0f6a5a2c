// ioc_read_ends.hip — the alternative ends of every segment of a call: start and stop sites, every read's sites and the variants
// (ioc_reads_ends, ioc_align_pairs_blocks_ends; the definition is ioc_host_reads_ends, ioc_align.cpp).  Eight kernels in a row on one
// stream; but for the first, a wave per item, IOC_READ_ENDS_WAVES items per workgroup; nothing is shared between the waves of a
// workgroup, so there is no barrier and a wave either runs whole or returns.
//   k_end_hist      a lane per pair: one integer add into its start row, one into its stop row, one into its segment's N — no-return
//                   atomics into zeroed words, as k_ops_pileup has them.  Integer adds commute, so the rows are a function of the
//                   inputs alone.  The other way, a lane per row over the segment's extents, reads every extent of a segment once per
//                   64 rows: 24 passes over 600 extents for a 1500-row representative, against three adds a read.
//   k_end_rows      a wave per 64 rows of a segment, a lane per row: Ws and We from two wave prefix sums each, over the 64 rows and
//                   over a halo of 32 on either side (window_sums, ioc_read_stage.h; slack <= 32 fits the halo), the row test, the
//                   start-row and stop-row words by ballot, and the row table where it is asked for.
//   k_end_list      a wave per (segment, kind) sweeps its words for runs of any length (run_list_any, ioc_read_stage.h); the first
//                   max_sites are written.
//   k_end_class     a wave per read: lanes 0 .. 31 the kept start sites, lanes 32 .. 63 the kept stop sites; (distance, site) as one
//                   word, its minimum over each half of the wave; then the read's key and whether it is placed.
//   k_end_count     a wave per kept site: the segment's reads 64 at a time, n_reads and n_over by ballot and popcount; then the peak,
//                   the wave maximum over the site's rows of (count, rlen - row) as one word.  (The peak stands here and not in
//                   k_end_list: there the lanes that would read a site's bounds are not the lanes that wrote them, within one wave
//                   and with no kernel boundary between the store and the load; here the bounds come from an earlier kernel.)
//   k_end_support, k_end_variants, k_ends_record
//                   the shape of key_support, key_isoform and key_tallies (ioc_read_stage.h) over one unsigned 64-bit key a read
//                   whose order is the variants'; unplaced reads are left out by a flag and a read's support is a `same` word, not
//                   masks, so these keep bodies of their own and share tally_hits.  A wave per read over its segment's reads: the
//                   two kernels quadratic in a segment's reads.
// No floating point, no LDS; but for the adds of k_end_hist every output word has one writer.  Every row, word, slot and record is
// held against the sizes passed.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ioc_internal.h"
#include "ioc_read_ends.h"
#include "ioc_read_stage.h"

namespace {

constexpr uint32_t WAVES = IOC_READ_ENDS_WAVES;
typedef unsigned long long u64;

enum : uint8_t { END_PLACED = 1 };
enum : uint32_t { SAME_FIRST = 0x80000000u, SAME_COUNT = 0x7FFFFFFFu };  // `same`: how many placed reads carry the read's key; bit 31: none before it

__global__ void __launch_bounds__(64 * WAVES)
k_end_hist(IocReadEndsDev v)
{
    const uint32_t i = blockIdx.x * (64u * WAVES) + threadIdx.x;
    if (i >= v.n_pairs) return;
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;  // (the entry points refuse such a pair, and an extent outside its segment)
    const IocPileSeg s = v.segs[g];
    const ioc_read_extent e = v.extents[i];
    if (!ends_extent_ok(e, s.rlen) || !ends_takes_part(e)) return;
    const u64 a = u64(s.row0) + u64(uint32_t(e.first_row)), z = u64(s.row0) + u64(uint32_t(e.end_row));
    if (a >= v.n_rows || z >= v.n_rows) return;
    atomicAdd(&v.hist[a].x, 1u);
    atomicAdd(&v.hist[z].y, 1u);
    atomicAdd(&v.n_part[g], 1u);
}

__global__ void __launch_bounds__(64 * WAVES)
k_end_rows(IocReadEndsDev v, EndsRule rule)
{
    const uint32_t lane = threadIdx.x & 63u;
    const u64 t = u64(blockIdx.x) * WAVES + (threadIdx.x >> 6);
    if (t >= v.n_seg_words) return;  // (whole waves: there is no barrier below)
    const uint32_t g = uint32_t(v.word_seg[t]);
    if (g >= v.n_segs) return;
    const IocPileSeg s = v.segs[g];
    const long long rlen = s.rlen, p0 = (long long)(t - v.seg_word[g]) * 64;
    auto at = [&](long long q) -> uint2 { return q >= 0 && q <= rlen && u64(s.row0) + u64(q) < v.n_rows ? v.hist[u64(s.row0) + u64(q)] : make_uint2(0u, 0u); };
    const uint2 own = at(p0 + lane), halo = at(lane < 32u ? p0 - 32 + lane : p0 + 32 + lane);
    const uint32_t ws = window_sums(own.x, halo.x, uint32_t(rule.slack), lane), we = window_sums(own.y, halo.y, uint32_t(rule.slack), lane);
    const long long p = p0 + lane;
    const bool in = p <= rlen;
    const uint32_t N = v.n_part[g];
    const u64 bs = __ballot(in && rule.row(N, ws)), be = __ballot(in && rule.row(N, we));
    if (lane == 0) v.bits_start[t] = bs, v.bits_stop[t] = be;
    if (v.rows && in && u64(s.row0) + u64(p) < v.n_rows) v.rows[u64(s.row0) + u64(p)] = ioc_end_row{own.x, own.y, ws, we};
}

__global__ void __launch_bounds__(64 * WAVES)
k_end_list(IocReadEndsDev v)
{
    const uint32_t lane = threadIdx.x & 63u, u = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (u >= 2u * v.n_segs) return;
    const uint32_t g = u >> 1, kind = u & 1u;
    const uint32_t W = seg_words(v.segs[g]);
    const u64 sb = u64(v.site_base[u]), at = v.seg_word[g];
    const uint32_t most = uint32_t(u64(v.site_base[u + 1u]) - sb);  // min(max_sites, rlen + 1)
    const u64* bits = kind ? v.bits_stop : v.bits_start;
    const uint32_t base_s = run_list_any(bits, at, v.n_seg_words, W, lane, v.sites, sb, v.n_site_slots, most);
    if (lane == 0) {
        ioc_ends_seg* r = v.seg_out + g;
        if (kind) r->n_stops = int32_t(min(base_s, most)), r->n_stops_found = int32_t(base_s);
        else r->n_starts = int32_t(min(base_s, most)), r->n_starts_found = int32_t(base_s);
    }
}

__device__ __forceinline__ uint32_t kept_sites(const IocReadEndsDev& v, uint32_t g, uint32_t kind)
{
    return min(uint32_t(kind ? v.seg_out[g].n_stops : v.seg_out[g].n_starts), uint32_t(IOC_ENDS_MAX));
}

__global__ void __launch_bounds__(64 * WAVES)
k_end_class(IocReadEndsDev v, EndsRule rule)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;
    const ioc_read_extent e = v.extents[i];
    const bool part = ends_extent_ok(e, v.segs[g].rlen) && ends_takes_part(e);
    const uint32_t kind = lane >> 5, b = lane & 31u;
    const u64 x = u64(v.site_base[2u * g + kind]) + b;
    uint32_t word = ENDS_FAR;
    if (part && b < kept_sites(v, g, kind) && x < v.n_site_slots)
        word = ends_near_word(ends_distance(v.sites[x].first, v.sites[x].end, kind ? e.end_row : e.first_row), b, rule.slack);
#pragma unroll
    for (uint32_t d = 16; d >= 1u; d >>= 1) word = min(word, uint32_t(__shfl_xor(int(word), int(d), 64)));  // (within each half of the wave)
    const int32_t start = ends_near_site(shfl32(word, 0u)), stop = ends_near_site(shfl32(word, 32u));
    if (lane == 0) {
        const int32_t pre = v.pre_group ? v.pre_group[u64(i) * v.pre_stride] : 0;
        const bool placed = ends_placed(pre, start, stop);
        v.reads[i] = ioc_read_ends{start, stop, -1, 0};
        v.key[i] = placed ? ends_key(pre, start, stop) : 0ull;
        v.flags[i] = placed ? uint8_t(END_PLACED) : uint8_t(0);
    }
}

__global__ void __launch_bounds__(64 * WAVES)
k_end_count(IocReadEndsDev v, EndsRule rule)
{
    const uint32_t lane = threadIdx.x & 63u;
    const u64 x = u64(blockIdx.x) * WAVES + (threadIdx.x >> 6);
    if (x >= v.n_site_slots) return;
    const uint32_t u = uint32_t(v.slot_unit[x]);
    if (u >= 2u * v.n_segs) return;
    const uint32_t g = u >> 1, kind = u & 1u, k = uint32_t(x - u64(v.site_base[u]));
    if (k >= kept_sites(v, g, kind)) return;
    uint32_t n_reads = 0, n_over = 0;
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u];
    for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
        bool mine = false, over = false;
        if (m0 + lane < me) {
            const uint32_t i = v.members[m0 + lane];
            if (i < v.n_pairs) {
                mine = (kind ? v.reads[i].stop_site : v.reads[i].start_site) == int32_t(k);
                over = mine && (kind ? v.extents[i].tail : v.extents[i].head) >= rule.min_over;
            }
        }
        n_reads += uint32_t(__popcll(__ballot(mine))), n_over += uint32_t(__popcll(__ballot(over)));
    }
    const IocPileSeg s = v.segs[g];
    const long long first = v.sites[x].first, end = v.sites[x].end;
    u64 peak = 0;
    for (long long p0 = first; p0 < end; p0 += 64) {
        const long long p = p0 + lane;
        if (p < end && p <= (long long)s.rlen && u64(s.row0) + u64(p) < v.n_rows) {
            const uint2 h = v.hist[u64(s.row0) + u64(p)];
            peak = max(peak, ends_peak_word(kind ? h.y : h.x, uint32_t(s.rlen), uint32_t(p)));
        }
    }
    peak = wave_max64(peak);
    if (lane == 0) {
        ioc_end_site* r = v.sites + x;
        r->n_reads = n_reads, r->n_over = n_over, r->peak_row = ends_peak_row(peak, uint32_t(s.rlen)), r->peak_reads = ends_peak_count(peak);
        r->kind = int32_t(kind), r->reserved = 0u;
    }
}

// what a wave reads of member m of its segment (lane's member of a chunk): the pair, whether it is placed, its key, its `same` word
struct EndMember {
    uint32_t pair = 0xFFFFFFFFu, same = 0;
    u64 key = 0;
    bool placed = false;
};
__device__ __forceinline__ EndMember end_member_at(const IocReadEndsDev& v, uint32_t m, uint32_t me, bool with_same)
{
    EndMember x;
    if (m >= me) return x;
    x.pair = v.members[m];
    if (x.pair >= v.n_pairs) return x;
    x.placed = (v.flags[x.pair] & END_PLACED) != 0, x.key = v.key[x.pair];
    if (with_same) x.same = v.same[x.pair];
    return x;
}

__global__ void __launch_bounds__(64 * WAVES)
k_end_support(IocReadEndsDev v)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;
    uint32_t same = 0, earlier = 0;
    if (v.flags[i] & END_PLACED) {  // (uniform over the wave)
        const u64 key = v.key[i];
        const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u];
        for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
            const EndMember x = end_member_at(v, m0 + lane, me, false);
            const bool hit = x.placed && x.key == key;
            tally_hits(hit, x.pair < i, same, earlier);  // (a segment's reads are its pairs in ascending order)
        }
    }
    if (lane == 0) v.same[i] = same ? (same & SAME_COUNT) | (earlier == 0u ? uint32_t(SAME_FIRST) : 0u) : 0u;
}

__global__ void __launch_bounds__(64 * WAVES)
k_end_variants(IocReadEndsDev v, EndsRule rule)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;
    const uint32_t mine = v.same[i];
    if ((mine & SAME_COUNT) < uint32_t(rule.min_alt)) return;  // (unplaced: 0; uniform over the wave)
    const u64 key = v.key[i];
    uint32_t rank = 0;  // the supported keys below the read's, each counted at its first read
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u];
    for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
        const EndMember x = end_member_at(v, m0 + lane, me, true);
        rank += uint32_t(__popcll(__ballot(x.placed && (x.same & SAME_FIRST) && (x.same & SAME_COUNT) >= uint32_t(rule.min_alt) && x.key < key)));
    }
    const u64 vb = u64(v.var_base[g]);
    const uint32_t most = uint32_t(u64(v.var_base[g + 1u]) - vb);  // min(max_variants, reads)
    if (lane != 0 || rank >= most) return;
    v.reads[i].variant = int32_t(rank);
    if ((mine & SAME_FIRST) && vb + rank < v.n_var_slots)
        v.variants[vb + rank] = ioc_end_variant{int32_t(uint32_t(key >> 32)), int32_t((key >> 8) & 0xFFull), int32_t(key & 0xFFull), mine & SAME_COUNT};
}

__global__ void __launch_bounds__(64 * WAVES)
k_ends_record(IocReadEndsDev v, EndsRule rule)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (g >= v.n_segs) return;
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u];
    uint32_t placed = 0, found = 0;
    for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
        const EndMember x = end_member_at(v, m0 + lane, me, true);
        placed += uint32_t(__popcll(__ballot(x.placed)));
        found += uint32_t(__popcll(__ballot(x.placed && (x.same & SAME_FIRST) && (x.same & SAME_COUNT) >= uint32_t(rule.min_alt))));
    }
    if (lane == 0) {
        ioc_ends_seg* r = v.seg_out + g;
        const uint32_t most = uint32_t(v.var_base[g + 1u] - v.var_base[g]);
        r->n_reads = int32_t(v.n_part[g]), r->n_variants = int32_t(min(found, most)), r->n_variants_found = int32_t(found), r->n_placed = int32_t(placed);
    }
}

}  // namespace

static_assert(sizeof(ioc_read_extent) == 16 && sizeof(ioc_end_site) == 32 && sizeof(ioc_end_variant) == 16 && sizeof(ioc_read_ends) == 16 &&
                  sizeof(ioc_ends_seg) == 32 && sizeof(ioc_end_row) == 16,
              "the records are laid out as the public ones");

// The eight kernels over the view, in a row on `st`.  The caller has set v.hist, v.n_part, v.sites, v.variants and v.seg_out to 0.
// `each` (9 events, or NULL): one is recorded in front of every kernel and one behind the last, so that every kernel can be timed
// on its own.
hipError_t iock_read_ends(hipStream_t st, const IocReadEndsDev& v, int32_t slack, int32_t min_over, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                          int32_t max_sites, int32_t max_variants, hipEvent_t* each)
{
    const EndsRule rule{slack, min_over, min_depth, min_alt, min_pct, max_sites, max_variants};
    if (v.n_segs == 0) return hipSuccess;
    auto grid = [](uint64_t items) { return dim3(uint32_t((items + WAVES - 1u) / WAVES)); };
    const dim3 block(64 * WAVES);
    int step = 0;
    auto mark = [&]() { if (each) (void)hipEventRecord(each[step++], st); };
    mark();
    if (v.n_pairs) hipLaunchKernelGGL(k_end_hist, dim3((v.n_pairs + 64u * WAVES - 1u) / (64u * WAVES)), block, 0, st, v);
    mark();
    if (v.n_seg_words) hipLaunchKernelGGL(k_end_rows, grid(v.n_seg_words), block, 0, st, v, rule);
    mark();
    hipLaunchKernelGGL(k_end_list, grid(2ull * v.n_segs), block, 0, st, v);
    mark();
    if (v.n_pairs) hipLaunchKernelGGL(k_end_class, grid(v.n_pairs), block, 0, st, v, rule);
    mark();
    if (v.n_site_slots) hipLaunchKernelGGL(k_end_count, grid(v.n_site_slots), block, 0, st, v, rule);
    mark();
    if (v.n_pairs) hipLaunchKernelGGL(k_end_support, grid(v.n_pairs), block, 0, st, v);
    mark();
    if (v.n_pairs) hipLaunchKernelGGL(k_end_variants, grid(v.n_pairs), block, 0, st, v, rule);
    mark();
    hipLaunchKernelGGL(k_ends_record, grid(v.n_segs), block, 0, st, v, rule);
    mark();
    return hipGetLastError();
}
