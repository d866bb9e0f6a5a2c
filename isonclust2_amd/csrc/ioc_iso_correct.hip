// ioc_iso_correct.hip — every read of a call corrected against the tables of its own isoform, with a long insertion carried
// through as the read has it (ioc_planes_correct_groups, ioc_align_pairs_blocks_correct; the definition is
// ioc_host_read_correct_long, ioc_align.cpp).
//
// The shape is k_read_correct's (ioc_read_correct.hip): one wave per pair, IOC_ISO_CORRECT_WAVES pairs per workgroup, nothing
// shared between the waves, no barrier; the wave walks its pair's rlen + 1 rows in chunks of 64, a lane per row, decides every
// chunk one chunk ahead and holds the fill and remove masks of the chunks c - 1, c and c + 1 for the run guard.  What differs:
//   - the tables are those of the group-segment table[i] names — the pair's isoform, or its whole segment (k_group_pile made
//     both) — not of seg_of_pair[i];
//   - a lane also reads its row's bytes of the length and the position plane, and forms the row with iso_correct_row
//     (ioc_iso_correct.h): a long row emits ilen bytes of the read and then its base, so a lane's length is up to 254 + 1, which
//     the wave scan and the running carry take as they are;
//   - a row can make the pair unresolved: the count pass ORs that over the pair, and such a pair counts 0 bytes and writes none.
//   k_iso_correct_count  per lane the bytes and the record's counters over the chunks, summed over the wave at the end:
//                        pair_len[i] and the 48-byte record.
//   k_pile_scan          (ioc_pile_call.hip, through iock_pile_scan) out_off[0 .. n_pairs] = the exclusive scan of pair_len.
//   k_iso_correct_emit   decides again and writes.  A long run is copied from the pool by the whole wave: over the __ballot of the
//                        chunk's long-row lanes, run after run, a lane per byte (at most four steps of 64), so that no lane writes
//                        254 bytes one after the other; every lane then writes its row's own 0 to 7 bytes behind its run.
// No atomics and no LDS: every output byte has one writer and its place is a function of the inputs alone.  Every table row, plane
// byte, frame byte, pool byte and output byte is held against the sizes passed.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ioc_internal.h"
#include "ioc_iso_correct.h"
#include "ioc_wave.h"

namespace {

constexpr uint32_t WAVES = IOC_ISO_CORRECT_WAVES;

// what a wave reads of its pair beside ReadPairView: the length and the position plane, and the read in the pool
struct IsoPairView {
    ReadPairView v;
    const uint8_t* __restrict__ ilen_planes;
    const uint32_t* __restrict__ qpos_planes;
    const uint8_t* __restrict__ pool;
    uint64_t pool_bytes, q0;
    uint32_t qlen;  // (0 where the read does not lie inside the pool: every long row is then unresolved)

    // what row p emits, its decision and the guard's verdict known (a row outside: nothing)
    __device__ __forceinline__ IsoRowOut row(uint32_t p, uint32_t decision, bool guarded, const ReadRule& k) const
    {
        return v.row_as(p, [&](uint64_t r, uint64_t at, unsigned long long D, bool spans, uint8_t own, unsigned long long slots) {
            return iso_correct_row(v.cols[r], v.ins[r], D, spans, own, slots, ilen_planes[at], qpos_planes[at], qlen, decision, guarded, k);
        });
    }
};

template <bool EMIT>
__device__ __forceinline__ void iso_correct_pair(const IocIsoCorrectDev& d, const ReadRule& rule, const long long* __restrict__ out_off,
                                                 uint8_t* __restrict__ out_seq, uint8_t* __restrict__ out_qual, uint64_t out_bytes)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= d.n_pairs) return;  // (whole waves: there is no barrier below)
    long long* const pair_len = reinterpret_cast<long long*>(d.pair_len);
    const uint32_t tab = d.table[i];
    if (tab >= d.n_tables) {  // (the entry points name no such table: an empty result)
        if (!EMIT && lane == 0) pair_len[i] = 0, d.stats[i] = ioc_iso_correct_stats{};
        return;
    }
    if (EMIT && pair_len[i] <= 0) return;  // (an unresolved pair, or one that emits nothing: the same in every lane)
    const uint64_t q0 = d.q_off[i];
    const uint32_t ql = d.q_len[i];
    const IsoPairView v{ReadPairView{d.cols, d.ins, d.n_rows, d.frames, d.frame_bytes, d.base_planes, d.slot_planes, d.plane_bytes, d.gsegs[tab], d.plane[i]},
                        d.ilen_planes, d.qpos_planes, d.pool, d.pool_bytes, q0, q0 <= d.pool_bytes && ql <= d.pool_bytes - q0 ? ql : 0u};
    const uint32_t rows = uint32_t(v.v.s.rlen) + 1u, nchunks = (rows + 63u) / 64u;

    uint32_t n = 0, k_sub = 0, k_fill = 0, k_rem = 0, k_add = 0, k_drop = 0, k_low = 0, k_guard = 0, k_runs = 0;
    unsigned long long k_bases = 0;  // (64 bits: planes that are not a read's can name more bytes than 32 bits hold)
    bool unresolved = false;
    unsigned long long carry = EMIT ? (unsigned long long)out_off[i] : 0ull;
    unsigned long long fill_prev = 0, rem_prev = 0;
    uint32_t dec = v.v.decide(lane, rule);  // (chunk 0; every lane of the wave takes every step below: there are ballots in it)
    unsigned long long fill_cur = __ballot(read_kind(dec) == READ_FILL), rem_cur = __ballot(read_kind(dec) == READ_REMOVE);
    for (uint32_t c = 0; c < nchunks; ++c) {
        const uint32_t p = c * 64u + lane;
        const uint32_t dec_next = c + 1u < nchunks ? v.v.decide(p + 64u, rule) : uint32_t(READ_NONE);
        const unsigned long long fill_next = __ballot(read_kind(dec_next) == READ_FILL), rem_next = __ballot(read_kind(dec_next) == READ_REMOVE);
        const uint32_t kind = read_kind(dec);
        const bool guarded = kind == READ_FILL     ? read_run_exceeds(fill_prev, fill_cur, fill_next, lane, rule.max_run)
                             : kind == READ_REMOVE ? read_run_exceeds(rem_prev, rem_cur, rem_next, lane, rule.max_run)
                                                   : false;
        const IsoRowOut r = v.row(p, dec, guarded, rule);
        if (!EMIT) {
            n += r.row.n, k_sub += r.row.n_sub, k_fill += r.row.n_fill, k_rem += r.row.n_remove, k_add += r.row.n_ins_add, k_drop += r.row.n_ins_drop,
                k_low += r.row.n_low, k_guard += r.row.n_guarded, k_runs += r.long_len > 0u, k_bases += r.long_len;
            unresolved = unresolved || r.unresolved;
        } else {
            const uint32_t incl = wave_scan_incl(r.bytes(), lane), before = incl - r.bytes();
            // the chunk's long runs, one after the other, by the whole wave: a lane per byte
            for (unsigned long long todo = __ballot(r.long_len > 0u); todo; todo &= todo - 1ull) {
                const int src = __builtin_ctzll(todo);
                const uint32_t len = uint32_t(__shfl(int(r.long_len), src, 64)), from = uint32_t(__shfl(int(r.long_from), src, 64));
                const unsigned long long to = carry + uint32_t(__shfl(int(before), src, 64));
                for (uint32_t x = lane; x < len; x += 64u) {
                    const uint64_t q = v.q0 + from + x;  // (from + len <= qlen in a resolved pair, and the read lies inside the pool)
                    if (to + x < out_bytes && q < v.pool_bytes) out_seq[to + x] = v.pool[q], out_qual[to + x] = uint8_t('!');
                }
            }
            unsigned long long at = carry + before + r.long_len;
            for (uint32_t x = 0; x < r.row.n; ++x, ++at)
                if (at < out_bytes) {
                    out_seq[at] = uint8_t(r.row.seq >> (8u * x));
                    out_qual[at] = uint8_t(r.row.qual >> (8u * x));
                }
            carry += uint32_t(__shfl(int(incl), 63, 64));
        }
        fill_prev = fill_cur, rem_prev = rem_cur, fill_cur = fill_next, rem_cur = rem_next, dec = dec_next;
    }
    if (EMIT) return;
    // (the bytes of a resolved pair, at most 7 per row and its read's length, fit 32 bits like the record's out_len: the entries refuse
    // longer pairs, and long runs that together exceed the read make the pair unresolved)
    const uint32_t t[9] = {wave_sum(n), wave_sum(k_sub), wave_sum(k_fill), wave_sum(k_rem), wave_sum(k_add), wave_sum(k_drop), wave_sum(k_low), wave_sum(k_guard), wave_sum(k_runs)};
    const unsigned long long bases = wave_sum64(k_bases);
    const bool any_unresolved = __ballot(unresolved) != 0ull || bases > (unsigned long long)v.qlen;
    if (lane == 0) {
        ioc_iso_correct_stats st{};
        st.table = iso_table_name(tab, d.n_group_tables);
        if (any_unresolved) {
            st.flags = IOC_ISOC_UNRESOLVED;
        } else {
            st.out_len = int32_t(t[0] + uint32_t(bases)), st.n_sub = int32_t(t[1]), st.n_fill = int32_t(t[2]), st.n_remove = int32_t(t[3]), st.n_ins_add = int32_t(t[4]),
            st.n_ins_drop = int32_t(t[5]), st.n_low = int32_t(t[6]), st.n_guarded = int32_t(t[7]), st.n_long_runs = int32_t(t[8]), st.n_long_bases = int32_t(bases);
        }
        pair_len[i] = any_unresolved ? 0ll : (long long)(t[0] + uint32_t(bases));
        d.stats[i] = st;
    }
}

__global__ void __launch_bounds__(64 * WAVES) k_iso_correct_count(IocIsoCorrectDev d, ReadRule rule)
{
    iso_correct_pair<false>(d, rule, nullptr, nullptr, nullptr, 0);
}

__global__ void __launch_bounds__(64 * WAVES)
k_iso_correct_emit(IocIsoCorrectDev d, ReadRule rule, const long long* __restrict__ out_off, uint8_t* __restrict__ out_seq, uint8_t* __restrict__ out_qual,
                   uint64_t out_bytes)
{
    iso_correct_pair<true>(d, rule, out_off, out_seq, out_qual, out_bytes);
}

}  // namespace

static_assert(sizeof(ioc_iso_correct_stats) == 48, "the record is laid out as the public one");
static_assert(sizeof(long long) == sizeof(int64_t), "offsets");

// The count pass and the scan over the pairs of v: v.pair_len[i] and v.stats[i], and out_off[0 .. n_pairs] (device) — out_off[n_pairs]
// is what the write pass needs of out_seq / out_qual.
hipError_t iock_iso_correct_count(hipStream_t st, const IocIsoCorrectDev& v, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_run,
                                  int64_t* out_off)
{
    if (v.n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_iso_correct_count, dim3((v.n_pairs + WAVES - 1u) / WAVES), dim3(64 * WAVES), 0, st, v, ReadRule{min_depth, min_alt, min_pct, max_run});
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : iock_pile_scan(st, v.pair_len, v.n_pairs, out_off);
}

// The write pass: pair i's bytes to out_seq / out_qual (out_bytes bytes each; nothing is written behind them) from out_off[i] on.
hipError_t iock_iso_correct_emit(hipStream_t st, const IocIsoCorrectDev& v, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_run,
                                 const int64_t* out_off, uint8_t* out_seq, uint8_t* out_qual, uint64_t out_bytes)
{
    if (v.n_pairs == 0 || out_bytes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_iso_correct_emit, dim3((v.n_pairs + WAVES - 1u) / WAVES), dim3(64 * WAVES), 0, st, v, ReadRule{min_depth, min_alt, min_pct, max_run},
                       reinterpret_cast<const long long*>(out_off), out_seq, out_qual, out_bytes);
    return hipGetLastError();
}
