// ioc_read_correct.hip — every read of a call corrected against the pileup of its segment, where the tables and the reads' own
// planes lie (ioc_planes_correct, ioc_align_pairs_correct; the definition is ioc_host_read_correct, ioc_align.cpp).
//
// One wave per pair, IOC_READ_CORRECT_WAVES pairs per workgroup; nothing is shared between the waves, so there is no barrier and a
// wave either runs whole or returns.  The wave walks its pair's rlen + 1 rows in chunks of 64, a lane per row:
//   - the lane decides the base of its row (read_base_decide, ioc_read_correct.h — the function the definition uses) from the row's
//     record of counts, the byte of the read's base plane and the frame's base, read reverse-complemented where the segment says so;
//   - __ballot of "fill" and of "remove" gives the chunk's two masks.  A chunk is decided once, one chunk ahead: the wave holds the
//     masks of the chunks c - 1, c and c + 1 while it finishes chunk c, which is all the run guard needs (read_run_exceeds);
//   - the lane forms its row's 0 to 7 bytes, sequence and qualities, in two 64-bit registers (read_correct_row), reading the row's
//     insertion record and its six slot bytes.
//   k_read_correct<false>  counts: per lane the bytes and the record's counters over the chunks, summed over the wave at the end:
//                          pair_len[i] and the 32-byte record.
//   k_pile_scan            (ioc_pile_call.hip, through iock_pile_scan) out_off[0 .. n_pairs] = the exclusive scan of pair_len.
//   k_read_correct<true>   decides again and writes: a wave scan (shuffles) gives a lane's offset in its chunk, a running carry
//                          runs down the pair's chunks from out_off[i].
// No atomics and no LDS: every output byte has one writer and its place is a function of the inputs alone.  Every table row, plane
// byte and frame byte is held against the sizes passed; a row that lies outside them emits nothing and decides nothing.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ioc_internal.h"
#include "ioc_read_correct.h"
#include "ioc_wave.h"

namespace {

constexpr uint32_t WAVES = IOC_READ_CORRECT_WAVES;

template <bool EMIT>
__global__ void __launch_bounds__(64 * WAVES)
k_read_correct(const IocPileSeg* __restrict__ segs, uint32_t n_segs, const int32_t* __restrict__ seg_of_pair, const uint64_t* __restrict__ plane,
               uint32_t n_pairs, const ioc_pileup_col* __restrict__ cols, const ioc_pileup_ins* __restrict__ ins, uint64_t n_rows,
               const uint8_t* __restrict__ frames, uint64_t frame_bytes, const uint8_t* __restrict__ base_planes,
               const uint8_t* __restrict__ slot_planes, uint64_t plane_bytes, ReadRule rule, long long* __restrict__ pair_len,
               ioc_correct_stats* __restrict__ stats, const long long* __restrict__ out_off, uint8_t* __restrict__ out_seq,
               uint8_t* __restrict__ out_qual, uint64_t out_bytes)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= n_pairs) return;  // (whole waves: there is no barrier below)
    const uint32_t g = uint32_t(seg_of_pair[i]);
    if (g >= n_segs) {  // (the entry points refuse such a pair: an empty result)
        if (!EMIT && lane == 0) pair_len[i] = 0, stats[i] = ioc_correct_stats{};
        return;
    }
    const ReadPairView v{cols, ins, n_rows, frames, frame_bytes, base_planes, slot_planes, plane_bytes, segs[g], plane[i]};
    const uint32_t rows = uint32_t(v.s.rlen) + 1u, nchunks = (rows + 63u) / 64u;

    uint32_t n = 0, k_sub = 0, k_fill = 0, k_rem = 0, k_add = 0, k_drop = 0, k_low = 0, k_guard = 0;
    unsigned long long carry = EMIT ? (unsigned long long)out_off[i] : 0ull;
    unsigned long long fill_prev = 0, rem_prev = 0;
    uint32_t dec = v.decide(lane, rule);  // (chunk 0; every lane of the wave takes every step below: there are ballots in it)
    unsigned long long fill_cur = __ballot(read_kind(dec) == READ_FILL), rem_cur = __ballot(read_kind(dec) == READ_REMOVE);
    for (uint32_t c = 0; c < nchunks; ++c) {
        const uint32_t p = c * 64u + lane;
        const uint32_t dec_next = c + 1u < nchunks ? v.decide(p + 64u, rule) : uint32_t(READ_NONE);
        const unsigned long long fill_next = __ballot(read_kind(dec_next) == READ_FILL), rem_next = __ballot(read_kind(dec_next) == READ_REMOVE);
        const uint32_t kind = read_kind(dec);
        const bool guarded = kind == READ_FILL     ? read_run_exceeds(fill_prev, fill_cur, fill_next, lane, rule.max_run)
                             : kind == READ_REMOVE ? read_run_exceeds(rem_prev, rem_cur, rem_next, lane, rule.max_run)
                                                   : false;
        const ReadRowOut r = v.row(p, dec, guarded, rule);
        if (!EMIT) {
            n += r.n, k_sub += r.n_sub, k_fill += r.n_fill, k_rem += r.n_remove, k_add += r.n_ins_add, k_drop += r.n_ins_drop, k_low += r.n_low,
                k_guard += r.n_guarded;
        } else {
            const uint32_t incl = wave_scan_incl(r.n, lane);
            unsigned long long at = carry + (incl - r.n);
            for (uint32_t x = 0; x < r.n; ++x, ++at)
                if (at < out_bytes) {
                    out_seq[at] = uint8_t(r.seq >> (8u * x));
                    out_qual[at] = uint8_t(r.qual >> (8u * x));
                }
            carry += uint32_t(__shfl(int(incl), 63, 64));
        }
        fill_prev = fill_cur, rem_prev = rem_cur, fill_cur = fill_next, rem_cur = rem_next, dec = dec_next;
    }
    if (EMIT) return;
    // (the bytes of a pair, at most 7 per row, fit 32 bits like the record's out_len: the entries refuse longer segments)
    const uint32_t t[8] = {wave_sum(n), wave_sum(k_sub), wave_sum(k_fill), wave_sum(k_rem), wave_sum(k_add), wave_sum(k_drop), wave_sum(k_low), wave_sum(k_guard)};
    if (lane == 0) {
        pair_len[i] = (long long)t[0];
        ioc_correct_stats st{};
        st.out_len = int32_t(t[0]), st.n_sub = int32_t(t[1]), st.n_fill = int32_t(t[2]), st.n_remove = int32_t(t[3]), st.n_ins_add = int32_t(t[4]),
        st.n_ins_drop = int32_t(t[5]), st.n_low = int32_t(t[6]), st.n_guarded = int32_t(t[7]);
        stats[i] = st;
    }
}

template <bool EMIT>
hipError_t launch(hipStream_t st, const IocReadCorrectDev& v, const ReadRule& rule, const int64_t* out_off, uint8_t* out_seq, uint8_t* out_qual, uint64_t out_bytes)
{
    static_assert(sizeof(long long) == sizeof(int64_t), "offsets");
    hipLaunchKernelGGL((k_read_correct<EMIT>), dim3((v.n_pairs + WAVES - 1u) / WAVES), dim3(64 * WAVES), 0, st, v.segs, v.n_segs, v.seg_of_pair, v.plane,
                       v.n_pairs, v.cols, v.ins, v.n_rows, v.frames, v.frame_bytes, v.base_planes, v.slot_planes, v.plane_bytes, rule,
                       reinterpret_cast<long long*>(v.pair_len), v.stats, reinterpret_cast<const long long*>(out_off), out_seq, out_qual, out_bytes);
    return hipGetLastError();
}

}  // namespace

static_assert(sizeof(ioc_correct_stats) == 32, "the record is laid out as the public one");

// The count pass and the scan over the pairs of v: v.pair_len[i] and v.stats[i], and out_off[0 .. n_pairs] (device) — out_off[n_pairs]
// is what the write pass needs of out_seq / out_qual.
hipError_t iock_read_correct_count(hipStream_t st, const IocReadCorrectDev& v, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_run,
                                   int64_t* out_off)
{
    if (v.n_pairs == 0) return hipSuccess;
    const hipError_t e = launch<false>(st, v, ReadRule{min_depth, min_alt, min_pct, max_run}, nullptr, nullptr, nullptr, 0);
    return e != hipSuccess ? e : iock_pile_scan(st, v.pair_len, v.n_pairs, out_off);
}

// The write pass: pair i's bytes to out_seq / out_qual (out_bytes bytes each; nothing is written behind them) from out_off[i] on.
hipError_t iock_read_correct_emit(hipStream_t st, const IocReadCorrectDev& v, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_run,
                                  const int64_t* out_off, uint8_t* out_seq, uint8_t* out_qual, uint64_t out_bytes)
{
    if (v.n_pairs == 0 || out_bytes == 0) return hipSuccess;
    return launch<true>(st, v, ReadRule{min_depth, min_alt, min_pct, max_run}, out_off, out_seq, out_qual, out_bytes);
}
