// ioc_pile_call.hip — the consensus call of many references at once from their pileup tables, where the tables lie
// (ioc_pileup_call, ioc_align_pairs_polish; the definition is ioc_host_pileup_call, ioc_align.cpp).
//
// A segment is one reference: rlen + 1 rows of both tables from a row base on, and its frame in a pool of sequences, read
// reverse-complemented on the fly where the segment says so (as the aligner reads its references).  One workgroup per segment
// walks it in chunks of IOC_PILE_CALL_CHUNK rows, a lane per row: the lane decides its row (pile_call_seg_row and pile_call_row, ioc_pile_call.h — the
// function the definition uses) and holds the 0 to 7 bytes it emits, sequence and qualities, in two 64-bit registers.
//
//   (each of the two passes in two modes: the majority call, and the weighted call of ioc_host_pileup_call_weighted, which
//   decides on the tables of weights and reads the table of counts for the depth gates only — 32 bytes more per row)
//   k_pile_call<false>  counts: per lane the bytes and the record's counters over the segment's chunks, summed over the workgroup
//                       at the end: seg_len[g] and the 32-byte record.
//   k_pile_scan         one wave: out_off[0 .. n_segs] = the exclusive scan of seg_len, 64 segments a step, a running carry.
//   k_pile_call<true>   decides again and writes: a wave scan (shuffles) and a workgroup scan (the waves' totals through LDS) give
//                       a lane's offset in its chunk, a running carry runs down the segment's chunks from out_off[g].
//
// No atomics: every output byte has one writer and its place is a function of the tables alone, so the result does not depend on
// scheduling.  A row's records are 160 bytes (most rows stop at the first insertion slot: 52 bytes read); both passes read them,
// which is cheaper than keeping 14 bytes per row between the passes only for rows that are decided in a few dozen instructions.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ioc_internal.h"
#include "ioc_pile_call.h"
#include "ioc_wave.h"

namespace {

constexpr uint32_t CHUNK = IOC_PILE_CALL_CHUNK;  // rows per step of a workgroup = its threads
constexpr uint32_t WAVES = CHUNK / 64u;
static_assert(CHUNK % 64u == 0 && WAVES >= 1 && WAVES <= 16, "whole waves");

template <bool EMIT, bool WEIGHTED>
__global__ void __launch_bounds__(CHUNK)
k_pile_call(const IocPileSeg* __restrict__ segs, uint32_t n_segs, const ioc_pileup_col* __restrict__ cols,
            const ioc_pileup_ins* __restrict__ ins, const ioc_pileup_col* __restrict__ gate, uint64_t n_rows,
            const uint8_t* __restrict__ frames, uint64_t frame_bytes, int32_t min_depth, long long* __restrict__ seg_len, ioc_polish_stats* __restrict__ stats,
            const long long* __restrict__ out_off, uint8_t* __restrict__ out_seq, uint8_t* __restrict__ out_qual, uint64_t out_bytes)
{
    __shared__ uint32_t part[2][WAVES * 5u];
    const uint32_t g = blockIdx.x;
    if (g >= n_segs) return;  // (whole workgroups)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const IocPileSeg s = segs[g];
    const uint32_t rows = uint32_t(s.rlen) + 1u, nchunks = (rows + CHUNK - 1u) / CHUNK;

    if (!EMIT) {
        uint32_t n = 0, k_ins = 0, k_sub = 0, k_del = 0, k_low = 0;
        for (uint32_t c = 0; c < nchunks; ++c) {
            const uint32_t p = c * CHUNK + tid;
            if (p >= rows) break;
            const PileRowCall r = pile_call_seg_row<WEIGHTED>(s, p, cols, ins, gate, n_rows, frames, frame_bytes, min_depth);
            n += r.n, k_ins += r.n_ins, k_sub += r.n_sub, k_del += r.n_del, k_low += r.n_low;
        }
        // (the bytes of a segment, at most 7 per row, fit 32 bits like the record's out_len: the entries refuse longer segments)
        const uint32_t v[5] = {wave_sum(n), wave_sum(k_ins), wave_sum(k_sub), wave_sum(k_del), wave_sum(k_low)};
        if (lane == 0)
            for (uint32_t x = 0; x < 5u; ++x) part[0][wave * 5u + x] = v[x];
        __syncthreads();
        if (tid == 0) {
            uint32_t t[5] = {0, 0, 0, 0, 0};
            for (uint32_t w = 0; w < WAVES; ++w)
                for (uint32_t x = 0; x < 5u; ++x) t[x] += part[0][w * 5u + x];
            seg_len[g] = (long long)t[0];
            ioc_polish_stats st{};
            st.out_len = int32_t(t[0]), st.n_ins = int32_t(t[1]), st.n_sub = int32_t(t[2]), st.n_del = int32_t(t[3]), st.n_low = int32_t(t[4]);
            stats[g] = st;
        }
        return;
    }

    unsigned long long carry = (unsigned long long)out_off[g];
    for (uint32_t c = 0; c < nchunks; ++c) {  // (every lane of the workgroup takes every step: there are barriers in it)
        const uint32_t p = c * CHUNK + tid;
        PileRowCall r{};
        if (p < rows) r = pile_call_seg_row<WEIGHTED>(s, p, cols, ins, gate, n_rows, frames, frame_bytes, min_depth);
        const uint32_t incl = wave_scan_incl(r.n, lane);
        uint32_t* tot = part[c & 1u];  // (two sets: a wave may be a step ahead of another one's reads)
        if (lane == 63u) tot[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < WAVES; ++w) {
            const uint32_t t = tot[w];
            before += w < wave ? t : 0u;
            all += t;
        }
        unsigned long long at = carry + before + (incl - r.n);
        for (uint32_t x = 0; x < r.n; ++x, ++at)
            if (at < out_bytes) {
                out_seq[at] = uint8_t(r.seq >> (8u * x));
                out_qual[at] = uint8_t(r.qual >> (8u * x));
            }
        carry += all;
    }
}

// out_off[0 .. n_segs]: the exclusive scan of seg_len; one wave, 64 segments a step
__global__ void __launch_bounds__(64)
k_pile_scan(const long long* __restrict__ seg_len, uint32_t n_segs, long long* __restrict__ out_off)
{
    const uint32_t lane = threadIdx.x;
    unsigned long long carry = 0;
    if (lane == 0) out_off[0] = 0;
    for (uint32_t base = 0; base < n_segs; base += 64u) {
        const uint32_t g = base + lane;
        unsigned long long v = g < n_segs ? (unsigned long long)seg_len[g] : 0ull;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const unsigned long long up = shfl_up64(v, d);
            if (lane >= d) v += up;
        }
        if (g < n_segs) out_off[g + 1u] = (long long)(carry + v);
        carry += shfl64(v, 63u);
    }
}

template <bool WEIGHTED>
hipError_t pile_call_launch(hipStream_t st, const IocPileSeg* segs, uint32_t n_segs, const ioc_pileup_col* cols, const ioc_pileup_ins* ins,
                            const ioc_pileup_col* gate, uint64_t n_rows, const uint8_t* frames, uint64_t frame_bytes, int32_t min_depth,
                            int64_t* seg_len, ioc_polish_stats* stats, int64_t* out_off, uint8_t* out_seq, uint8_t* out_qual, uint64_t out_bytes)
{
    static_assert(sizeof(long long) == sizeof(int64_t), "offsets");
    if (n_segs == 0) return hipSuccess;
    hipLaunchKernelGGL((k_pile_call<false, WEIGHTED>), dim3(n_segs), dim3(CHUNK), 0, st, segs, n_segs, cols, ins, gate, n_rows, frames, frame_bytes,
                       min_depth, reinterpret_cast<long long*>(seg_len), stats, static_cast<const long long*>(nullptr),
                       static_cast<uint8_t*>(nullptr), static_cast<uint8_t*>(nullptr), uint64_t(0));
    hipLaunchKernelGGL(k_pile_scan, dim3(1), dim3(64), 0, st, reinterpret_cast<const long long*>(seg_len), n_segs,
                       reinterpret_cast<long long*>(out_off));
    hipLaunchKernelGGL((k_pile_call<true, WEIGHTED>), dim3(n_segs), dim3(CHUNK), 0, st, segs, n_segs, cols, ins, gate, n_rows, frames, frame_bytes,
                       min_depth, static_cast<long long*>(nullptr), static_cast<ioc_polish_stats*>(nullptr),
                       reinterpret_cast<const long long*>(out_off), out_seq, out_qual, out_bytes);
    return hipGetLastError();
}

}  // namespace

// The segments segs[0 .. n_segs) (device) are called from `cols` / `ins` (n_rows records each) and the frames at `frames`
// (frame_bytes bytes): out_off[0 .. n_segs] (device), the records, and the packed sequences and qualities in out_seq / out_qual
// (out_bytes bytes each; nothing is written behind them).  seg_len: n_segs words of scratch.
hipError_t iock_pile_call(hipStream_t st, const IocPileSeg* segs, uint32_t n_segs, const ioc_pileup_col* cols, const ioc_pileup_ins* ins,
                          uint64_t n_rows, const uint8_t* frames, uint64_t frame_bytes, int32_t min_depth, int64_t* seg_len,
                          ioc_polish_stats* stats, int64_t* out_off, uint8_t* out_seq, uint8_t* out_qual, uint64_t out_bytes)
{
    return pile_call_launch<false>(st, segs, n_segs, cols, ins, nullptr, n_rows, frames, frame_bytes, min_depth, seg_len, stats, out_off, out_seq,
                                   out_qual, out_bytes);
}

// ... by weight (ioc_host_pileup_call_weighted): `cols` (the counts) gates, wcols / wins decide
hipError_t iock_pile_call_weighted(hipStream_t st, const IocPileSeg* segs, uint32_t n_segs, const ioc_pileup_col* cols, const ioc_pileup_col* wcols,
                                   const ioc_pileup_ins* wins, uint64_t n_rows, const uint8_t* frames, uint64_t frame_bytes, int32_t min_depth,
                                   int64_t* seg_len, ioc_polish_stats* stats, int64_t* out_off, uint8_t* out_seq, uint8_t* out_qual,
                                   uint64_t out_bytes)
{
    return pile_call_launch<true>(st, segs, n_segs, wcols, wins, cols, n_rows, frames, frame_bytes, min_depth, seg_len, stats, out_off, out_seq,
                                  out_qual, out_bytes);
}

// k_pile_scan for the stages that count per item of their own (ioc_read_correct.hip): out_off[0 .. n] = the exclusive scan of len
hipError_t iock_pile_scan(hipStream_t st, const int64_t* len, uint32_t n, int64_t* out_off)
{
    hipLaunchKernelGGL(k_pile_scan, dim3(1), dim3(64), 0, st, reinterpret_cast<const long long*>(len), n, reinterpret_cast<long long*>(out_off));
    return hipGetLastError();
}
