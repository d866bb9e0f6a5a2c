// ioc_pile_call.h — the decision of one row of a consensus call (ioc_host_pileup_call, isonclust2_hip.h), shared between the
// definition on the host (ioc_align.cpp) and the call kernels (ioc_pile_call.hip): a lane decides a row with this function.
// tools/pile_call_check.cpp and tools/pile_weight_check.cpp drive it on the CPU under the sanitizers; the tests hold both against a
// restatement in Python.
#pragma once

#include <cstdint>

#include "isonclust2_hip.h"
#include "ioc_ops_pileup.h"

// What a row emits: 0 to IOC_PILE_INS_SLOTS inserted bases and then 0 or 1 base of its own, byte x of `seq` / `qual` in bits
// 8x .. 8x + 7 (qualities as written: 33 + q), and what it adds to the segment's record.
struct PileRowCall {
    unsigned long long seq = 0, qual = 0;
    uint32_t n = 0;
    uint32_t n_ins = 0, n_sub = 0, n_del = 0, n_low = 0;
    IOC_PILE_HD void put(uint8_t base, uint32_t q)
    {
        seq |= (unsigned long long)base << (8u * n);
        qual |= (unsigned long long)(33u + q) << (8u * n);
        ++n;
    }
};

#define IOC_PILE_CALL_CHUNK 256  // rows a workgroup of the call kernels takes per step (ioc_pile_call.hip)
constexpr uint32_t PILE_CALL_MAX_ROW = IOC_PILE_INS_SLOTS + 1;  // bytes a row can emit

IOC_PILE_HD unsigned long long pile_depth(const ioc_pileup_col& c)
{
    return (unsigned long long)c.a + c.c + c.g + c.t + c.other + c.del;
}

IOC_PILE_HD uint32_t pile_qual(unsigned long long most, unsigned long long depth)  // (depth > 0; most < 2^33: no overflow)
{
    const unsigned long long q = 40ull * most / depth;
    return q < 40ull ? uint32_t(q) : 40u;
}

// Row p of a segment.  col / in: its records (col is not read where has_base is false and d_ins comes from the row before);
// d_ins: the depth its insertions are held against; has_base: p < rlen, and then `frame` is frame[p].  The two gates: c_ins and
// c_base are the depths that min_depth is held against, of the insertions and of the row's own base.  The majority call passes
// d_ins and the depth of col; the weighted call (ioc_host_pileup_call_weighted) decides on tables of weights and passes the
// depths of the table of counts, and a row whose weights sum to 0 is then as good as not covered.
IOC_PILE_HD PileRowCall pile_call_row(const ioc_pileup_col& col, const ioc_pileup_ins& in, unsigned long long d_ins, bool has_base,
                                      uint8_t frame, int32_t min_depth, unsigned long long c_ins, unsigned long long c_base)
{
    const char letter[5] = {'A', 'C', 'G', 'T', 'N'};
    PileRowCall out;
    const unsigned long long need = (unsigned long long)min_depth;
    if (c_ins >= need && d_ins > 0ull) {
        for (uint32_t s = 0; s < uint32_t(IOC_PILE_INS_SLOTS); ++s) {
            unsigned long long n = 0;
            uint32_t most = 0, who = 0;
            for (uint32_t ch = 0; ch < 5u; ++ch) {
                const uint32_t v = in.slot[s][ch];
                n += v;
                if (v > most) most = v, who = ch;
            }
            if (!(2ull * n > d_ins)) break;
            out.put(uint8_t(letter[who]), pile_qual(most, d_ins));
            ++out.n_ins;
        }
    }
    if (!has_base) return out;
    const unsigned long long depth = pile_depth(col);
    if (c_base < need || depth == 0ull) {
        out.put(frame, 0u);
        ++out.n_low;
        return out;
    }
    const uint32_t cnt[6] = {col.a, col.c, col.g, col.t, col.other, col.del};
    uint32_t most = 0, who = 0;
    for (uint32_t ch = 0; ch < 6u; ++ch)
        if (cnt[ch] > most) most = cnt[ch], who = ch;
    const uint32_t fch = PileAcc::channel(frame);
    if (cnt[fch] == most) who = fch;
    if (who == uint32_t(PILE_DEL)) {
        ++out.n_del;
        return out;
    }
    if (who != fch) ++out.n_sub;
    out.put(who == fch ? frame : uint8_t(letter[who]), pile_qual(most, depth));
    return out;
}

// the majority call's row: one table, which is its own gate
IOC_PILE_HD PileRowCall pile_call_row(const ioc_pileup_col& col, const ioc_pileup_ins& in, unsigned long long d_ins, bool has_base,
                                      uint8_t frame, int32_t min_depth)
{
    return pile_call_row(col, in, d_ins, has_base, frame, min_depth, d_ins, has_base ? pile_depth(col) : 0ull);
}

#if defined(__HIPCC__)
// Device code only from here on: a lane of the call kernels (ioc_pile_call.hip, ioc_iso_splice.hip) fetches its row and decides it.
#include <hip/hip_runtime.h>

#include "ioc_sink_plan.h"

// the complement of a frame byte where a segment is read reverse-complemented (the aligner's rule, ioc_align_gpu.hip, which keeps
// its own copy beside its kernels: anything but A C G T stays)
__device__ __forceinline__ uint8_t comp_base(uint8_t ch)
{
    return ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : ch;
}

// Row p of segment s (p <= s.rlen) fetched and called, or nothing where its records or its frame byte lie outside what was passed.
// WEIGHTED (ioc_host_pileup_call_weighted): cols / ins are the tables of weights, which decide, and `gate` is the table of counts,
// whose depths min_depth is held against (n_rows records like the others); the majority call does not read `gate`.
template <bool WEIGHTED>
__device__ __forceinline__ PileRowCall pile_call_seg_row(const IocPileSeg& s, uint32_t p, const ioc_pileup_col* __restrict__ cols,
                                                         const ioc_pileup_ins* __restrict__ ins, const ioc_pileup_col* __restrict__ gate,
                                                         uint64_t n_rows, const uint8_t* __restrict__ frames, uint64_t frame_bytes, int32_t min_depth)
{
    const uint32_t rlen = uint32_t(s.rlen);
    const uint64_t row = uint64_t(s.row0) + p;
    if (row >= n_rows) return PileRowCall{};
    const bool has_base = p < rlen;
    uint8_t fb = 0;
    if (has_base) {
        const uint64_t at = uint64_t(s.f_off) + (s.rc ? rlen - 1u - p : p);
        if (at >= frame_bytes) return PileRowCall{};
        fb = s.rc ? comp_base(frames[at]) : frames[at];
    }
    const unsigned long long d_ins = has_base ? pile_depth(cols[row]) : rlen > 0u ? pile_depth(cols[row - 1u]) : 0ull;
    if (!WEIGHTED) return pile_call_row(cols[row], ins[row], d_ins, has_base, fb, min_depth);
    const unsigned long long c_ins = has_base ? pile_depth(gate[row]) : rlen > 0u ? pile_depth(gate[row - 1u]) : 0ull;
    return pile_call_row(cols[row], ins[row], d_ins, has_base, fb, min_depth, c_ins, has_base ? pile_depth(gate[row]) : 0ull);
}
#endif
