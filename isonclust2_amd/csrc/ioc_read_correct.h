// ioc_read_correct.h — the correction of one read against the pileup of its cluster (ioc_host_read_correct, isonclust2_hip.h):
// the decision of one row, the run guard and what a row emits, shared between the definition on the host (ioc_align.cpp) and
// k_read_correct (ioc_read_correct.hip): a lane decides a row with these functions.  tools/read_correct_check.cpp drives them on the
// CPU under the sanitizers, chunk by chunk as the kernel does; the tests hold them against a restatement in Python.
#pragma once

#include <cstdint>

#include "isonclust2_hip.h"
#include "ioc_pile_call.h"
#include "ioc_pile_sites.h"

struct ReadRule {  // the thresholds of a correction, and those ioc_host_read_correct refuses
    int32_t min_depth, min_alt, min_pct, max_run;
    IOC_PILE_HD bool ok() const { return min_depth >= 1 && min_alt >= 1 && min_pct >= 1 && min_pct <= 50 && max_run >= 0 && max_run <= 64; }
    IOC_PILE_HD unsigned long long need(unsigned long long D) const { return pile_site_need(PileSiteRule{min_depth, min_alt, min_pct}, D); }
};

#define IOC_READ_CORRECT_WAVES 4  // pairs per workgroup of k_read_correct (ioc_read_correct.hip), a wave each

// what is decided about the base of a row: the kind in bits 0 .. 7, the winner's channel (sub, fill) in bits 8 .. 15
enum : uint32_t { READ_NONE = 0, READ_LOW, READ_KEEP, READ_SUB, READ_FILL, READ_REMOVE };
IOC_PILE_HD uint32_t read_kind(uint32_t decision) { return decision & 0xFFu; }
IOC_PILE_HD uint32_t read_winner(uint32_t decision) { return (decision >> 8) & 0xFFu; }

// a base plane byte that says something: a channel or IOC_ALLELE_DEL (IOC_ALLELE_NONE and every byte ioc_host_ops_project does
// not write: nothing); a slot plane byte likewise: 1 + a channel, else 0
IOC_PILE_HD bool read_covers(uint8_t b) { return b <= uint8_t(IOC_ALLELE_DEL); }
IOC_PILE_HD uint32_t read_slot(uint32_t b) { return b >= 1u && b <= 5u ? b : 0u; }
IOC_PILE_HD uint8_t read_letter(uint32_t ch) { return uint8_t(ch == 0u ? 'A' : ch == 1u ? 'C' : ch == 2u ? 'G' : ch == 3u ? 'T' : 'N'); }
IOC_PILE_HD uint32_t read_count(const ioc_pileup_col& c, uint32_t ch)  // (a chain of selects: no indexed array in a lane's registers)
{
    return ch == 0u ? c.a : ch == 1u ? c.c : ch == 2u ? c.g : ch == 3u ? c.t : ch == 4u ? c.other : c.del;
}

// The base of row p < rlen.  col: the row's record; own: base[p] of the read's projection; frame: the reference's base there.
IOC_PILE_HD uint32_t read_base_decide(const ioc_pileup_col& col, uint8_t own, uint8_t frame, const ReadRule& k)
{
    if (!read_covers(own)) return READ_NONE;
    const unsigned long long depth = pile_depth(col);
    if (depth < (unsigned long long)k.min_depth) return READ_LOW;
    if ((unsigned long long)read_count(col, own) >= k.need(depth)) return READ_KEEP;
    const uint32_t cnt[6] = {col.a, col.c, col.g, col.t, col.other, col.del};  // (the winner: pile_call_row's base decision)
    uint32_t most = 0, who = 0;
    for (uint32_t ch = 0; ch < 6u; ++ch)
        if (cnt[ch] > most) most = cnt[ch], who = ch;
    const uint32_t fch = PileAcc::channel(frame);
    if (read_count(col, fch) == most) who = fch;
    if (who == uint32_t(own)) return READ_KEEP;
    if (own == uint8_t(IOC_ALLELE_DEL)) return READ_FILL | who << 8;
    if (who == uint32_t(PILE_DEL)) return READ_REMOVE;
    return READ_SUB | who << 8;
}

// The run guard.  Bit l of `cur`: the row of lane l of a chunk of 64 rows is decided as fill (or as remove: the two are guarded
// apart); prev / next: the same of the chunk before and behind (0 where there is none).  For a lane whose bit is set: whether the
// maximal run of set bits it stands in has more than max_run of them.  max_run <= 64, so a run that reaches through a whole
// neighbour is too long whatever lies beyond it: one chunk either side decides every case.
IOC_PILE_HD bool read_run_exceeds(unsigned long long prev, unsigned long long cur, unsigned long long next, uint32_t lane, int32_t max_run)
{
    const unsigned long long upto = lane == 63u ? ~0ull : (1ull << (lane + 1u)) - 1ull;
    const unsigned long long gap_below = ~cur & upto;  // the rows of the chunk up to the lane that end the run
    uint32_t below;                                     // the run's rows up to the lane, itself included
    if (gap_below)
        below = lane - (63u - uint32_t(__builtin_clzll(gap_below)));
    else
        below = lane + 1u + (~prev ? uint32_t(__builtin_clzll(~prev)) : 64u);
    const unsigned long long gap_above = ~cur >> lane;  // (bit 0: the lane's own, which is set)
    uint32_t above;                                     // the run's rows from the lane on, itself included
    if (gap_above)
        above = uint32_t(__builtin_ctzll(gap_above));
    else
        above = 64u - lane + (~next ? uint32_t(__builtin_ctzll(~next)) : 64u);
    return below + above - 1u > uint32_t(max_run);
}

// What a row emits — PileRowCall's two registers — and what it adds to the read's record.
struct ReadRowOut {
    unsigned long long seq = 0, qual = 0;
    uint32_t n = 0;
    uint32_t n_sub = 0, n_fill = 0, n_remove = 0, n_ins_add = 0, n_ins_drop = 0, n_low = 0, n_guarded = 0;
    IOC_PILE_HD void put(uint8_t base, uint32_t q)
    {
        seq |= (unsigned long long)base << (8u * n);
        qual |= (unsigned long long)(33u + q) << (8u * n);
        ++n;
    }
};

// Row p <= rlen of a read.  col / in: the row's records (col is not read where the decision is READ_NONE, as for p == rlen); D:
// the depth the insertions are held against, D(p) of ioc_host_pileup_sites; spans: the read spans the row (ioc_host_site_alleles);
// own / slots: base[p] and, byte j, slots[j][p] of the read's projection; decision: read_base_decide's; guarded: the row is a fill
// or a remove in a run the guard turns back.
IOC_PILE_HD ReadRowOut read_correct_row(const ioc_pileup_col& col, const ioc_pileup_ins& in, unsigned long long D, bool spans, uint8_t own,
                                        unsigned long long slots, uint32_t decision, bool guarded, const ReadRule& k)
{
    ReadRowOut out;
    if (spans && D < (unsigned long long)k.min_depth) {
        for (uint32_t j = 0; j < uint32_t(IOC_PILE_INS_SLOTS); ++j) {
            const uint32_t s = read_slot(uint32_t(slots >> (8u * j)) & 0xFFu);
            if (s) out.put(read_letter(s - 1u), 0u);
        }
    } else if (spans) {
        const unsigned long long need = k.need(D);
        bool cons = true;
        for (uint32_t j = 0; j < uint32_t(IOC_PILE_INS_SLOTS); ++j) {
            const uint32_t s = read_slot(uint32_t(slots >> (8u * j)) & 0xFFu);
            unsigned long long n = 0;
            uint32_t most = 0, who = 0, mine = 0;
            for (uint32_t ch = 0; ch < 5u; ++ch) {
                const uint32_t v = in.slot[j][ch];
                n += v;
                if (v > most) most = v, who = ch;
                if (ch + 1u == s) mine = v;
            }
            cons = cons && 2ull * n > D;
            if (s) {
                if ((unsigned long long)mine >= need)
                    out.put(read_letter(s - 1u), pile_qual(mine, D));
                else if (cons)
                    out.put(read_letter(who), pile_qual(most, D)), ++out.n_sub;
                else
                    ++out.n_ins_drop;
            } else if (cons && (D > n ? D - n : 0ull) < need) {
                out.put(read_letter(who), pile_qual(most, D)), ++out.n_ins_add;
            }
        }
    }
    uint32_t kind = read_kind(decision);
    if (kind == READ_NONE) return out;
    const unsigned long long depth = pile_depth(col);
    if (kind == READ_LOW) {
        if (own != uint8_t(IOC_ALLELE_DEL)) out.put(read_letter(own), 0u);
        ++out.n_low;
        return out;
    }
    if (guarded && (kind == READ_FILL || kind == READ_REMOVE)) ++out.n_guarded, kind = READ_KEEP;
    if (kind == READ_REMOVE) {
        ++out.n_remove;
        return out;
    }
    const uint32_t ch = kind == READ_KEEP ? uint32_t(own) : read_winner(decision);
    out.n_sub += kind == READ_SUB, out.n_fill += kind == READ_FILL;
    if (ch != uint32_t(PILE_DEL)) out.put(read_letter(ch), pile_qual(read_count(col, ch), depth));
    return out;
}

#if defined(__HIPCC__)
// Device code only from here on: a lane fetches its row and decides it.  What a wave of k_read_correct, and of the kernels of
// ioc_iso_correct.hip, reads of its pair: the tables, the frames and the planes with their sizes, and where the pair's rows lie in
// them.
struct ReadPairView {
    const ioc_pileup_col* __restrict__ cols;
    const ioc_pileup_ins* __restrict__ ins;
    uint64_t n_rows;
    const uint8_t* __restrict__ frames;
    uint64_t frame_bytes;
    const uint8_t* __restrict__ base_planes;
    const uint8_t* __restrict__ slot_planes;
    uint64_t plane_bytes;
    IocPileSeg s;
    uint64_t po;  // the pair's first byte in every plane

    // row p <= rlen lies inside everything that was passed
    __device__ __forceinline__ bool inside(uint32_t p) const
    {
        const uint32_t rlen = uint32_t(s.rlen);
        if (uint64_t(s.row0) + p >= n_rows || po + p >= plane_bytes) return false;
        return p >= rlen || uint64_t(s.f_off) + (s.rc ? rlen - 1u - p : p) < frame_bytes;
    }
    // the decision of the base of row p (READ_NONE for row rlen and for a row outside)
    __device__ __forceinline__ uint32_t decide(uint32_t p, const ReadRule& k) const
    {
        const uint32_t rlen = uint32_t(s.rlen);
        if (p >= rlen || !inside(p)) return READ_NONE;
        const uint64_t at = uint64_t(s.f_off) + (s.rc ? rlen - 1u - p : p);
        const uint8_t fb = s.rc ? comp_base(frames[at]) : frames[at];
        return read_base_decide(cols[uint64_t(s.row0) + p], base_planes[po + p], fb, k);
    }
    // Row p <= rlen fetched and formed: form(r, at, D, spans, own, slots) takes the row of the tables, the row's byte in every plane
    // and what read_correct_row takes of the planes; a row outside, of which nothing is read, yields form's result as it is made.
    template <class Form>
    __device__ __forceinline__ auto row_as(uint32_t p, Form form) const -> decltype(form(uint64_t(0), uint64_t(0), 0ull, false, uint8_t(0), 0ull))
    {
        const uint32_t rlen = uint32_t(s.rlen);
        if (p > rlen || !inside(p)) return decltype(form(uint64_t(0), uint64_t(0), 0ull, false, uint8_t(0), 0ull)){};
        const uint64_t r = uint64_t(s.row0) + p, at = po + p;
        const bool has_base = p < rlen;
        // (row rlen: the depth and the span of row rlen - 1, which lies inside where row rlen does)
        const unsigned long long D = has_base ? pile_depth(cols[r]) : rlen > 0u ? pile_depth(cols[r - 1u]) : 0ull;
        const uint8_t own = base_planes[at];
        const uint8_t span = has_base ? own : rlen > 0u ? base_planes[at - 1u] : uint8_t(IOC_ALLELE_NONE);
        unsigned long long slots = 0;
#pragma unroll
        for (uint32_t j = 0; j < uint32_t(IOC_PILE_INS_SLOTS); ++j) slots |= (unsigned long long)slot_planes[uint64_t(j) * plane_bytes + at] << (8u * j);
        return form(r, at, D, read_covers(span), own, slots);
    }
    // what row p emits, its decision and the guard's verdict known
    __device__ __forceinline__ ReadRowOut row(uint32_t p, uint32_t decision, bool guarded, const ReadRule& k) const
    {
        return row_as(p, [&](uint64_t r, uint64_t, unsigned long long D, bool spans, uint8_t own, unsigned long long slots) {
            return read_correct_row(cols[r], ins[r], D, spans, own, slots, decision, guarded, k);
        });
    }
};
#endif
