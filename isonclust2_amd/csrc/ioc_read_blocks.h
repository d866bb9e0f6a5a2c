// ioc_read_blocks.h — the exon blocks of a cluster and every read's isoform (ioc_host_planes_blocks, isonclust2_hip.h): the small
// decisions shared between the definition on the host (ioc_align.cpp) and the kernels of ioc_read_blocks.hip — need(D), the
// variable-row test, a block's state, key agreement under a mask — and the word logic the kernels run on bit planes: which bits of
// a 64-row word stand in a run of at least so many rows, given what the run carries in from either side.  tools/read_blocks_check.cpp
// drives the word logic on the CPU under the sanitizers, lane by lane as the kernels do; the tests hold the definition against a
// restatement in Python.
#pragma once

#include <cstdint>

#include "isonclust2_hip.h"
#include "ioc_pile_call.h"
#include "ioc_pile_sites.h"

struct BlocksRule {  // the thresholds of a block search, and those ioc_host_planes_blocks refuses
    int32_t min_gap, min_depth, min_alt, min_pct, min_block, max_blocks;
    IOC_PILE_HD bool ok() const
    {
        return min_gap >= 1 && min_depth >= 1 && min_alt >= 1 && min_pct >= 1 && min_pct <= 50 && min_block >= 1 && max_blocks >= 1 &&
               max_blocks <= IOC_BLOCKS_MAX;
    }
    IOC_PILE_HD unsigned long long need(unsigned long long D) const { return pile_site_need(PileSiteRule{min_depth, min_alt, min_pct}, D); }
};

#define IOC_READ_BLOCKS_WAVES 4  // waves per workgroup of the kernels of ioc_read_blocks.hip, an item each

// a base plane byte that covers its row: a channel or IOC_ALLELE_DEL
IOC_PILE_HD bool blocks_covers(uint8_t b) { return b <= uint8_t(IOC_ALLELE_DEL); }

// row p is variable: D reads cover it, `in` of them with a long gap
IOC_PILE_HD bool blocks_row_variable(const BlocksRule& k, uint32_t D, uint32_t in)
{
    if (D < uint32_t(k.min_depth) || in > D) return false;
    const unsigned long long need = k.need(D);
    return (unsigned long long)in >= need && (unsigned long long)(D - in) >= need;
}

// a read's state at a block of len rows of which it covers c and has s deleted
IOC_PILE_HD uint32_t blocks_state(uint32_t len, uint32_t c, uint32_t s)
{
    if (c < len) return IOC_BLOCK_NONE;
    if (4ull * s >= 3ull * len) return IOC_BLOCK_SKIP;
    if (4ull * s <= (unsigned long long)len) return IOC_BLOCK_KEEP;
    return IOC_BLOCK_PART;
}

// The mask of a key: both bits of every block at which the state is not NONE; the mask of a complete read of n_blocks blocks.
IOC_PILE_HD unsigned long long blocks_state_mask(uint32_t b, uint32_t state) { return state == uint32_t(IOC_BLOCK_NONE) ? 0ull : 3ull << (2u * b); }
IOC_PILE_HD unsigned long long blocks_full_mask(uint32_t n_blocks) { return n_blocks >= 32u ? ~0ull : (1ull << (2u * n_blocks)) - 1ull; }
// a supported key agrees with a read's key at every block the mask names
IOC_PILE_HD bool blocks_key_agrees(unsigned long long key, unsigned long long supported, unsigned long long mask) { return ((key ^ supported) & mask) == 0ull; }

// ---- runs of set bits across 64-bit words ----
// A plane of bits is held 64 rows a word, bit l the row 64 w + l; a wave holds 64 words at a time, lane w word w.  A run's length
// is only ever compared with a least length `sat`, so it is carried saturated: min(length, sat), sat < 2^31.
IOC_PILE_HD uint32_t run_sat(unsigned long long v, uint32_t sat) { return v > (unsigned long long)sat ? sat : uint32_t(v); }
IOC_PILE_HD uint32_t run_trail(unsigned long long w) { return ~w ? uint32_t(__builtin_clzll(~w)) : 64u; }  // the set bits from bit 63 down
IOC_PILE_HD uint32_t run_lead(unsigned long long w) { return ~w ? uint32_t(__builtin_ctzll(~w)) : 64u; }   // the set bits from bit 0 up
// `nonfull`: bit j says that word j of the batch has a clear bit.  The nearest such word below / above lane's (64: none)
IOC_PILE_HD uint32_t run_src_below(unsigned long long nonfull, uint32_t lane)
{
    const unsigned long long below = nonfull & ((1ull << lane) - 1ull);
    return below ? 63u - uint32_t(__builtin_clzll(below)) : 64u;
}
IOC_PILE_HD uint32_t run_src_above(unsigned long long nonfull, uint32_t lane)
{
    const unsigned long long above = lane >= 63u ? 0ull : nonfull & ~((2ull << lane) - 1ull);
    return above ? uint32_t(__builtin_ctzll(above)) : 64u;
}
// The run that ends right below lane's word: src = run_src_below, src_trail = run_trail of word src (anything where src == 64),
// carry = the same of the batch's first word.  And the run that begins right above it, likewise.
IOC_PILE_HD uint32_t run_left_in(uint32_t lane, uint32_t src, uint32_t src_trail, uint32_t carry, uint32_t sat)
{
    return src < 64u ? run_sat(64ull * (lane - 1u - src) + src_trail, sat) : run_sat(64ull * lane + carry, sat);
}
IOC_PILE_HD uint32_t run_right_in(uint32_t lane, uint32_t src, uint32_t src_lead, uint32_t carry, uint32_t sat)
{
    return src < 64u ? run_sat(64ull * (src - 1u - lane) + src_lead, sat) : run_sat(64ull * (63u - lane) + carry, sat);
}
// The bits of w that stand in a run of at least `least` set bits, where the run that reaches bit 0 has `left` more bits below the
// word and the one that reaches bit 63 `right` more above it (both saturated at `least`).
IOC_PILE_HD unsigned long long run_long_bits(unsigned long long w, uint32_t left, uint32_t right, uint32_t least)
{
    unsigned long long out = 0, x = w;
    while (x) {
        const unsigned long long low = x & (~x + 1ull), run = x & ~(x + low);  // the lowest run of x
        unsigned long long len = (unsigned long long)__builtin_popcountll(run);
        if (run & 1ull) len += left;
        if (run >> 63) len += right;
        if (len >= (unsigned long long)least) out |= run;
        x &= ~run;
    }
    return out;
}
// the bits at which a run of q begins / ends, given that the run at bit 0 comes from below (left > 0) / goes on above (right > 0)
IOC_PILE_HD unsigned long long run_starts(unsigned long long q, uint32_t left) { return q & ~((q << 1) | (left > 0u ? 1ull : 0ull)); }
IOC_PILE_HD unsigned long long run_ends(unsigned long long q, uint32_t right) { return q & ~((q >> 1) | (right > 0u ? 1ull << 63 : 0ull)); }
// the bits of a word that lie in rows [first, end) when the word's first row is row0
IOC_PILE_HD unsigned long long run_row_mask(long long row0, long long first, long long end)
{
    const long long lo = first > row0 ? first - row0 : 0, hi = end - row0 < 64 ? end - row0 : 64;
    if (lo >= hi) return 0ull;
    const unsigned long long upto = hi >= 64 ? ~0ull : (1ull << hi) - 1ull;
    return upto & ~((1ull << lo) - 1ull);
}
