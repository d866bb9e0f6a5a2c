// ioc_site_split.h — the four small rules of the split of a cluster's reads by linked sites (ioc_host_alleles_split,
// isonclust2_hip.h), shared between the definition on the host (ioc_align.cpp) and the kernels of ioc_site_split.hip: the mark of
// an allele byte, d of two sites from their four 64-bit words, the phase of a sum and the group of a vote.
// tools/site_split_check.cpp drives them, and a lane-by-lane restatement of the kernels' indexing, on the CPU under the
// sanitizers; the tests hold the host function against a restatement in Python.
#pragma once

#include <cstdint>

#include "isonclust2_hip.h"
#include "ioc_ops_pileup.h"

// m(i, s): +1 for the site's minor allele, -1 for its major, 0 for anything else (the minor is asked first)
IOC_PILE_HD int32_t split_mark(uint8_t allele, int32_t minor, int32_t major)
{
    return int32_t(allele) == minor ? 1 : int32_t(allele) == major ? -1 : 0;
}

IOC_PILE_HD int32_t split_popc(unsigned long long v) { return __builtin_popcountll(v); }  // (host and device alike)

// What one word of 64 reads adds to d(s, t): ms / Ms = the reads that carry the minor / the major at s, mt / Mt at t.  (A read has
// at most one of the two bits of a site, so the four sets are disjoint; the same words with the group masks in place of a site's
// give dg(t): group 1 as "minor", group 0 as "major".)
IOC_PILE_HD int32_t split_d_word(unsigned long long ms, unsigned long long Ms, unsigned long long mt, unsigned long long Mt)
{
    return split_popc(ms & mt) + split_popc(Ms & Mt) - split_popc(ms & Mt) - split_popc(Ms & mt);
}

// phase of a sum d: its sign where |d| >= min_link, else 0
IOC_PILE_HD int8_t split_phase(long long d, int32_t min_link)
{
    return d >= (long long)min_link ? int8_t(1) : d <= -(long long)min_link ? int8_t(-1) : int8_t(0);
}

// group of a vote: 1, 0 or IOC_SPLIT_NONE
IOC_PILE_HD uint8_t split_group(long long vote, int32_t min_margin)
{
    return vote >= (long long)min_margin ? uint8_t(1) : vote <= -(long long)min_margin ? uint8_t(0) : uint8_t(IOC_SPLIT_NONE);
}
