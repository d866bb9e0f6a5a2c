// ioc_read_ends.h — the alternative ends of a cluster (ioc_host_reads_ends, isonclust2_hip.h): the small decisions shared between
// the definition on the host (ioc_align.cpp) and the kernels of ioc_read_ends.hip — the rule and what it refuses, what an extent may
// be, the row test, a read's distance to a site, the packed word a site's peak is the largest of, and the key of a (pre_group,
// start site, stop site) triple, whose unsigned order is the order of the variants.  need(N) is that of the site search
// (ioc_pile_sites.h), the run logic on words that of the exon blocks (ioc_read_blocks.h).  tools/read_ends_check.cpp drives the
// word logic on the CPU under the sanitizers, lane by lane as the kernels do; the tests hold the definition against a restatement
// in Python.
#pragma once

#include <cstdint>

#include "isonclust2_hip.h"
#include "ioc_read_blocks.h"

struct EndsRule {  // the thresholds of a search for ends, and those ioc_host_reads_ends refuses
    int32_t slack, min_over, min_depth, min_alt, min_pct, max_sites, max_variants;
    IOC_PILE_HD bool ok() const
    {
        return slack >= 0 && slack <= IOC_ENDS_SLACK_MAX && min_over >= 1 && min_depth >= 1 && min_alt >= 1 && min_pct >= 1 && min_pct <= 100 &&
               max_sites >= 1 && max_sites <= IOC_ENDS_MAX && max_variants >= 1;
    }
    // row p is a start (stop) row: N reads take part, W of them start (stop) within slack rows of p.  One-sided: no "and enough do not".
    // (min_pct <= 100 and N < 2^32: no overflow in need)
    IOC_PILE_HD bool row(uint32_t N, uint32_t W) const
    {
        return N >= uint32_t(min_depth) && (unsigned long long)W >= pile_site_need(PileSiteRule{min_depth, min_alt, min_pct}, N);
    }
};

// what an extent may be on a reference of rlen rows, and whether its read takes part
IOC_PILE_HD bool ends_extent_ok(const ioc_read_extent& e, long long rlen)
{
    return e.first_row >= 0 && (long long)e.end_row <= rlen && e.end_row >= e.first_row && e.head >= 0 && e.tail >= 0;
}
IOC_PILE_HD bool ends_takes_part(const ioc_read_extent& e) { return e.end_row > e.first_row; }

// the sites of one kind a search of max_sites may keep of a segment of rlen rows, and the variants it may keep of so many reads
IOC_PILE_HD long long ends_sites_most(long long rlen, int32_t max_sites) { return rlen + 1 < max_sites ? rlen + 1 : max_sites; }
IOC_PILE_HD long long ends_variants_most(long long reads, int32_t max_variants) { return reads < max_variants ? reads : max_variants; }

// the distance of row x to the site [first, end)
IOC_PILE_HD uint32_t ends_distance(int32_t first, int32_t end, int32_t x) { return x < first ? uint32_t(first - x) : x >= end ? uint32_t(x - end) + 1u : 0u; }
// (distance, site) as one word whose minimum is the nearest site, the lower on a tie; ENDS_FAR: beyond slack, or no site
enum : uint32_t { ENDS_FAR = 0xFFFFFFFFu };
IOC_PILE_HD uint32_t ends_near_word(uint32_t dist, uint32_t site, int32_t slack) { return dist <= uint32_t(slack) ? dist << 8 | site : uint32_t(ENDS_FAR); }
IOC_PILE_HD int32_t ends_near_site(uint32_t word) { return word == uint32_t(ENDS_FAR) ? -1 : int32_t(word & 0xFFu); }

// (count, rlen - row) as one word whose maximum is the row with the largest count, the lowest on a tie; 0: no row
IOC_PILE_HD unsigned long long ends_peak_word(uint32_t count, uint32_t rlen, uint32_t row) { return (unsigned long long)count << 32 | (rlen - row); }
IOC_PILE_HD uint32_t ends_peak_count(unsigned long long w) { return uint32_t(w >> 32); }
IOC_PILE_HD int32_t ends_peak_row(unsigned long long w, uint32_t rlen) { return int32_t(rlen - uint32_t(w)); }

// A placed read's triple as one word: pre_group (>= 0) in the high word, the start site and the stop site (< 32 each) below it.
// Its unsigned order is the order of the variants.  Unplaced reads are told by a flag, never by a key value.
IOC_PILE_HD bool ends_placed(int32_t pre_group, int32_t start_site, int32_t stop_site) { return pre_group >= 0 && start_site >= 0 && stop_site >= 0; }
IOC_PILE_HD unsigned long long ends_key(int32_t pre_group, int32_t start_site, int32_t stop_site)
{
    return (unsigned long long)uint32_t(pre_group) << 32 | (unsigned long long)(uint32_t(start_site) & 0xFFu) << 8 | (uint32_t(stop_site) & 0xFFu);
}

#define IOC_READ_ENDS_WAVES IOC_READ_BLOCKS_WAVES  // waves per workgroup of the kernels of ioc_read_ends.hip, an item each
