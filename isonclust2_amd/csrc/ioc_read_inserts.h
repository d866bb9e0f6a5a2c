// ioc_read_inserts.h — the insertion sites of a cluster and every read's combined isoform (ioc_host_planes_inserts,
// isonclust2_hip.h): the small decisions shared between the definition on the host (ioc_align.cpp) and the kernels of
// ioc_read_inserts.hip — the rule and what it refuses, the byte of a length plane, the window of a junction, a site's state, and
// agreement and order of two-word keys.  The variable-junction test, need(D), the masks and the run logic on words are those of the
// exon blocks (ioc_read_blocks.h).  tools/read_inserts_check.cpp drives the word logic on the CPU under the sanitizers, lane by lane
// as the kernels do; the tests hold the definition against a restatement in Python.
#pragma once

#include <cstdint>

#include "isonclust2_hip.h"
#include "ioc_read_blocks.h"

struct InsertsRule {  // the thresholds of a site search, and those ioc_host_planes_inserts refuses
    int32_t min_ins, slack, min_depth, min_alt, min_pct, max_sites;
    IOC_PILE_HD bool ok() const
    {
        return min_ins >= 1 && min_ins <= 255 && slack >= 0 && slack <= IOC_INS_SLACK_MAX && min_depth >= 1 && min_alt >= 1 && min_pct >= 1 &&
               min_pct <= 50 && max_sites >= 1 && max_sites <= IOC_INSERTS_MAX;
    }
    // junction p is variable: S reads span it, `in` of them near an insertion — the test of a block's rows
    IOC_PILE_HD bool variable(uint32_t S, uint32_t in) const { return blocks_row_variable(BlocksRule{1, min_depth, min_alt, min_pct, 1, 1}, S, in); }
};

#define IOC_READ_INSERTS_WAVES 4  // waves per workgroup of the kernels of ioc_read_inserts.hip, an item each

// the byte of a length plane for a run of n 'I'
IOC_PILE_HD uint8_t inserts_len_byte(unsigned long long n) { return uint8_t(n > 255ull ? 255ull : n); }
// the junctions a segment of rlen rows has (1 .. rlen - 1), and the sites a search of max_sites may keep of it
IOC_PILE_HD long long inserts_junctions(long long rlen) { return rlen > 1 ? rlen - 1 : 0; }
IOC_PILE_HD long long inserts_sites_most(long long rlen, int32_t max_sites) { return inserts_junctions(rlen) < max_sites ? inserts_junctions(rlen) : max_sites; }
// the window of junction p: rows lo .. hi of the length plane, both included
IOC_PILE_HD long long inserts_win_lo(long long p, int32_t slack) { return p > slack ? p - slack : 0; }
IOC_PILE_HD long long inserts_win_hi(long long p, int32_t slack, long long rlen) { return p + slack < rlen ? p + slack : rlen; }

// a read's state at a site of len junctions of which it spans c and is near an insertion at s
IOC_PILE_HD uint32_t inserts_state(uint32_t len, uint32_t c, uint32_t s) { return c < len ? IOC_INS_NONE : s > 0u ? IOC_INS_CARRY : IOC_INS_LACK; }

// two-word keys, the block stage's word major: agreement under both masks, and the order of the isoforms
IOC_PILE_HD bool inserts_key_agrees(unsigned long long pre, unsigned long long key, unsigned long long s_pre, unsigned long long s_key,
                                    unsigned long long pre_mask, unsigned long long mask)
{
    return blocks_key_agrees(pre, s_pre, pre_mask) && blocks_key_agrees(key, s_key, mask);
}
IOC_PILE_HD bool inserts_key_less(unsigned long long a_pre, unsigned long long a_key, unsigned long long b_pre, unsigned long long b_key)
{
    return a_pre < b_pre || (a_pre == b_pre && a_key < b_key);
}
