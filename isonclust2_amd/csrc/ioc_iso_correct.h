// ioc_iso_correct.h — the correction of one read against the tables of its own isoform, with a long insertion carried through
// verbatim (ioc_host_read_correct_long, isonclust2_hip.h): what a row emits beside ioc_read_correct.h's row and what makes a pair
// unresolved, shared between the definition on the host (ioc_align.cpp) and k_iso_correct_count / k_iso_correct_emit
// (ioc_iso_correct.hip): a lane forms a row with iso_correct_row.  The base decision, the run guard and the row itself are
// ioc_read_correct.h's (read_base_decide, read_run_exceeds, read_correct_row); nothing of them is written again here.
// tools/iso_correct_check.cpp drives both kernels' steps on the CPU under the sanitizers; the tests hold the definition against a
// restatement in Python.
#pragma once

#include <cstdint>

#include "isonclust2_hip.h"
#include "ioc_read_correct.h"

#define IOC_ISO_CORRECT_WAVES 4  // pairs per workgroup of the kernels of ioc_iso_correct.hip, a wave each

// a length plane byte that says "more than the slot planes hold" / "the plane's cap: the length is not known"
IOC_PILE_HD bool iso_long_row(uint8_t ilen) { return ilen > uint8_t(IOC_PILE_INS_SLOTS); }
IOC_PILE_HD bool iso_len_capped(uint8_t ilen) { return ilen == 255u; }

// the table a pair is held against (§ "which table" of ioc_planes_correct_groups): group-segment gseg_off + group where the pair is in
// a group of at least min_depth members, else the segment's own table behind the G group tables
IOC_PILE_HD bool iso_uses_group(int32_t group, uint32_t members, int32_t min_depth) { return group >= 0 && members >= uint32_t(min_depth); }
// ... and how the record names it: the group-segment's index, or -1 - segment
IOC_PILE_HD int32_t iso_table_name(uint32_t tab, uint32_t n_group_tables) { return tab < n_group_tables ? int32_t(tab) : -1 - int32_t(tab - n_group_tables); }

// What a row emits: `long_len` bytes of the read from query[long_from] on (a long row; else 0), each at quality 0, and behind them
// read_correct_row's bytes — of a long row its base alone, the slot rule is not applied there.  unresolved: the row makes its pair
// unresolved (the length plane's cap, a long run that leaves the read, a long row the read does not span).
struct IsoRowOut {
    ReadRowOut row;
    uint32_t long_len = 0, long_from = 0;
    bool unresolved = false;
    IOC_PILE_HD uint32_t bytes() const { return long_len + row.n; }
};

// Row p <= rlen of a read: read_correct_row's arguments, and ilen / qpos: the row's entries of the read's length and position
// planes; qlen: the read's length.
IOC_PILE_HD IsoRowOut iso_correct_row(const ioc_pileup_col& col, const ioc_pileup_ins& in, unsigned long long D, bool spans, uint8_t own,
                                      unsigned long long slots, uint8_t ilen, uint32_t qpos, uint32_t qlen, uint32_t decision, bool guarded,
                                      const ReadRule& k)
{
    IsoRowOut out;
    const bool lng = iso_long_row(ilen);
    out.unresolved = iso_len_capped(ilen) || (lng && (!spans || (unsigned long long)qpos + ilen > (unsigned long long)qlen));
    out.row = read_correct_row(col, in, D, spans && !lng, own, slots, decision, guarded, k);  // (not spanned: no insertion step)
    if (lng) out.long_len = ilen, out.long_from = qpos;
    return out;
}
