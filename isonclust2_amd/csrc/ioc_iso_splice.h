// ioc_iso_splice.h — the plan and the row logic of an isoform's splice (ioc_host_isoform_splice, isonclust2_hip.h), shared between
// the definition on the host (ioc_align.cpp) and the kernels of ioc_iso_splice.hip: the plan kernel walks the sites with
// splice_state, a lane of the call kernel asks splice_row what its row is.  tools/iso_splice_check.cpp restates both kernels lane by
// lane on the CPU under the sanitizers (tools/iso_splice_variants_check.cpp the slot-aware plan); the tests hold the definition against a restatement in Python.
#pragma once

#include <cstdint>

#include "isonclust2_hip.h"
#include "ioc_ops_pileup.h"

// One DONE site of an isoform: the rows [lo, hi) are replaced by `len` bytes that stand at `off` of the packed windows; `site` is
// the site's index in its segment.  The intervals of a plan ascend and do not overlap: lo of one is at least hi of the one before.
struct IocSpliceIv {
    int32_t lo, hi;
    int32_t len, site;
    int64_t off;
};
#define IOC_SPLICE_PLAN_MAX IOC_INSERTS_MAX  // intervals a plan holds at most: a site each
static_assert(sizeof(IocSpliceIv) == 24, "plan layout");

// Rule 1 for a site once it is known whether the key carries it, and with which template length, given the hi of the last DONE site
// in front of it (0 without: every lo is at least 1)
IOC_PILE_HD int32_t splice_state_of(bool carries, int32_t tlen, int32_t lo, int32_t last_hi)
{
    if (!carries) return IOC_SPLICE_LACK;
    if (tlen == 0) return IOC_SPLICE_UNCALLED;
    return lo < last_hi ? IOC_SPLICE_OVERLAP : IOC_SPLICE_DONE;
}
// ... for site b under an insert key: the window is the site's one
IOC_PILE_HD int32_t splice_state(uint64_t key, uint32_t b, const ioc_insert_window& w, int32_t last_hi)
{
    return splice_state_of(((key >> (2u * b)) & 3u) == uint64_t(IOC_INS_CARRY), w.tlen, w.lo, last_hi);
}

// The splice by variant (ioc_host_isoform_splice_variants): which of a site's two slots a key2 state takes — 0: slot 2 b, variant A;
// 1: slot 2 b + 1, variant B; -1: the state carries nothing — and the template length that slot was called from.  A key may claim B
// where nothing split: that length is 0 and the site UNCALLED.
IOC_PILE_HD int32_t splice_variant_which(uint32_t state)
{
    return state == uint32_t(IOC_INS_CARRY) ? 0 : state == uint32_t(IOC_INS_CARRY_B) ? 1 : -1;
}
IOC_PILE_HD int32_t splice_variant_tlen(int32_t which, const ioc_insert_window& w, const ioc_window_variant& v)
{
    return which == 0 ? w.tlen : v.split ? v.tlen_b : 0;
}
// ... and rule 1 for site b under a key2
IOC_PILE_HD int32_t splice_state_variants(uint64_t key, uint32_t b, const ioc_insert_window& w, const ioc_window_variant& v, int32_t last_hi)
{
    const int32_t which = splice_variant_which(uint32_t(key >> (2u * b)) & 3u);
    return splice_state_of(which >= 0, which >= 0 ? splice_variant_tlen(which, w, v) : 0, w.lo, last_hi);
}

// What row p is under a plan of n intervals: IOC_SPLICE_ROW_CALL, a row that is called as always; the index of the interval that
// begins at p, whose window stands there; IOC_SPLICE_ROW_GONE, a later row of an interval, which emits nothing.
#define IOC_SPLICE_ROW_CALL (-1)
#define IOC_SPLICE_ROW_GONE (-2)
IOC_PILE_HD int32_t splice_row(const IocSpliceIv* iv, uint32_t n, int32_t p)
{
    for (uint32_t x = 0; x < n; ++x) {
        if (p < iv[x].lo) break;  // (ascending)
        if (p < iv[x].hi) return p == iv[x].lo ? int32_t(x) : IOC_SPLICE_ROW_GONE;
    }
    return IOC_SPLICE_ROW_CALL;
}
