// ioc_pile_sites.h — the decision of one row of a site search (ioc_host_pileup_sites, isonclust2_hip.h), shared between the
// definition on the host (ioc_align.cpp) and the kernels of ioc_pile_sites.hip: a lane decides a row with this function; and the
// allele of one read at one site (ioc_host_site_alleles), shared in the same way.  tools/pile_sites_check.cpp drives both on the
// CPU under the sanitizers; the tests hold them against a restatement in Python.
#pragma once

#include <cstdint>

#include "isonclust2_hip.h"
#include "ioc_pile_call.h"

// What a row yields: its insertion site and / or its base site, the insertion site first.
struct PileRowSites {
    ioc_pile_site ins, base;
    bool has_ins = false, has_base = false;
    IOC_PILE_HD uint32_t n() const { return uint32_t(has_ins) + uint32_t(has_base); }
};

struct PileSiteRule {
    int32_t min_depth, min_alt, min_pct;
};

IOC_PILE_HD uint32_t pile_sat32(unsigned long long v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(v); }

// need(D) = max(min_alt, ceil(min_pct * D / 100)); D < 6 * 2^32 and min_pct <= 50: no overflow
IOC_PILE_HD unsigned long long pile_site_need(const PileSiteRule& k, unsigned long long D)
{
    const unsigned long long pct = ((unsigned long long)k.min_pct * D + 99ull) / 100ull;
    return pct > (unsigned long long)k.min_alt ? pct : (unsigned long long)k.min_alt;
}

// Row p of a reference.  col: its record (of row rlen only ins_runs is read); d_ins: the depth its insertions are held against,
// D(p); has_base: p < rlen.
IOC_PILE_HD PileRowSites pile_sites_row(const ioc_pileup_col& col, unsigned long long d_ins, bool has_base, int32_t p, const PileSiteRule& k)
{
    PileRowSites out;
    if (d_ins >= (unsigned long long)k.min_depth) {
        const unsigned long long with = col.ins_runs, without = d_ins > with ? d_ins - with : 0ull, need = pile_site_need(k, d_ins);
        if (with >= need && without >= need) {
            const bool present = with > without;  // (a tie goes to "absent")
            out.has_ins = true;
            out.ins = ioc_pile_site{p, IOC_SITE_INS, present ? 1 : 0, present ? 0 : 1, pile_sat32(d_ins), pile_sat32(present ? with : without),
                                    pile_sat32(present ? without : with), 0u};
        }
    }
    if (!has_base) return out;
    const unsigned long long depth = pile_depth(col);
    if (depth < (unsigned long long)k.min_depth) return out;
    const uint32_t cnt[6] = {col.a, col.c, col.g, col.t, col.other, col.del};
    uint32_t major = 0, minor = 6;
    for (uint32_t ch = 1; ch < 6u; ++ch)
        if (cnt[ch] > cnt[major]) major = ch;
    for (uint32_t ch = 0; ch < 6u; ++ch)
        if (ch != major && (minor == 6u || cnt[ch] > cnt[minor])) minor = ch;
    if ((unsigned long long)cnt[minor] >= pile_site_need(k, depth)) {
        out.has_base = true;
        out.base = ioc_pile_site{p, IOC_SITE_BASE, int32_t(major), int32_t(minor), pile_sat32(depth), cnt[major], cnt[minor], 0u};
    }
    return out;
}

// The allele of a read at a site: b_row = base[row] of its projection (anything where row == rlen), i_row = insf[row], b_last =
// base[rlen - 1] (IOC_ALLELE_NONE where rlen == 0).
IOC_PILE_HD uint8_t pile_site_allele(int32_t kind, bool last_row, uint8_t b_row, uint8_t i_row, uint8_t b_last)
{
    if (kind == IOC_SITE_BASE) return b_row;
    const uint8_t span = last_row ? b_last : b_row;
    return span != uint8_t(IOC_ALLELE_NONE) ? i_row : uint8_t(IOC_ALLELE_NONE);
}
