// ioc_window_variants.h — two exons at one junction (ioc_host_insert_window_variants, isonclust2_hip.h): the small decisions shared
// between the definition on the host (ioc_align.cpp) and the kernels of ioc_window_variants.hip — what a call refuses, the agreement
// of an alignment from its four counts, the NEAR test, whether round B runs and whether a site splits, a voter's variant and the
// state a read gets in key2.  tools/window_variants_check.cpp drives these on the CPU under the sanitizers, lane by lane as the
// kernels do; the tests hold the definition against a restatement in Python.
#pragma once

#include <cstdint>

#include "isonclust2_hip.h"
#include "ioc_insert_windows.h"
#include "ioc_pile_sites.h"

#define IOC_WINVAR_WAVES 4  // waves per workgroup of the kernels of ioc_window_variants.hip, an item each

struct WinVarRule {  // what a variant call is run with beside the window rule, and what it refuses
    int32_t min_agree, min_alt, min_pct;
    IOC_PILE_HD bool ok() const { return min_agree >= 1 && min_agree <= 100 && min_alt >= 1 && min_pct >= 1 && min_pct <= 50; }
    // need(n_voters): what either side of a split must count, the insert stage's test of a junction
    IOC_PILE_HD uint32_t need(uint32_t n_voters) const { return uint32_t(pile_site_need(PileSiteRule{1, min_alt, min_pct}, n_voters)); }
};

// a (pair, site) entry of a round: not aligned in it, NEAR its template, or not
enum : uint8_t { WINVAR_UNSEEN = 0, WINVAR_NEAR = 1, WINVAR_FAR = 2 };

// the agreement of an alignment with eq '=', x 'X', d 'D' and i 'I' bytes
IOC_PILE_HD int32_t winvar_agreement(uint32_t eq, uint32_t x, uint32_t d, uint32_t i) { return int32_t(eq) - int32_t(x) - int32_t(d) - int32_t(i); }
// The same from a voter's base plane in the template's frame: of the template's tlen rows, eq hold the template's channel and del
// IOC_ALLELE_DEL; every other row is an 'X' and the voter's bases that no row took are 'I'.  (tlen - del <= qlen: a row that is
// no 'D' took a base.)
IOC_PILE_HD int32_t winvar_plane_agreement(uint32_t qlen, uint32_t tlen, uint32_t eq, uint32_t del)
{
    return winvar_agreement(eq, tlen - del - eq, del, qlen - (tlen - del));
}
IOC_PILE_HD bool winvar_near(int32_t a, uint32_t qlen, uint32_t tlen, int32_t min_agree)
{
    return a >= 1 && 100ll * a >= (long long)min_agree * (long long)(qlen > tlen ? qlen : tlen);
}
// round B runs at a site: both sides of round A are large enough
IOC_PILE_HD bool winvar_round_b(const WinVarRule& k, uint32_t n_voters, uint32_t n_far)
{
    return n_far <= n_voters && n_far >= k.need(n_voters) && n_voters - n_far >= k.need(n_voters);
}
// the site splits: round B ran and n_b of its far voters are NEAR template B
IOC_PILE_HD bool winvar_splits(const WinVarRule& k, uint32_t n_voters, uint32_t n_far, uint32_t n_b) { return winvar_round_b(k, n_voters, n_far) && n_b >= k.need(n_voters); }
// a read's variant at a site from its class there and what the two rounds said of it
IOC_PILE_HD uint8_t winvar_variant(uint32_t cls, bool split, uint8_t round_a, uint8_t round_b)
{
    if (cls != uint32_t(IOC_WIN_VOTER)) return IOC_WINVAR_NONE;
    if (!split || round_a == WINVAR_NEAR) return IOC_WINVAR_A;
    return round_b == WINVAR_NEAR ? IOC_WINVAR_B : IOC_WINVAR_OTHER;
}
// the state of key2 at a site: the insert stage's, changed where the site splits
IOC_PILE_HD uint32_t winvar_state(uint32_t state, uint32_t cls, bool split, uint8_t variant)
{
    if (!split || state != uint32_t(IOC_INS_CARRY)) return state;
    if (cls != uint32_t(IOC_WIN_VOTER)) return IOC_INS_NONE;  // (IOC_WIN_SHORT, IOC_WIN_LONG: nobody knows which exon it holds)
    return variant == IOC_WINVAR_B ? uint32_t(IOC_INS_CARRY_B) : variant == IOC_WINVAR_OTHER ? uint32_t(IOC_INS_NONE) : state;
}
