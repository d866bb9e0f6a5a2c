// align_plan_check.cpp — the batched aligner's host planner (isonclust2_amd/csrc/ioc_align_plan.h), driven on the CPU over a fixed
// sweep of the smallest shapes at which each of its rules can break, and held against the conditions the kernels rely on:
//
//  * bands: bstart[0] = 0, strictly ascending over nbands, bstart[nbands] = the coarse rows, 1 <= nbands <= V2_MAX_BANDS;
//  * the corridor: plo <= phi < nstrips in every band, neither falls down the bands, every band holds the strips of its own diagonal
//    cells — and, stated directly, no computed tile off the border lacks both the tile above it and the tile to its left; the
//    probe's rectangle inside the corridor with plo = 0 and reached by both pairs; a fifth of the grid skipped; the parent bound and
//    the start bound against a restatement written here, by enumeration of the skipped tiles; without a corridor plo = 0,
//    phi = nstrips - 1, cert = INT32_MIN, start = INT32_MAX;
//  * the tile list: tile_counts' closed forms against what tile_lists produces (tile_lists_check); in every list the probe's tiles
//    first, then every tile of every couple exactly once, each after the tile above it and the tile to its left;
//  * slices: every couple in exactly one, in order; a slice of several couples within the budget (checkpoints, profiles, operation
//    bytes); the four checkpoint regions of a slice's couples disjoint, starting at multiples of 4 words; profile ranges disjoint;
//    pck of every pair its couple's; arena_words and prof_total the largest slice's;
//  * version 1: every pair from n_v2 on in exactly one slice, one kernel family per slice, regions disjoint, the row pitch a multiple
//    of 16 int2 and row_off / col_off multiples of 4 int2 (the int4 stores need 16 bytes), ops_end ascending within a slice; plan_waves a power of two in 1 .. ALN_MAXW that meets the rule it states (a forced
//    count: that count);
//  * the real plan against the certificate: seven pairs of 5 - 9 kb (five related, two unrelated), the bands and plo / phi that
//    plan_couples planned — tapered and one width — handed to ioc_host_align_corridor; wherever its score strictly beats
//    min(parent, max(start, exit)) the score, end cell and operation string are ioc_host_align_ops', byte for byte.  With the
//    sequences of seed 20260 all five related pairs (summed error rates 0.06, 0.12, 0.16, 0.20, 0.24) certify, under the taper and
//    under one width; the two unrelated pairs never do.
//
// The sweep: lengths 1, 511 .. 513, 1023 .. 1025 (a strip's edge), 2047 .. 2049, 4600, 16 700, 20 480 and 20 481 (40 and 41 coarse
// rows: V2_MAX_BANDS, the merge from the middle), 70 000, and one couple of n = 1 against m = 2^26 - 2 (65 536 strips: the 16-bit
// strip); couples of two equal pairs, of a long query on a short reference with its mirror image, of two different lengths, and a
// last couple of one pair; summed error rates 0, 0.02, 0.1, 0.3, 1 and NaN over the gap-open classes 2 .. 5 and a negative one;
// the fitted line absent and present (pairs inside and outside its range); scores 2 / -2 / 1, 1 / -1 / 1 and a set with match 0;
// the taper on and off, margins 0 and 256, fixed fractions 0, 0.2 and 1, the every-tile route; band targets 12, 17, 40 and — no call
// asks for it, but a target within V2_MAX_BANDS never leaves plan_bands more heights than that to merge — 64; budgets of nothing
// and of everything, with and without operation bytes.
//
// Every plan's fields go into a digest, field by field (no padding enters): one line per group of plans, `--all` one per plan.
// Two builds of the planner plan alike iff their lines are equal.
//
// Host code only, meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/align_plan_check tools/align_plan_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/align_plan_check
//
// Exit status 0 and "ok" when everything holds; a line naming the shape for every condition that does not.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ioc_align_plan.h"
#include "isonclust2_hip.h"

namespace {

long g_checks = 0;
bool g_ok = true;
int g_said = 0;
std::string g_shape;
#define EXPECT(cond)                                                                                         \
    do {                                                                                                     \
        ++g_checks;                                                                                          \
        if (!(cond)) {                                                                                       \
            if (++g_said <= 40) fprintf(stderr, "line %d (%s): %s\n", __LINE__, g_shape.c_str(), #cond);     \
            g_ok = false;                                                                                    \
        }                                                                                                    \
    } while (0)

struct Digest {  // FNV-1a over the values it is given, 8 bytes each
    uint64_t h = 1469598103934665603ull;
    void put(uint64_t v)
    {
        for (int x = 0; x < 8; ++x) h = (h ^ ((v >> (8 * x)) & 0xFFu)) * 1099511628211ull;
    }
    void put_i(int64_t v) { put(uint64_t(v)); }
};
bool g_all = false;

constexpr uint32_t NONE = 0xFFFFFFFFu, STRIP = 64u * FW_C;

// ---- the sweep's batches -------------------------------------------------------------------------------------------------

struct Scores {
    const char* name;
    AlnParams P;
};
const Scores SCORES[] = {{"2/-2/1", {2, -2, 1, 15, 1u << 17}}, {"1/-1/1", {1, -1, 1, 15, 1u << 17}}, {"0/-2/1", {0, -2, 1, 15, 1u << 17}}};

struct Corr {
    const char* name;
    bool corridor;  // (false: the every-tile route)
    AlnPlanOpts o;
};
std::vector<Corr> corridor_plans()
{
    std::vector<Corr> v;
    auto add = [&](const char* name, bool corridor, bool fixed, double frac, bool taper, uint32_t margin) {
        Corr c{name, corridor, AlnPlanOpts()};
        c.o.corridor_fixed = fixed;
        if (fixed) c.o.corridor_frac = frac;
        c.o.taper = taper;
        c.o.taper_margin = margin;
        v.push_back(c);
    };
    add("taper margin 256", true, false, 0, true, 256);
    add("taper margin 0", true, false, 0, true, 0);
    add("one width", true, false, 0, false, 256);
    add("fixed 0", true, true, 0.0, true, 256);
    add("fixed 0.2", true, true, 0.2, true, 256);
    add("fixed 1", true, true, 1.0, true, 256);
    add("every tile", false, false, 0, true, 256);
    return v;
}

struct Rate {
    float e;
    int go;
};
const Rate RATES[] = {{0.0f, 2}, {0.02f, 2}, {0.02f, 5}, {0.1f, 3}, {0.1f, 4}, {0.1f, -1}, {0.3f, 5}, {0.3f, 2}, {1.0f, 3}, {NAN, 4}};

const uint32_t LENGTHS[] = {1, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4600, 16700, 20480, 20481, 70000};

AlnPairDev pair_of(uint32_t n, uint32_t m, const Rate& r, uint32_t pad = 2)
{
    AlnPairDev d{};
    d.n = n;
    d.m = m;
    d.gap_open = r.go;
    d.e_sum = r.e;
    d.pad = pad;
    return d;
}

// per length: two equal pairs | the long query on a short reference, and its mirror image | the length with the next one; then the
// 16-bit strip's couple (`strip16`: its list has 65 536 tiles, so not in every batch), and a last couple of one pair
std::vector<AlnPairDev> batch_of(const Rate& r, bool strip16)
{
    std::vector<AlnPairDev> dp;
    const size_t nl = sizeof LENGTHS / sizeof LENGTHS[0];
    for (size_t x = 0; x < nl; ++x) {
        const uint32_t L = LENGTHS[x], S = std::max(1u, L / 3u), L2 = LENGTHS[(x + 1) % nl];
        dp.push_back(pair_of(L, L, r));
        dp.push_back(pair_of(L, L, r));
        dp.push_back(pair_of(L, S, r));
        dp.push_back(pair_of(S, L, r));
        dp.push_back(pair_of(L, L, r));
        dp.push_back(pair_of(L2, L2, r));
    }
    for (int x = 0; x < 2 && strip16; ++x) dp.push_back(pair_of(1, (1u << 26) - 2u, r));
    dp.push_back(pair_of(16700, 16650, r));
    return dp;
}

// the four classes' records: empty, or 200 related pairs per class on the line rho = match (1 - 1.9 e) with a little scatter,
// e in [0.05, 0.2] — 0.1 lies inside the range, 0.02 at its edge's slack, 0.3 outside
void fill_fit(CorridorFit (&fit)[4], bool fitted, const AlnParams& P)
{
    for (CorridorFit& f : fit) f = CorridorFit();
    if (!fitted) return;
    for (int g = 0; g < 4; ++g)
        for (int x = 0; x < 200; ++x) {
            const double e = 0.05 + 0.15 * double(x) / 199.0, rho = double(P.match) * (1.0 - 1.9 * e) + 0.01 * double((x * 7 + g) % 5 - 2);
            CorridorFit& f = fit[g];
            f.n += 1.0, f.se += e, f.sr += rho, f.see += e * e, f.ser += e * rho, f.srr += rho * rho;
            f.e_lo = std::min(f.e_lo, e), f.e_hi = std::max(f.e_hi, e);
        }
}

void couple_extent(const V2Couple& cp, const std::vector<AlnPairDev>& dp, uint32_t& nmax, uint32_t& mmax)
{
    nmax = mmax = 0;
    for (int h = 0; h < 2; ++h)
        if (cp.pid[h] != NONE) nmax = std::max(nmax, dp[cp.pid[h]].n), mmax = std::max(mmax, dp[cp.pid[h]].m);
}

// ---- the couples -------------------------------------------------------------------------------------------------------

void check_couple(const V2Plan& pl, uint32_t k2, const std::vector<AlnPairDev>& dp, const CorridorModel& cm, Digest& dg)
{
    const V2Couple& cp = pl.cps[k2];
    uint32_t nmax, mmax;
    couple_extent(cp, dp, nmax, mmax);
    const std::string base = g_shape;
    g_shape += ", couple " + std::to_string(k2) + " (" + std::to_string(nmax) + " x " + std::to_string(mmax) + ")";
    const uint32_t ncoarse = (nmax + CK2 - 1) / CK2;
    EXPECT(cp.pid[0] != NONE && cp.nstrips == (mmax + STRIP - 1) / STRIP);
    // bands
    EXPECT(cp.nbands >= 1 && cp.nbands <= uint32_t(V2_MAX_BANDS));
    EXPECT(cp.bstart[0] == 0 && cp.bstart[cp.nbands] == ncoarse);
    for (uint32_t b = 0; b < cp.nbands; ++b) EXPECT(cp.bstart[b] < cp.bstart[b + 1]);
    auto row0 = [&](uint32_t b) { return uint64_t(cp.bstart[b]) * CK2; };
    auto row1 = [&](uint32_t b) { return std::min<uint64_t>(nmax, uint64_t(cp.bstart[b + 1]) * CK2); };
    uint64_t skipped = 0;
    for (uint32_t b = 0; b < cp.nbands; ++b) {
        EXPECT(cp.plo[b] <= cp.phi[b] && cp.phi[b] < cp.nstrips);
        skipped += cp.plo[b] + (cp.nstrips - 1u - cp.phi[b]);
    }
    if (!cp.corridor) {
        for (uint32_t b = 0; b < cp.nbands; ++b) EXPECT(cp.plo[b] == 0 && cp.phi[b] == cp.nstrips - 1u);
        EXPECT(cp.probe_band == 0 && cp.probe_strip == 0);
    } else {
        EXPECT(cm.frac > 0.0 && cm.P.match > 0);  // (no corridor on the every-tile route, at fraction 0, or where a match scores nothing)
        for (uint32_t b = 0; b < cp.nbands; ++b) {
            if (b) EXPECT(cp.plo[b] >= cp.plo[b - 1] && cp.phi[b] >= cp.phi[b - 1]);
            // the strips of the band's diagonal cells (r0, r0) .. (r1, r1), as far as the grid has them
            const uint64_t r0 = row0(b), r1 = row1(b), s0 = (r0 ? r0 - 1u : 0u) / STRIP, s1 = std::min<uint64_t>((r1 - 1u) / STRIP, cp.nstrips - 1u);
            EXPECT(cp.plo[b] <= s0 && cp.phi[b] >= s1);
            // ... from which: of a computed tile off the border at most one of the tile above and the tile to its left is missing
            for (uint32_t p = std::max<uint32_t>(cp.plo[b], 1u); b && p <= cp.phi[b]; ++p)
                EXPECT(p - 1u >= cp.plo[b] || (p >= cp.plo[b - 1] && p <= cp.phi[b - 1]));
        }
        // the probe
        const uint32_t pb = cp.probe_band, ps = cp.probe_strip;
        EXPECT(pb + 1u < cp.nbands && ps < cp.nstrips);
        for (uint32_t b = 0; b <= pb && b < cp.nbands; ++b) EXPECT(cp.plo[b] == 0 && cp.phi[b] >= ps);
        const uint64_t R = row0(pb + 1u);
        for (int h = 0; h < 2; ++h)
            if (cp.pid[h] != NONE) EXPECT(dp[cp.pid[h]].n >= R && dp[cp.pid[h]].m > uint64_t(ps) * STRIP);
        EXPECT(skipped * 5u >= uint64_t(cp.nbands) * cp.nstrips);
    }
    // the bounds, restated: D = the least |row - column| over the cells (0-based) of the skipped tiles; the planner's Beff is
    // short of it by one, and a path through a skipped cell scores match x (max(n, m) - Beff - 1) at most
    int64_t D = INT64_MAX, first_col = -1, first_row = -1;  // ... the first skipped column of row 0, the first skipped row of column 0
    for (uint32_t b = 0; b < cp.nbands; ++b)
        for (uint32_t p = 0; p < cp.nstrips; ++p) {
            if (p >= cp.plo[b] && p <= cp.phi[b]) continue;
            const int64_t r0 = int64_t(row0(b)), r1 = int64_t(row1(b)), c0 = int64_t(p) * STRIP, c1 = std::min<int64_t>(mmax, c0 + STRIP);
            D = std::min(D, c1 <= r0 ? r0 - (c1 - 1) : r1 <= c0 ? c0 - (r1 - 1) : 0);
            if (b == 0 && (first_col < 0 || c0 < first_col)) first_col = c0;
            if (p == 0 && first_row < 0) first_row = r0;
        }
    for (int h = 0; h < 2; ++h) {
        if (cp.pid[h] == NONE) continue;
        const AlnPairDev& d = dp[cp.pid[h]];
        const V2PairEnd& e = pl.pend[cp.pid[h]];
        EXPECT(e.couple == k2 && e.nbands == cp.nbands && e.lrow0 == cp.lrow0[h] && e.best0 == cp.best0[h] && e.exit == INT32_MIN);
        if (!cp.corridor) {
            EXPECT(e.cert == INT32_MIN && e.start == INT32_MAX);
            continue;
        }
        EXPECT(D >= 2 && D < INT64_MAX);
        const int64_t len = std::max(d.n, d.m);
        EXPECT(e.cert == std::min<int64_t>(INT32_MAX, int64_t(cm.P.match) * std::max<int64_t>(0, len - (D - 1) - 1)));
        int64_t steps = -1;
        if (first_col >= 0 && first_col < int64_t(d.m)) steps = std::min<int64_t>(d.n, int64_t(d.m) - first_col);
        if (first_row >= 0 && first_row < int64_t(d.n)) steps = std::max(steps, std::min<int64_t>(int64_t(d.n) - first_row, d.m));
        const int64_t start = steps < 0 ? INT32_MIN : std::min<int64_t>(INT32_MAX, steps * cm.P.match);
        EXPECT(e.start == INT32_MAX || e.start == start);
        EXPECT(e.start == v2_start_bound(cp, d.n, d.m, cm.P.match) || e.start == INT32_MAX);
        if (!cm.taper || cm.fixed) EXPECT(e.start == INT32_MAX);
    }
    for (int h = 0; h < 2; ++h) dg.put(cp.pid[h]), dg.put(cp.lrow0[h]), dg.put(cp.best0[h]);
    dg.put(cp.nbands), dg.put(cp.nstrips), dg.put(cp.tpb), dg.put(cp.mpad), dg.put(cp.nq), dg.put(cp.corridor), dg.put(cp.probe_band), dg.put(cp.probe_strip),
        dg.put(cp.b0), dg.put(pl.cwords[k2]);
    for (uint32_t b = 0; b <= uint32_t(V2_MAX_BANDS); ++b) dg.put(cp.bstart[b]);
    for (uint32_t b = 0; b < uint32_t(V2_MAX_BANDS); ++b) dg.put(cp.plo[b]), dg.put(cp.phi[b]);
    g_shape = base;
}

void digest_pairs(const V2Plan& pl, Digest& dg)
{
    for (const V2PairEnd& e : pl.pend) dg.put(e.lrow0), dg.put(e.best0), dg.put(e.nbands), dg.put(e.couple), dg.put_i(e.cert), dg.put_i(e.start), dg.put_i(e.exit);
    dg.put(pl.lrow_total), dg.put(pl.best_total), dg.put(pl.max_strips), dg.put(pl.tiles_skipped), dg.put(pl.tiles_all);
}

// ---- slices and tile lists ---------------------------------------------------------------------------------------------

struct Span {
    uint64_t lo, hi;
};
bool disjoint(std::vector<Span>& v)
{
    std::sort(v.begin(), v.end(), [](const Span& a, const Span& b) { return a.lo < b.lo; });
    for (size_t x = 1; x < v.size(); ++x)
        if (v[x].lo < v[x - 1].hi) return false;
    return true;
}

// `pl`: the couples as plan_couples left them (a copy: slicing places the regions)
void check_slices(V2Plan pl, const std::vector<AlnPairDev>& dp, uint64_t budget, const std::vector<uint64_t>& cops, bool lists, Digest& dg)
{
    const std::string base = g_shape;
    const V2Plan before = pl;
    slice_couples(pl, budget, cops);
    uint32_t next = 0;
    uint64_t most_words = 0, most_prof = 0;
    for (size_t si = 0; si < pl.slices.size(); ++si) {
        g_shape = base + ", slice " + std::to_string(si);
        const uint32_t k_lo = pl.slices[si].first, cnt = pl.slices[si].second;
        EXPECT(k_lo == next && cnt >= 1 && k_lo + cnt <= pl.ncouples);
        next = k_lo + cnt;
        uint64_t words = 0, prof = 0, ops = 0;
        std::vector<Span> regions, profs;
        for (uint32_t k2 = k_lo; k2 < k_lo + cnt && k2 < pl.ncouples; ++k2) {
            const V2Couple& cp = pl.cps[k2];
            uint32_t nmax, mmax;
            couple_extent(cp, dp, nmax, mmax);
            const uint64_t ncr = (nmax - 1u) / CK2, ncc = (mmax - 1u) / CK2;
            const uint64_t size[4] = {ncr * 2u * cp.mpad, ncr * (cp.mpad / 16u) * 2u, ncc * uint64_t(cp.nq) * 8u, ncc * uint64_t(cp.nq) * 2u};
            const uint64_t at[4] = {cp.rdat, cp.rbase, cp.cdat, cp.cbase}, was[4] = {before.cps[k2].rdat, before.cps[k2].rbase, before.cps[k2].cdat, before.cps[k2].cbase};
            EXPECT(cp.mpad % 16u == 0 && cp.mpad >= mmax && cp.mpad < mmax + 16u && cp.nq == (nmax + 3u) / 4u);
            for (int x = 0; x < 4; ++x) {
                EXPECT(at[x] % 4u == 0 && at[x] == words + was[x] && at[x] + size[x] <= words + pl.cwords[k2]);
                if (size[x]) regions.push_back(Span{at[x], at[x] + size[x]});
            }
            const uint64_t prof_k = uint64_t(cp.nstrips) * 2u * 5u * 64u;
            EXPECT(cp.prof == prof);
            profs.push_back(Span{cp.prof, cp.prof + prof_k});
            for (int h = 0; h < 2; ++h) {
                if (cp.pid[h] == NONE) continue;
                const V2PairCk& c = pl.pck[cp.pid[h]];
                EXPECT(c.rdat == cp.rdat && c.rbase == cp.rbase && c.cdat == cp.cdat && c.cbase == cp.cbase && c.mpad == cp.mpad && c.nq == cp.nq &&
                       c.half == uint32_t(h) && c.couple == k2);
            }
            words += pl.cwords[k2], prof += prof_k, ops += cops.empty() ? 0u : cops[k2];
        }
        EXPECT(disjoint(regions) && disjoint(profs));
        if (cnt > 1) EXPECT(words * 4u + prof * 16u + ops <= budget);
        if (next < pl.ncouples)  // (the slice ended because the next couple did not fit)
            EXPECT((words + pl.cwords[next]) * 4u + (prof + uint64_t(pl.cps[next].nstrips) * 640u) * 16u + ops + (cops.empty() ? 0u : cops[next]) > budget);
        most_words = std::max(most_words, words), most_prof = std::max(most_prof, prof);
        dg.put(k_lo), dg.put(cnt);
    }
    g_shape = base;
    EXPECT(next == pl.ncouples && pl.arena_words == most_words && pl.prof_total == most_prof);

    // the tile lists: the closed forms, then the lists themselves (`lists` false: the same slices have been through it)
    tile_counts(pl);
    const std::string differs = lists ? tile_lists_check(pl) : std::string("not made");
    EXPECT(differs.empty() || !lists);
    if (lists && !differs.empty() && g_said <= 40) fprintf(stderr, "  (%s) %s\n", g_shape.c_str(), differs.c_str());
    uint32_t max_items = 0, max_flags = 0, max_pairs = 0;
    for (size_t si = 0; si < pl.slices.size() && differs.empty(); ++si) {
        g_shape = base + ", slice " + std::to_string(si);
        const uint32_t k_lo = pl.slices[si].first, k_hi = k_lo + pl.slices[si].second;
        const std::vector<V2Item>& it = pl.items[si];
        uint32_t nf = 0, diag = 1;
        uint64_t n_probe = 0;
        for (uint32_t k2 = k_lo; k2 < k_hi; ++k2) {
            const V2Couple& cp = pl.cps[k2];
            EXPECT(cp.flag0 == nf);
            nf += cp.nbands * cp.nstrips;
            if (cp.corridor) n_probe += (uint64_t(cp.probe_band) + 1u) * (uint64_t(cp.probe_strip) + 1u);
            diag = std::max(diag, cp.nbands + cp.nstrips - 1u);
        }
        EXPECT(pl.n_probe[si] == n_probe && pl.n_items[si] == n_probe + nf && it.size() == pl.n_items[si] && pl.n_diag[si] == diag);
        // where a tile stands in the probe's part and in the main part (0: nowhere yet)
        std::vector<uint32_t> at_probe(nf, 0), at_main(nf, 0);
        bool good = it.size() == n_probe + nf;
        for (size_t x = 0; x < it.size() && good; ++x) {
            const V2Item& t = it[x];
            good = t.couple >= k_lo && t.couple < k_hi && t.band < pl.cps[t.couple].nbands && t.strip < pl.cps[t.couple].nstrips;
            if (!good) break;
            const V2Couple& cp = pl.cps[t.couple];
            const bool probe = x < n_probe;
            if (probe) good = cp.corridor && t.band <= cp.probe_band && t.strip <= cp.probe_strip;
            std::vector<uint32_t>& at = probe ? at_probe : at_main;
            const uint32_t f = cp.flag0 + t.band * cp.nstrips + t.strip;
            good = good && at[f] == 0;  // (exactly once)
            // after the tile above it and the tile to its left
            if (good && t.band) good = at[f - cp.nstrips] != 0;
            if (good && t.strip) good = at[f - 1u] != 0;
            at[f] = uint32_t(x) + 1u;
        }
        EXPECT(good);
        for (uint32_t f = 0; f < nf && good; ++f) good = at_main[f] != 0;  // (every tile of every couple)
        EXPECT(good);
        max_items = std::max(max_items, pl.n_items[si]), max_flags = std::max(max_flags, nf);
        max_pairs = std::max(max_pairs, std::min(pl.cnt, 2u * k_hi) - 2u * k_lo);
        dg.put(pl.n_items[si]), dg.put(pl.n_probe[si]), dg.put(pl.n_diag[si]);
    }
    g_shape = base;
    if (lists && differs.empty()) EXPECT(pl.max_items == max_items && pl.max_flags == max_flags && pl.max_pairs == max_pairs);
    for (const V2Couple& cp : pl.cps) dg.put(cp.rdat), dg.put(cp.rbase), dg.put(cp.cdat), dg.put(cp.cbase), dg.put(cp.prof), dg.put(cp.flag0);
    for (const V2PairCk& c : pl.pck) dg.put(c.rdat), dg.put(c.rbase), dg.put(c.cdat), dg.put(c.cbase), dg.put(c.mpad), dg.put(c.nq), dg.put(c.half), dg.put(c.couple);
    dg.put(pl.arena_words), dg.put(pl.prof_total), dg.put(pl.max_items), dg.put(pl.max_flags), dg.put(pl.max_pairs);
}

void sweep_v2()
{
    const std::vector<Corr> plans = corridor_plans();
    int group = 0;
    for (const Scores& sc : SCORES)
        for (const Corr& co : plans)
            for (int fitted = 0; fitted < 2; ++fitted) {
                CorridorFit fit[4];
                fill_fit(fit, fitted != 0, sc.P);
                const CorridorModel cm = corridor_model(sc.P, co.corridor, co.o, fit, true);
                Digest group_dg;
                int nth = 0;
                uint64_t with_corridor = 0, tapered = 0;
                for (uint32_t want_bands : {12u, 17u, 40u, 64u})  // (64: beyond what band_target asks for — the only way to more than V2_MAX_BANDS heights)
                    for (const Rate& r : RATES) {
                        const std::vector<AlnPairDev> dp = batch_of(r, &r == &RATES[0] || &r == &RATES[3]);
                        std::vector<uint32_t> order(dp.size());
                        for (size_t x = 0; x < order.size(); ++x) order[x] = uint32_t(x);
                        g_shape = std::string("scores ") + sc.name + ", " + co.name + (fitted ? ", fitted" : ", no fit") + ", band target " + std::to_string(want_bands) +
                                  ", e " + std::to_string(r.e) + ", gap open " + std::to_string(r.go);
                        Digest dg;
                        V2Plan pl;
                        pl.cnt = pl.np = uint32_t(dp.size());
                        pl.ncouples = (pl.cnt + 1u) / 2u;
                        plan_couples(pl, dp, order.data(), cm, want_bands);
                        EXPECT(pl.cps.size() == pl.ncouples && pl.cps.back().pid[1] == NONE);
                        uint64_t skipped = 0, all = 0;
                        for (uint32_t k2 = 0; k2 < pl.ncouples; ++k2) {
                            check_couple(pl, k2, dp, cm, dg);
                            const V2Couple& cp = pl.cps[k2];
                            all += uint64_t(cp.nbands) * cp.nstrips;
                            for (uint32_t b = 0; b < cp.nbands && cp.corridor; ++b) skipped += cp.plo[b] + (cp.nstrips - 1u - cp.phi[b]);
                            with_corridor += cp.corridor;
                            tapered += cp.corridor && pl.pend[cp.pid[0]].start != INT32_MAX;
                        }
                        EXPECT(pl.tiles_skipped == skipped && pl.tiles_all == all);
                        digest_pairs(pl, dg);
                        std::vector<uint64_t> cops(pl.ncouples, 0);
                        for (uint32_t x = 0; x < pl.cnt; ++x) cops[x / 2u] += uint64_t(dp[x].n) + dp[x].m;
                        for (uint64_t budget : {uint64_t(0), ~uint64_t(0) >> 1}) {  // every couple its own slice | one slice
                            check_slices(pl, dp, budget, {}, true, dg);
                            check_slices(pl, dp, budget, cops, false, dg);
                        }
                        if (g_all) printf("plan %d.%d (%s): %016llx\n", group, nth, g_shape.c_str(), (unsigned long long)dg.h);
                        group_dg.put(dg.h);
                        ++nth;
                    }
                // (what the sweep must reach: corridors where one may be planned, tapered ones where the model plans them)
                g_shape = std::string("scores ") + sc.name + ", " + co.name;
                const bool may = co.corridor && sc.P.match > 0 && !(co.o.corridor_fixed && (co.o.corridor_frac == 0.0 || co.o.corridor_frac == 1.0));  // (1: nothing skipped)
                EXPECT((with_corridor > 0) == may);
                EXPECT((tapered > 0) == (may && co.o.taper && !co.o.corridor_fixed));
                printf("v2 plans %2d  scores %-7s %-17s %-7s %3d plans, %5llu couples with a corridor (%llu tapered): %016llx\n", group, sc.name, co.name,
                       fitted ? "fitted" : "no fit", nth, (unsigned long long)with_corridor, (unsigned long long)tapered, (unsigned long long)group_dg.h);
                ++group;
            }
    Digest dg;
    g_shape = "band_target";
    for (uint32_t ncouples : {1u, 31u, 128u, 129u, 811u, 100000u})
        for (uint32_t few : {0u, 128u})
            for (int occ : {2, 3}) {
                const uint32_t want = band_target(ncouples, few, occ, 256);
                EXPECT(want >= 12u && want <= uint32_t(V2_MAX_BANDS) && (!(few && ncouples <= few) || want <= 17u));
                dg.put(want);
            }
    printf("band_target: %016llx\n", (unsigned long long)dg.h);
}

// ---- version 1 ----------------------------------------------------------------------------------------------------------

void sweep_v1()
{
    Digest dg;
    const Rate r{0.1f, 3};
    // the lengths above, with the kernel families in runs: version 2's pairs in front (n_v2), then profile and comparing pairs
    std::vector<AlnPairDev> dp;
    for (uint32_t L : LENGTHS) {
        dp.push_back(pair_of(L, L, r, 2));
        dp.push_back(pair_of(L, std::max(1u, L / 3u), r, 1));
        dp.push_back(pair_of(std::max(1u, L / 3u), L, r, 1));
        dp.push_back(pair_of(L, L, r, 0));
    }
    const uint32_t np = uint32_t(dp.size());
    std::vector<uint32_t> order;
    for (uint32_t want : {2u, 1u, 0u})
        for (uint32_t x = 0; x < np; ++x)
            if (dp[x].pad == want) order.push_back(x);
    uint32_t n2 = 0;
    while (n2 < np && dp[order[n2]].pad == 2u) ++n2;
    for (uint32_t n_v2 : {0u, n2, np})
        for (uint64_t budget : {uint64_t(0), ~uint64_t(0) >> 1})
            for (int emit = 0; emit < 2; ++emit) {
                g_shape = "version 1, n_v2 " + std::to_string(n_v2) + ", budget " + (budget ? "all" : "0") + (emit ? ", emitting" : "");
                const V1Plan pl = plan_v1(dp, order.data(), n_v2, budget, emit != 0);
                EXPECT(pl.cko.size() == np && pl.ops_end.size() == (emit ? np : 0u) && pl.slice_ops.size() == pl.slices.size());
                uint32_t next = n_v2, max_cnt = 0;
                uint64_t arena = 0, ops_most = 0;
                for (size_t si = 0; si < pl.slices.size(); ++si) {
                    const uint32_t first = pl.slices[si].first, cnt = pl.slices[si].second;
                    EXPECT(first == next && cnt >= 1 && first + cnt <= np);
                    next = first + cnt;
                    std::vector<Span> regions;
                    uint64_t used = 0, ops = 0;
                    for (uint32_t x = first; x < first + cnt && x < np; ++x) {
                        const AlnPairDev& d = dp[order[x]];
                        const AlnCk& ck = pl.cko[order[x]];
                        EXPECT((d.pad != 0) == (dp[order[first]].pad != 0));  // one kernel family
                        const uint64_t rows = uint64_t((d.n - 1) / TILE) * row_pitch(d.m), cols = uint64_t((d.m - 1) / TILE) * col_pitch(d.n);
                        EXPECT(row_pitch(d.m) % 16u == 0 && row_pitch(d.m) >= d.m && col_pitch(d.n) % 4u == 0 && col_pitch(d.n) >= d.n && rows == v1_row_units(d));
                        // (16 int2 is the row PITCH; a pair's columns — multiples of 4 — lie between two pairs' rows, so an offset is a
                        // multiple of 4 int2: twice the 16 bytes the kernels' int4 stores need)
                        EXPECT(ck.row_off % 4u == 0 && ck.col_off % 4u == 0 && ck.row_off == used && ck.col_off == ck.row_off + rows);
                        if (rows) regions.push_back(Span{ck.row_off, ck.row_off + rows});
                        if (cols) regions.push_back(Span{ck.col_off, ck.col_off + cols});
                        used += rows + cols;
                        if (emit) {
                            EXPECT(pl.ops_end[order[x]] == ops + d.n + d.m);  // ascending, a region of n + m bytes each
                            ops += uint64_t(d.n) + d.m;
                        }
                        dg.put(ck.row_off), dg.put(ck.col_off), dg.put(emit ? pl.ops_end[order[x]] : 0u);
                    }
                    EXPECT(disjoint(regions) && pl.slice_ops[si] == ops);
                    if (cnt > 1) EXPECT(used * 8u + ops <= budget);
                    arena = std::max(arena, used), ops_most = std::max(ops_most, ops), max_cnt = std::max(max_cnt, cnt);
                    dg.put(first), dg.put(cnt), dg.put(pl.slice_ops[si]);
                }
                EXPECT(next == np && pl.arena == arena && pl.ops_most == ops_most && pl.max_cnt == max_cnt);
                dg.put(pl.arena), dg.put(pl.ops_most), dg.put(pl.max_cnt);
            }
    printf("version 1 plans: %016llx\n", (unsigned long long)dg.h);

    Digest dw;
    for (uint32_t max_n : LENGTHS)
        for (uint32_t max_m : LENGTHS)
            for (uint32_t pairs : {1u, 64u, 65u, 512u, 513u, 5000u})
                for (int carry = 0; carry < 2; ++carry)
                    for (int forced = 0; forced <= 9; ++forced)  // (0: no switch; 9: a switch out of range)
                        for (int nct = 0; nct < 2; ++nct) {
                            AlnPlanOpts o;
                            o.waves_set = forced != 0;
                            o.waves = forced;
                            o.no_cross_tail = nct != 0;
                            const WavePlan wp = plan_waves(max_n, max_m, pairs, carry != 0, o);
                            g_shape = "plan_waves " + std::to_string(max_n) + " x " + std::to_string(max_m) + ", " + std::to_string(pairs) + " pairs" + (carry ? ", carry" : "") +
                                      ", forced " + std::to_string(forced) + (nct ? ", no cross tail" : "");
                            const uint32_t w = wp.waves;
                            EXPECT(w >= 1 && w <= uint32_t(ALN_MAXW));
                            if (forced) {
                                EXPECT(w == (forced <= ALN_MAXW ? uint32_t(forced) : uint32_t(ALN_MAXW)) && !wp.few_pairs);
                            } else {
                                EXPECT((w & (w - 1u)) == 0);
                                const uint32_t strips = (max_m + STRIP - 1) / STRIP, tiles = (max_n + TILE - 1) / TILE;
                                // the rule: whole pairs' waves within 4096, and (traced) two strips and two tiles per band, (carry) a strip no wider than the reference
                                const bool meets = uint64_t(pairs) * w <= 4096 && (carry ? uint64_t(w / 2) * 64 * ALN_C < max_m : strips >= 2 * w && tiles >= 2 * w);
                                EXPECT(w == 1 || meets || (wp.few_pairs && w == 4));
                                EXPECT(!wp.few_pairs || (w == 4 && !carry && !nct && pairs <= 64));
                            }
                            dw.put(w), dw.put(wp.few_pairs);
                        }
    printf("plan_waves: %016llx\n", (unsigned long long)dw.h);
}

// ---- the real plan against the certificate -----------------------------------------------------------------------------

struct Rng {  // (a generator of its own: the same sequences wherever this is built)
    uint64_t s;
    uint32_t next()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return uint32_t(s >> 33);
    }
    double unit() { return double(next()) / 2147483648.0; }
    char base() { return "ACGT"[next() & 3u]; }
};

std::string random_seq(Rng& g, size_t len)
{
    std::string s(len, 'A');
    for (char& ch : s) ch = g.base();
    return s;
}

std::string mutate(Rng& g, const std::string& s, double e)  // a third each: substitution, deletion, insertion
{
    std::string out;
    for (char ch : s) {
        const double x = g.unit();
        if (x < e / 3) out.push_back(g.base());
        else if (x < 2 * e / 3) continue;
        else if (x < e) out.push_back(ch), out.push_back(g.base());
        else out.push_back(ch);
    }
    return out;
}

void check_certificate()
{
    Rng g{20260};
    const AlnParams P = SCORES[0].P;
    struct Case {
        std::string q, r;
        double e;
        bool related;
    };
    std::vector<Case> cases;
    const double rates[] = {0.06, 0.12, 0.16, 0.20, 0.24};  // summed error rates: reads at 3 to 12 % each
    const size_t lens[] = {9000, 8200, 7400, 6600, 5800};
    for (int x = 0; x < 5; ++x) {
        const std::string t = random_seq(g, lens[x]);
        cases.push_back(Case{mutate(g, t, rates[x] / 2), mutate(g, t, rates[x] / 2), rates[x], true});
    }
    for (int x = 0; x < 2; ++x) cases.push_back(Case{random_seq(g, 5200 + 900 * x), random_seq(g, 5000 + 1100 * x), 0.2, false});
    std::vector<AlnPairDev> dp;
    for (const Case& c : cases) {
        AlnPairDev d{};
        d.n = uint32_t(c.q.size()), d.m = uint32_t(c.r.size());
        d.gap_open = ioc_host_gap_open(c.e);
        d.e_sum = float(c.e);
        dp.push_back(d);
    }
    // couples: 0 + 1, 2 + 3, 4 alone | the unrelated pairs together — as order_pairs puts hinted wrong candidates behind the others
    const std::vector<uint32_t> order{0, 1, 2, 3, 5, 6, 4};
    // the full matrix once per pair
    std::vector<std::string> full(cases.size());
    std::vector<int32_t> fscore(cases.size()), fi(cases.size()), fj(cases.size());
    for (size_t x = 0; x < cases.size(); ++x) {
        const Case& c = cases[x];
        std::vector<char> ops(c.q.size() + c.r.size() + 1);
        const int len = ioc_host_align_ops(c.q.data(), int32_t(c.q.size()), c.r.data(), int32_t(c.r.size()), P.match, P.mismatch, dp[x].gap_open, P.gap_extend, ops.data(),
                                           int32_t(ops.size()), &fscore[x]);
        g_shape = "certificate, pair " + std::to_string(x);
        EXPECT(len > 0);
        full[x].assign(ops.data(), size_t(std::max(len, 0)));
        size_t td = 0, ti = 0;  // the end cell: what the trailing end gaps leave of either sequence
        while (td < full[x].size() && full[x][full[x].size() - 1 - td] == 'd') ++td;
        while (td + ti < full[x].size() && full[x][full[x].size() - 1 - td - ti] == 'i') ++ti;
        fi[x] = int32_t(c.q.size() - ti), fj[x] = int32_t(c.r.size() - td);
    }
    CorridorFit fit[4];
    fill_fit(fit, false, P);
    for (int taper = 1; taper >= 0; --taper) {
        AlnPlanOpts o;
        o.taper = taper != 0;
        const CorridorModel cm = corridor_model(P, true, o, fit, true);
        V2Plan pl;
        pl.cnt = pl.np = uint32_t(dp.size());
        pl.ncouples = (pl.cnt + 1u) / 2u;
        plan_couples(pl, dp, order.data(), cm, 17);
        uint32_t certified_related = 0;
        for (size_t x = 0; x < cases.size(); ++x) {
            const Case& c = cases[x];
            const V2PairEnd& e = pl.pend[x];
            const V2Couple& cp = pl.cps[e.couple];
            g_shape = std::string("certificate, ") + (taper ? "taper" : "one width") + ", pair " + std::to_string(x) + " (" + std::to_string(dp[x].n) + " x " +
                      std::to_string(dp[x].m) + ", e " + std::to_string(c.e) + ")";
            uint32_t nmax, mmax;
            couple_extent(cp, dp, nmax, mmax);
            int32_t rows[V2_MAX_BANDS], lo[V2_MAX_BANDS], hi[V2_MAX_BANDS], out[8];
            for (uint32_t b = 0; b < cp.nbands; ++b) {
                rows[b] = int32_t(uint32_t(cp.bstart[b + 1u]) - uint32_t(cp.bstart[b])) * CK2;
                lo[b] = cp.plo[b];
                hi[b] = cp.phi[b];
            }
            std::vector<char> ops(c.q.size() + c.r.size() + 1);
            const int len = ioc_host_align_corridor(c.q.data(), int32_t(c.q.size()), c.r.data(), int32_t(c.r.size()), P.match, P.mismatch, dp[x].gap_open, P.gap_extend, rows,
                                                    int32_t(cp.nbands), int32_t(STRIP), lo, hi, ops.data(), int32_t(ops.size()), out);
            EXPECT(len > 0 && out[0] <= fscore[x]);
            if (len <= 0) continue;
            if (!cp.corridor) {  // nothing skipped: the alignment itself, no bound
                EXPECT(out[6] == 0 && out[0] == fscore[x] && out[1] == fi[x] && out[2] == fj[x] && full[x] == std::string(ops.data(), size_t(len)));
                continue;
            }
            // the planner's bounds are the host aligner's (the parent bound is planned with the couple's larger rows and columns)
            const bool largest = dp[x].n == nmax && dp[x].m == mmax, own = e.start != INT32_MAX;
            EXPECT(largest ? e.cert == out[3] : e.cert >= out[3]);
            EXPECT((own ? taper != 0 : true) && (!own || e.start == out[4]));
            const int32_t bound = own ? std::min(e.cert, std::max(e.start, out[5])) : e.cert;
            const bool certified = out[0] > bound;
            if (certified) {
                EXPECT(out[0] > std::min(out[3], std::max(out[4], out[5])) || !largest);
                EXPECT(out[0] == fscore[x] && out[1] == fi[x] && out[2] == fj[x] && full[x] == std::string(ops.data(), size_t(len)));
                certified_related += c.related;
            }
            EXPECT(c.related || !certified);  // (an unrelated pair scores next to nothing: no bound lets it pass)
            printf("certificate, %-9s pair %zu %5u x %5u e %.2f %s: %u bands x %u strips, %d of %d tiles skipped, score %d (full %d), bounds %d / %d / %d: %s\n",
                   taper ? "taper" : "one width", x, dp[x].n, dp[x].m, c.e, c.related ? "related  " : "unrelated", cp.nbands, cp.nstrips, out[6], out[7], out[0], fscore[x],
                   e.cert, own ? e.start : out[4], out[5], certified ? "certified" : "not certified");
        }
        g_shape = std::string("certificate, ") + (taper ? "taper" : "one width");
        EXPECT(certified_related >= 1);
    }
}

}  // namespace

int main(int argc, char** argv)
{
    g_all = argc > 1 && strcmp(argv[1], "--all") == 0;
    static_assert(STRIP % CK2 == 0 && CK2 % TILE == 0, "a strip's edge is a coarse column, a coarse row a tile's edge");
    sweep_v2();
    sweep_v1();
    check_certificate();
    if (!g_ok) {
        fprintf(stderr, "FAILED (%ld checks)\n", g_checks);
        return 1;
    }
    printf("ok: %ld checks of the aligner's plans\n", g_checks);
    return 0;
}
