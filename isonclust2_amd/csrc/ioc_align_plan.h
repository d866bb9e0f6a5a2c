// ioc_align_plan.h — what the batched aligner (ioc_align_gpu.hip) decides on the host before it launches anything: the records the
// host and the kernels share, the constants the plan is written in, and the planner — bands, corridors, checkpoint words, couples,
// slices, the tile list's closed forms and its defining order, version 1's waves and arena.  Pure arithmetic over pair lengths,
// error rates, scores and the switches of AlnPlanOpts: no HIP header, no environment, no context.  tools/align_plan_check.cpp
// drives it on the CPU, under the sanitizers, and holds every plan against the conditions the kernels rely on.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define IOC_PLAN_HD __host__ __device__ inline __attribute__((always_inline))  // (__forceinline__, also where no HIP header came first)
#else
#define IOC_PLAN_HD inline
#endif

// The switches that shape a plan.  ioc_align_gpu.hip fills one from the environment per call of align_pairs, never across calls
// (plan_opts there: the clamps are applied where the record is filled).
struct AlnPlanOpts {
    bool corridor_fixed = false;   // IOC_ALIGN_CORRIDOR: one fraction for every couple ...
    double corridor_frac = 0.2;    // ... this one, in [0, 1]; the fraction without a model otherwise
    bool taper = true;             // IOC_ALIGN_CORRIDOR_TAPER
    uint32_t taper_margin = 256u;  // IOC_ALIGN_CORRIDOR_MARGIN, in [0, 2^20]
    bool no_fit = false;           // IOC_ALIGN_CORRIDOR_NO_FIT
    uint32_t few_limit = 128;      // IOC_ALIGN_V2_FEW
    bool waves_set = false;        // IOC_ALIGN_WAVES is there ...
    int waves = 0;                 // ... and says this
    bool no_cross_tail = false;    // IOC_ALIGN_NO_CROSS_TAIL
};

constexpr int ALN_C = 8;             // columns per thread
constexpr int ALN_MAXW = 8;          // waves per workgroup

struct AlnPairDev {
    uint32_t q_off, n;   // query (rows)
    uint32_t r_off, m;   // reference (columns)
    int32_t gap_open, ilimit;
    uint32_t rc;         // reference is read reverse-complemented
    uint32_t pad;
    // verdict mode (ioc_align_set_verdict_threshold): the traceback may stop once the count of good windows has reached stop_at
    // (the ratio is >= the threshold whatever follows) or can no longer reach it; 0 = walk to the end
    uint32_t stop_at;
    float e_sum;         // (host side only) the pair's summed error rate e1 + e2 (ioc_aln_pair::e): what the corridor is planned from
};

struct AlnParams {
    int32_t match, mismatch, gap_extend;
    uint32_t k;     // window length, 1..32
    uint32_t mbit;  // 1 << (32 - k): where a new comparison bit enters the (top-aligned) window
};

constexpr int FW_C = 16;      // columns per thread in the forward pass
#ifndef IOC_ALIGN_TILE
#define IOC_ALIGN_TILE 128
#endif
constexpr int TILE = IOC_ALIGN_TILE;  // checkpoint pitch = traceback tile edge (128 or 256)
static_assert(TILE == 128 || TILE == 256, "tile edge");

struct AlnCk {  // where a pair's checkpoints live in the arena, in int2 units
    uint64_t row_off;  // [(n - 1) / TILE][2][row_pitch(m)] ints: the Hq plane, then the F* plane, of rows TILE, 2 TILE, ...
    uint64_t col_off;  // [(m - 1) / TILE][col_pitch(n)]  (H, E) of columns TILE, 2 TILE, ...
};

// row checkpoints are padded to whole lane blocks (16 columns): a lane stores its block without per-column
// bounds checks — the store block runs in EVERY step of a wave (for the two lanes whose skewed row block ends a
// tile), so its instruction count matters as much as the cells'
IOC_PLAN_HD uint64_t row_pitch(uint32_t m) { return (uint64_t(m) + 15u) & ~uint64_t(15); }
// column checkpoints: 4 rows (one step of a lane) go out as two 16-byte stores
IOC_PLAN_HD uint64_t col_pitch(uint32_t n) { return (uint64_t(n) + 3u) & ~uint64_t(3); }

// ---- version 2 (ioc_align_v2.inc) ---------------------------------------------------------------------------------------

constexpr int CK2 = 512;          // coarse checkpoint pitch (rows and columns); a multiple of TILE
constexpr int V2_WAVES = 4;       // waves per workgroup: independent workers with LDS of their own
constexpr int V2_MAX_BANDS = 40;  // bands per couple (a 16.7 kb pair has 33 coarse rows: a band each when few couples share the chip)
static_assert(CK2 % TILE == 0, "block geometry");

struct V2Couple {
    uint32_t pid[2];          // the two pairs (0xFFFFFFFF: none)
    uint32_t nbands, nstrips; // tile grid of the couple (the larger of the two pairs)
    uint32_t tpb;             // (unused: bands have their own heights, see bstart)
    uint32_t flag0;           // flags[flag0 + band * nstrips + strip]
    uint32_t mpad;            // row-checkpoint pitch in words (multiple of 16)
    uint32_t nq;              // entries per checkpoint column: ceil(max n / 4)
    uint64_t rdat;            // [coarse row][plane Hq, F*][mpad] words                      (word offsets into the arena)
    uint64_t rbase;           // [coarse row][mpad / 16] int2: the two bases of a lane block
    uint64_t cdat;            // [coarse column][nq][8] words: hl[0..3], el[0..3] of a 4-row step
    uint64_t cbase;           // [coarse column][nq] int2
    uint64_t prof;            // query profiles of the couple's strips: [strip][pair][base code][lane] uint4 (uint4 index into the profile arena)
    uint32_t lrow0[2];        // per pair: first entry of its last-row bests [strip][lane] (int2)
    uint32_t best0[2];        // per pair: first entry of its per-band bests of the last column (int2)
    // band b covers the coarse rows [bstart[b], bstart[b + 1]).  (Heights may differ: short bands at the top and the bottom
    // of the matrix were tried as a way to shorten the ramp of the tile grid, and measured slower.)
    uint16_t bstart[V2_MAX_BANDS + 1];
    // THE CORRIDOR: only the tiles (band b, strips plo[b] .. phi[b]) are computed — those that meet |row - column| <= B —, the
    // others count as "no score".  What comes out is the alignment restricted to paths inside the computed tiles; it IS the
    // alignment (score, end cell, every choice along the traceback) whenever its score beats the most a path through a skipped
    // cell can reach, match x (max(n, m) - Beff - 1) with Beff the least |row - column| of a skipped cell: k_fwd2_ends checks
    // that per pair (V2PairEnd::cert) and the host runs a pair that fails it again without a corridor.  Pairs of one transcript
    // pass (their score is 1.6 - 1.8 per base where match = 2: B = 0.2 x length), wrong candidates do not.
    // Whether a pair is worth a corridor is not known beforehand: a PROBE launch computes the top left corner of every couple's
    // grid (bands 0 .. probe_band — 2048 rows —, strips 0 .. probe_strip: exact values, nothing is missing there), k_fwd2_probe reads the diagonal's
    // neighbourhood out of the coarse row at the probe band's end — a pair of one transcript has ~1.7 per base there, a wrong
    // candidate next to nothing — and opens the couple's grid (corridor = 0, every strip) if either pair looks wrong; the main
    // launch takes the full list of tiles and skips what is outside its couple's corridor or done already.
    uint16_t plo[V2_MAX_BANDS], phi[V2_MAX_BANDS];
    uint32_t corridor;        // some tile of the grid is skipped
    uint16_t probe_band, probe_strip;
    uint32_t b0;              // the half width the host planned the corridor with (columns)
};

struct V2Item {
    uint32_t couple;
    uint16_t band, strip;
};

// where a pair's checkpoints are: what the traceback needs of its couple
struct V2PairCk {
    uint64_t rdat, rbase, cdat, cbase;
    uint32_t mpad, nq, half, couple;
};

// end cell of every pair: best of the last column (rows ascending: bands top to bottom), replaced only by a strictly larger
// cell of the last row (columns ascending) — the host aligner's scan order (ioc_align.cpp).  One wave per pair.
struct V2PairEnd {
    uint32_t lrow0, best0, nbands, couple;
    int32_t cert;  // corridor: the score the pair has to BEAT for the corridor's result to stand (INT32_MIN: no corridor)
    // A TAPERED corridor (plan_corridor) is vouched for by the exit cells' scores instead: `cert` is then the parent bound, and
    // the pair has to beat min(cert, max(start, exit)).  A path through a skipped cell either has its first cell off row 0 and
    // column 0 skipped — `start`: match x the diagonal steps left from the first such cell of row 0 and of column 0
    // (v2_start_bound; INT32_MAX: one width for every band, `cert` alone decides) — or steps into its first skipped cell from a
    // computed cell y, its prefix inside the computed tiles: it scores H_C(y) + match x min(n - i_y, m - j_y) at most, H_C being
    // what the pass has just stored at y.  `exit`: the largest of these over the pair's exit cells (k_fwd2_cert; INT32_MIN: none).
    int32_t start, exit;
};

// the start bound of a pair (n rows, m columns) in its couple's corridor, whose band 0 starts at strip 0: row 0 is left for a skipped
// tile from column (phi[0] + 1) strips on, column 0 from the first row of the first band with plo > 0 on
IOC_PLAN_HD int32_t v2_start_bound(const V2Couple& cp, uint32_t n, uint32_t m, int32_t match)
{
    const unsigned long long strip_cols = 64ull * FW_C, j0 = (uint32_t(cp.phi[0]) + 1ull) * strip_cols;
    long long steps = -1;
    if (j0 < m) steps = (long long)(n < m - j0 ? n : m - j0);
    for (uint32_t b = 0; b < cp.nbands; ++b)
        if (cp.plo[b] > 0) {
            const unsigned long long r0 = (unsigned long long)cp.bstart[b] * uint32_t(CK2);
            if (r0 < n) {
                const long long down = (long long)(n - r0 < m ? n - r0 : m);
                steps = steps > down ? steps : down;
            }
            break;
        }
    if (steps < 0) return INT32_MIN;
    const long long v = steps * (long long)match;
    return v > 0x7FFFFFFFll ? 0x7FFFFFFF : int32_t(v);
}

// The aligner's corridor model (ioc_ctx::aln_fit): score per base of the pairs aligned so far against their summed error rate, one
// straight line per gap-open class (setGapOpen: 2..5).  Decides how wide a couple's corridor is PLANNED — which tiles are
// computed, never what comes out (the certificate and the re-run see to that).
struct CorridorFit {
    double n = 0, se = 0, sr = 0, see = 0, ser = 0, srr = 0, e_lo = 1e9, e_hi = -1e9;
};

// The corridor's half width as a fraction of the longer sequence (V2Couple; IOC_ALIGN_CORRIDOR=0: every tile; a pair whose
// result the corridor cannot vouch for is run again by the every-tile route).  0.2: a pair of one transcript scores 1.62 - 1.8
// per base at match 2 — it passes if 2 (1 - B / len) < 1.62 — and the tile grid of a 16.7 kb pair shrinks to about half.
// ROUND 5: the half width PER COUPLE, from the pairs' summed error rates.  A pair of one transcript scores
// rho = match - e x c per base, and passes the certificate iff B / length > 1 - rho / match.  Before anything has been aligned
// c comes from the error model behind setGapOpen's classes — a third each of substitutions (match - mismatch lost), insertions
// and deletions (gap open + the match) — plus 0.02 x length; once a gap-open class has 64 related pairs behind it (this
// context's earlier batches: ioc_ctx::aln_fit, fed by learn_corridor) the line fitted to THEM, 4.5 standard deviations down.
// Config 3: mean width 0.157 x length (round 4: 0.2 for everybody — set by the least similar pair of the batch).  A wrong
// guess costs time (the probe widens, or the pair is refuted and run again), never a result.
struct CorridorModel {
    const CorridorFit* fit;  // the four classes' records (ioc_ctx::aln_fit)
    AlnParams P;
    double frac;  // the fraction without a model (0: no corridor)
    bool fixed;   // (IOC_ALIGN_CORRIDOR: one fraction for every couple, as in round 4)
    bool fit_ok;  // `fit` belongs to these scores
    bool taper;   // the model's corridor narrows down the grid (IOC_ALIGN_CORRIDOR_TAPER=0: one width, the certificate of round 4)
    uint32_t taper_margin;  // columns on top of the taper's least passing width (IOC_ALIGN_CORRIDOR_MARGIN)
    // ... and the score per base it was derived from (rho_lo; 0: no model behind the fraction)
    struct Width {
        double frac, rho;
    };
    Width pair_width(const AlnPairDev& d) const
    {
        if (fixed || !(P.match > 0)) return {frac, 0.0};
        const double e = double(d.e_sum);
        if (!(e > 0.0) || !(e < 1.0)) return {frac, 0.0};
        const int go = std::max(2, std::min(5, d.gap_open));
        double rho = double(P.match) - e * (double(P.match - P.mismatch) / 3.0 + 2.0 / 3.0 * double(go + P.match)), margin = 0.02;
        const CorridorFit& f = fit[go - 2];
        if (fit_ok && f.n >= 64.0 && e >= f.e_lo - 0.02 && e <= f.e_hi + 0.02) {
            const double me = f.se / f.n, mr = f.sr / f.n, vee = f.see / f.n - me * me, ver = f.ser / f.n - me * mr, vrr = f.srr / f.n - mr * mr;
            const double slope = vee > 1e-9 ? ver / vee : 0.0;
            const double sd = std::sqrt(std::max(0.0, vrr - slope * ver));
            rho = mr + slope * (e - me) - 4.5 * std::max(sd, 0.004);
            margin = 0.003;
        }
        return {std::max(0.03, std::min(0.45, 1.0 - rho / double(P.match) + margin)), rho};
    }
    double pair_frac(const AlnPairDev& d) const { return pair_width(d).frac; }
};

// `fit`, `fit_sig_ok`: the context's four records, and whether they were summed under these scores (ioc_ctx::aln_fit_sig)
inline CorridorModel corridor_model(const AlnParams& P, bool corridor, const AlnPlanOpts& o, const CorridorFit* fit, bool fit_sig_ok)
{
    CorridorModel m{fit, P, corridor ? 0.2 : 0.0, false, false, true, 256u};
    if (o.corridor_fixed) {
        m.frac = corridor ? o.corridor_frac : 0.0;
        m.fixed = true;
    }
    m.taper = o.taper;
    m.taper_margin = o.taper_margin;
    m.fit_ok = fit_sig_ok && !o.no_fit;
    return m;
}

// Bands per couple.  A full batch (config 3: 811 couples) is bound by throughput: 11 bands of 1536 rows (66.8 ms; 7 of 2560:
// 69.2; 17 of 1024: worse again).  A small one (a merge aligns a few hundred representatives) is bound by ONE couple's
// critical path, (bands + strips - 1) tiles of rows / (4 bands) + 63 steps: more, shorter bands shorten it as long as the
// waves the chip holds outnumber the tiles in flight.
inline uint32_t band_target(uint32_t ncouples, uint32_t few_limit, int occ, int n_cu)
{
    const uint32_t waves = uint32_t(occ) * uint32_t(n_cu) * uint32_t(V2_WAVES);
    uint32_t want = std::max(12u, std::min(uint32_t(V2_MAX_BANDS), (waves + ncouples - 1u) / std::max(1u, ncouples)));
    // (with tiles that follow their left neighbours row by row — v2_wait_rows — a strip starts ~120 steps after the one on its
    // left whatever the band's height: fewer, taller bands win again.  A second round of 31 couples of 16.7 kb: 33 bands of 512
    // rows 16.6 ms, 17 of 1024 rows 14.9, 11 of 1536 rows 16.2; without: 16.9 / 19.4 / 23.5)
    if (few_limit && ncouples <= few_limit) want = std::min(want, 17u);
    return want;
}

// what align_v2_run plans on the host before its first launch
struct V2Plan {
    uint32_t cnt = 0, np = 0, ncouples = 0;
    std::vector<V2Couple> cps;
    std::vector<V2PairCk> pck;
    std::vector<V2PairEnd> pend;
    std::vector<uint64_t> cwords;  // arena words of a couple
    uint32_t lrow_total = 0, best_total = 0, max_strips = 1;
    uint64_t tiles_skipped = 0, tiles_all = 0;
    std::vector<std::pair<uint32_t, uint32_t>> slices;  // [first couple, count)
    uint64_t arena_words = 0, prof_total = 0;
    std::vector<uint32_t> n_items, n_probe, n_diag;  // per slice: tiles of its list, the probe launch's (they come first), anti-diagonals
    std::vector<std::vector<V2Item>> items;          // per slice: the host's list (tile_lists: IOC_V2_ITEMS_CHECK alone)
    uint32_t max_items = 0, max_flags = 0, max_pairs = 0;
};

// bands of whole coarse rows: enough of them for the anti-diagonals of the tile grid to keep the chip busy, each long enough
// (>= 1024 rows = 256 steps) for the 63 steps of pipeline fill to stay small (V2Couple::bstart)
inline void plan_bands(V2Couple& cp, uint32_t ncoarse, uint32_t want_bands, bool corridor)
{
    // (a pair long enough for a corridor: shorter bands follow the diagonal more closely — config 3 with the corridor: 17 bands
    // of 1024 rows 45.9 ms, 11 of 1536 47.6, 22 of 1024 / 512 46.1)
    const uint32_t wb = (corridor && ncoarse >= 16u) ? std::max(want_bands, 17u) : want_bands;
    const uint32_t reg = std::max<uint32_t>(want_bands > 16u ? 1u : 2u, (ncoarse + wb - 1) / wb);  // (coarse rows per band)
    // (measured on config 3: short first and last bands — 1, 2, 4 coarse rows, then the regular height, then 4, 2, 1 — cost
    // more in pipeline fill than they win: 69.9 against 69.2 ms at 7 regular bands)
    std::vector<uint32_t> hts;
    for (uint32_t left = ncoarse; left;) {
        const uint32_t hgt = std::min(reg, left);
        hts.push_back(hgt);
        left -= hgt;
    }
    while (hts.size() > size_t(V2_MAX_BANDS)) {  // (very long pairs: merge from the middle)
        const size_t mid = hts.size() / 2;
        hts[mid - 1] += hts[mid];
        hts.erase(hts.begin() + long(mid));
    }
    cp.nbands = uint32_t(hts.size());
    cp.tpb = reg;
    uint32_t acc = 0;
    for (uint32_t b = 0; b <= uint32_t(V2_MAX_BANDS); ++b) {
        cp.bstart[b] = uint16_t(std::min<uint32_t>(acc, 0xFFFFu));
        if (b < cp.nbands) acc += hts[b];
    }
}

// The corridor (V2Couple): tiles that meet |row - column| <= B, if that leaves out a fifth of the grid or more, and the probe.
// Returns the tiles the corridor skips; cert[h], start[h]: the parent bound and the start bound of pair h (V2PairEnd).
inline uint32_t plan_corridor(V2Couple& cp, const std::vector<AlnPairDev>& dp, const CorridorModel& cm, uint32_t nmax, uint32_t mmax, int32_t cert[2],
                              int32_t start[2])
{
    const AlnParams& P = cm.P;
    constexpr uint32_t probe_rows = 1024;
    cp.corridor = 0;
    for (uint32_t b = 0; b < uint32_t(V2_MAX_BANDS); ++b) {
        cp.plo[b] = 0;
        cp.phi[b] = uint16_t(std::min<uint32_t>(65535u, cp.nstrips - 1u));  // (V2Item::strip is 16 bits wide)
    }
    const uint32_t strip_cols = 64u * FW_C;
    double frac = 0.0, rho = double(P.match);
    for (int h = 0; h < 2; ++h)
        if (cp.pid[h] != 0xFFFFFFFFu) {  // (the wider plan of the two pairs)
            const CorridorModel::Width w = cm.pair_width(dp[cp.pid[h]]);
            frac = std::max(frac, w.frac);
            rho = std::min(rho, w.rho);
        }
    if (cm.frac <= 0.0) frac = 0.0;
    const uint32_t B = uint32_t(frac * double(std::max(nmax, mmax)));
    cp.b0 = B;
    int64_t beff = INT64_MAX;
    uint32_t skipped = 0;
    uint16_t lo[V2_MAX_BANDS], hi[V2_MAX_BANDS];
    // (the bound behind the certificate: a column of an alignment scores `match` at most — no reward for mismatches or gaps)
    const bool can = cm.frac > 0.0 && B >= strip_cols && cp.nstrips <= 65535u && cp.nbands <= uint32_t(V2_MAX_BANDS) && P.match > 0 && P.mismatch <= P.match &&
                     P.gap_extend >= 0;
    bool fits = can;
    for (int h = 0; fits && h < 2; ++h)
        if (cp.pid[h] != 0xFFFFFFFFu) fits = dp[cp.pid[h]].gap_open >= 0;
    // THE TAPER (model-planned corridors): a path that enters a skipped cell from a computed one is bound by the score the pass
    // stored at that exit cell (k_fwd2_cert), so the width only has to keep the exit cells' scores low enough — a cell d columns off
    // the diagonal at row i holds about rho i - go - ge d, and passes if d > (match - rho)(n - i) / (match + ge) to the right,
    // (match - rho)(n - i) / (rho + ge) to the left.  The top keeps today's width: there the start bound applies.
    const double g_right = rho > 0.0 ? std::max(0.0, double(P.match) - rho) / double(P.match + P.gap_extend) : 0.0;
    const double g_left = rho > 0.0 ? std::max(0.0, double(P.match) - rho) / (rho + double(P.gap_extend)) : 0.0;
    uint32_t pb = 0, ps = 0;
    auto geometry = [&](bool taper) {
        bool ok = true;
        beff = INT64_MAX;
        skipped = 0;
        for (uint32_t b = 0; ok && b < cp.nbands; ++b) {
            const uint32_t r0 = uint32_t(cp.bstart[b]) * uint32_t(CK2), r1 = std::min(nmax, uint32_t(cp.bstart[b + 1u]) * uint32_t(CK2));
            uint64_t d_left = B, d_right = B;
            if (taper) {
                const double left = nmax > r0 ? double(nmax - r0) : 0.0, top = B > r0 ? double(B - r0) : 0.0;
                d_left = uint64_t(std::max(top, g_left * left)) + cm.taper_margin;
                d_right = uint64_t(std::max(top, g_right * left)) + cm.taper_margin;
            }
            const uint32_t c_lo = r0 > d_left ? uint32_t(r0 - d_left) : 0u, c_hi = uint32_t(std::min<uint64_t>(mmax, uint64_t(r1) + d_right));
            if (c_hi <= c_lo) return false;  // (a band wholly below the last column's corridor: rows the longer query has alone)
            lo[b] = uint16_t(c_lo / strip_cols);
            hi[b] = uint16_t((c_hi - 1u) / strip_cols);
            skipped += lo[b] + (cp.nstrips - 1u - hi[b]);
            if (lo[b] > 0) beff = std::min<int64_t>(beff, int64_t(r0) - int64_t(lo[b]) * strip_cols);
            if ((uint64_t(hi[b]) + 1u) * strip_cols < mmax) beff = std::min<int64_t>(beff, int64_t(hi[b] + 1u) * strip_cols - int64_t(r1));
            // what v2_fwd_body relies on — of a computed tile off the border at most one of the tile above and the tile to its
            // left is missing — follows from: plo and phi never fall down the bands, and every band holds the strips of its own
            // diagonal cells (r0, r0) .. (r1, r1).  (One width for every band meets this by construction.)
            if (taper) {
                const uint32_t s0 = (r0 ? r0 - 1u : 0u) / strip_cols, s1 = std::min((r1 - 1u) / strip_cols, cp.nstrips - 1u);
                ok = lo[b] <= s0 && hi[b] >= s1 && (b == 0 || (lo[b] >= lo[b - 1u] && hi[b] >= hi[b - 1u]));
            }
        }
        if (!ok) return false;
        // the probe (V2Couple): the first band that ends at row 2048 or below, the strip its last diagonal cell is in; every tile
        // above and to the left of it must be inside the corridor with nothing missing around it, both pairs must reach it
        pb = 0;
        while (pb + 1u < cp.nbands && uint32_t(cp.bstart[pb + 1u]) * uint32_t(CK2) < probe_rows) ++pb;  // (3072 rows: a probe launch of 4.2 ms; 2048: 2.3)
        const uint32_t R = uint32_t(cp.bstart[pb + 1u]) * uint32_t(CK2);
        ps = (R - 1u) / strip_cols;
        ok = pb + 1u < cp.nbands && R >= probe_rows;
        for (uint32_t b = 0; ok && b <= pb; ++b) ok = lo[b] == 0 && hi[b] >= ps;
        for (int h = 0; ok && h < 2; ++h)
            if (cp.pid[h] != 0xFFFFFFFFu) ok = dp[cp.pid[h]].n >= R && dp[cp.pid[h]].m > ps * strip_cols;
        return ok && skipped * 5u >= cp.nbands * cp.nstrips && beff > 0 && beff < INT64_MAX;
    };
    // (a couple whose taper breaks a rule gets the one width of round 4, and its certificate)
    bool tapered = fits && cm.taper && !cm.fixed && rho > 0.0 && rho < double(P.match) && geometry(true);
    fits = tapered || (fits && geometry(false));
    cp.probe_band = uint16_t(fits ? pb : 0u);
    cp.probe_strip = uint16_t(fits ? ps : 0u);
    if (fits) {
        cp.corridor = 1;
        for (uint32_t b = 0; b < cp.nbands; ++b) {
            cp.plo[b] = lo[b];
            cp.phi[b] = hi[b];
        }
    }
    for (int h = 0; h < 2; ++h) {
        cert[h] = INT32_MIN;
        start[h] = INT32_MAX;  // (no exit-cell certificate: the parent bound alone, k_fwd2_ends)
        if (cp.pid[h] == 0xFFFFFFFFu || !cp.corridor) continue;
        const AlnPairDev& d = dp[cp.pid[h]];
        // (a path through a skipped cell has at most max(n, m) - Beff - 1 diagonal steps, each worth `match` at most)
        cert[h] = int32_t(std::min<int64_t>(INT32_MAX, int64_t(P.match) * std::max<int64_t>(0, int64_t(std::max(d.n, d.m)) - beff - 1)));
        if (tapered) start[h] = v2_start_bound(cp, d.n, d.m, P.match);
    }
    return cp.corridor ? skipped : 0u;
}

// the couple's checkpoints (V2Couple: rdat, rbase, cdat, cbase from the couple's start; slice_couples places them) in arena words
inline uint64_t couple_words(V2Couple& cp, uint32_t nmax, uint32_t mmax)
{
    auto up4 = [](uint64_t x) { return (x + 3u) & ~uint64_t(3); };
    cp.mpad = uint32_t((uint64_t(mmax) + 15u) & ~uint64_t(15));
    cp.nq = (nmax + 3u) / 4u;
    const uint64_t ncr = (nmax - 1u) / CK2, ncc = (mmax - 1u) / CK2;
    uint64_t w = 0;
    cp.rdat = w;
    w += up4(ncr * 2u * cp.mpad);
    cp.rbase = w;
    w += up4(ncr * (cp.mpad / 16u) * 2u);
    cp.cdat = w;
    w += up4(ncc * uint64_t(cp.nq) * 8u);
    cp.cbase = w;
    w += up4(ncc * uint64_t(cp.nq) * 2u);
    return w;
}

// the couples (pairs order[2 k2], order[2 k2 + 1]): tile grid, bands, corridor, probe, checkpoint words, and every pair's entries of
// the last-row and last-column bests
inline void plan_couples(V2Plan& pl, const std::vector<AlnPairDev>& dp, const uint32_t* order, const CorridorModel& cm, uint32_t want_bands)
{
    pl.cps.resize(pl.ncouples);
    pl.pck.resize(pl.np);
    pl.pend.resize(pl.np);
    pl.cwords.resize(pl.ncouples);
    for (uint32_t k2 = 0; k2 < pl.ncouples; ++k2) {
        V2Couple& cp = pl.cps[k2];
        cp.pid[0] = order[2u * k2];
        cp.pid[1] = 2u * k2 + 1u < pl.cnt ? order[2u * k2 + 1u] : 0xFFFFFFFFu;
        uint32_t nmax = 0, mmax = 0;
        for (int h = 0; h < 2; ++h)
            if (cp.pid[h] != 0xFFFFFFFFu) {
                nmax = std::max(nmax, dp[cp.pid[h]].n);
                mmax = std::max(mmax, dp[cp.pid[h]].m);
            }
        cp.nstrips = (mmax + 64u * FW_C - 1) / (64u * FW_C);
        plan_bands(cp, (nmax + CK2 - 1) / CK2, want_bands, cm.frac > 0.0);
        int32_t cert[2], start[2];
        pl.tiles_skipped += plan_corridor(cp, dp, cm, nmax, mmax, cert, start);
        pl.tiles_all += uint64_t(cp.nbands) * cp.nstrips;
        pl.cwords[k2] = couple_words(cp, nmax, mmax);
        cp.prof = 0;  // (uint4 entries; placed per slice: the profiles of a slice's couples count against the budget with its checkpoints)
        pl.max_strips = std::max(pl.max_strips, cp.nstrips);
        for (int h = 0; h < 2; ++h) {
            cp.lrow0[h] = pl.lrow_total;
            cp.best0[h] = pl.best_total;
            if (cp.pid[h] == 0xFFFFFFFFu) continue;
            const AlnPairDev& d = dp[cp.pid[h]];
            const uint32_t nstr = (d.m + 64u * FW_C - 1) / (64u * FW_C);
            pl.pend[cp.pid[h]] = V2PairEnd{pl.lrow_total, pl.best_total, cp.nbands, k2, cert[h], start[h], INT32_MIN};
            pl.lrow_total += nstr * 64u;
            pl.best_total += cp.nbands;
        }
    }
}

// slices of couples whose checkpoints and query profiles — and, in an emitting call, the operation bytes of their pairs (cops:
// per couple; empty otherwise) — fit the budget together
inline void slice_couples(V2Plan& pl, uint64_t budget, const std::vector<uint64_t>& cops)
{
    constexpr uint64_t prof_entry = 16;  // bytes of a profile entry (a uint4)
    for (uint32_t first = 0; first < pl.ncouples;) {
        uint64_t used = 0;
        uint32_t k2 = first;
        uint64_t prof_used = 0;  // uint4 entries of query profiles in this slice (they used to be made for every couple of the call at once)
        uint64_t ops_used = 0;
        while (k2 < pl.ncouples) {
            const uint64_t prof_k = uint64_t(pl.cps[k2].nstrips) * 2u * 5u * 64u, ops_k = cops.empty() ? 0u : cops[k2];
            if (k2 != first && (used + pl.cwords[k2]) * 4ull + (prof_used + prof_k) * prof_entry + ops_used + ops_k > budget) break;
            V2Couple& cp = pl.cps[k2];
            cp.prof = prof_used;
            prof_used += prof_k;
            cp.rdat += used;
            cp.rbase += used;
            cp.cdat += used;
            cp.cbase += used;
            for (int h = 0; h < 2; ++h)
                if (cp.pid[h] != 0xFFFFFFFFu) pl.pck[cp.pid[h]] = V2PairCk{cp.rdat, cp.rbase, cp.cdat, cp.cbase, cp.mpad, cp.nq, uint32_t(h), k2};
            used += pl.cwords[k2];
            ops_used += ops_k;
            ++k2;
        }
        pl.arena_words = std::max(pl.arena_words, used);
        pl.prof_total = std::max(pl.prof_total, prof_used);
        pl.slices.emplace_back(first, k2 - first);
        first = k2;
    }
}

// every slice's flags (V2Couple::flag0) and what the launches need to know of its list of tiles, in closed form from the grids:
// the list itself is made on the device (k_fwd2_items), in the order tile_lists defines
inline void tile_counts(V2Plan& pl)
{
    const size_t ns = pl.slices.size();
    pl.n_items.assign(ns, 0);
    pl.n_probe.assign(ns, 0);
    pl.n_diag.assign(ns, 1);
    for (size_t si = 0; si < ns; ++si) {
        const uint32_t k_lo = pl.slices[si].first, k_hi = pl.slices[si].first + pl.slices[si].second;
        uint32_t nf = 0;
        uint64_t n_all = 0, n_probe = 0;
        for (uint32_t k2 = k_lo; k2 < k_hi; ++k2) {
            V2Couple& cp = pl.cps[k2];
            cp.flag0 = nf;
            nf += cp.nbands * cp.nstrips;
            n_all += uint64_t(cp.nbands) * cp.nstrips;
            if (cp.corridor) n_probe += (uint64_t(cp.probe_band) + 1u) * (uint64_t(cp.probe_strip) + 1u);
            pl.n_diag[si] = std::max(pl.n_diag[si], cp.nbands + cp.nstrips - 1u);
        }
        pl.n_probe[si] = uint32_t(n_probe);
        pl.n_items[si] = uint32_t(n_probe + n_all);
        pl.max_items = std::max(pl.max_items, pl.n_items[si]);
        pl.max_flags = std::max(pl.max_flags, nf);
        pl.max_pairs = std::max(pl.max_pairs, std::min(pl.cnt, 2u * k_hi) - 2u * k_lo);
    }
}

// every slice's list of tiles and flags (V2Couple::flag0) on the host: the definition of the list's order, and what
// IOC_V2_ITEMS_CHECK holds the device's list against
inline void tile_lists(V2Plan& pl)
{
    pl.items.resize(pl.slices.size());
    pl.n_probe.assign(pl.slices.size(), 0);
    for (size_t si = 0; si < pl.slices.size(); ++si) {
        const uint32_t k_lo = pl.slices[si].first, k_hi = pl.slices[si].first + pl.slices[si].second;
        uint32_t nf = 0;
        auto& it = pl.items[si];
        uint32_t maxdiag = 0;
        size_t total_items = 0;
        for (uint32_t k2 = k_lo; k2 < k_hi; ++k2) {
            V2Couple& cp = pl.cps[k2];
            cp.flag0 = nf;
            nf += cp.nbands * cp.nstrips;
            total_items += size_t(cp.nbands) * cp.nstrips;
            maxdiag = std::max(maxdiag, cp.nbands + cp.nstrips - 2u);
        }
        // anti-diagonal by anti-diagonal, couples side by side: every tile comes after the tile above it and the tile to its left
        // (generated in that order: sorting 150 000 items cost 4 ms of host time per call)
        it.reserve(total_items + 64u * pl.slices[si].second);
        // first the probe's tiles (couples with a corridor: the top left corner of the grid, V2Couple), in the same order
        for (uint32_t dg = 0; dg <= maxdiag; ++dg) {
            bool any = false;
            for (uint32_t k2 = k_lo; k2 < k_hi; ++k2) {
                const V2Couple& cp = pl.cps[k2];
                if (!cp.corridor || dg > uint32_t(cp.probe_band) + cp.probe_strip) continue;
                any = true;
                const uint32_t b_lo = dg >= uint32_t(cp.probe_strip) + 1u ? dg - cp.probe_strip : 0u, b_hi = std::min<uint32_t>(dg, cp.probe_band);
                for (uint32_t b = b_lo; b <= b_hi; ++b) it.push_back(V2Item{k2, uint16_t(b), uint16_t(dg - b)});
            }
            if (!any && dg > 64u) break;
        }
        pl.n_probe[si] = uint32_t(it.size());
        for (uint32_t dg = 0; dg <= maxdiag; ++dg)
            for (uint32_t k2 = k_lo; k2 < k_hi; ++k2) {
                const V2Couple& cp = pl.cps[k2];
                if (dg > cp.nbands + cp.nstrips - 2u) continue;
                const uint32_t b_lo = dg >= cp.nstrips ? dg - cp.nstrips + 1u : 0u, b_hi = std::min(dg, cp.nbands - 1u);
                for (uint32_t b = b_lo; b <= b_hi; ++b) it.push_back(V2Item{k2, uint16_t(b), uint16_t(dg - b)});
            }
        pl.max_items = std::max<uint32_t>(pl.max_items, uint32_t(it.size()));
        pl.max_flags = std::max(pl.max_flags, nf);
        pl.max_pairs = std::max(pl.max_pairs, std::min(pl.cnt, 2u * k_hi) - 2u * k_lo);
    }
}

// IOC_V2_ITEMS_CHECK (developer switch): the host's lists into pl.items, and tile_counts' closed forms against what they say.
// Returns the first difference in words ("": none); the caller fails the call with it.
inline std::string tile_lists_check(V2Plan& pl)
{
    V2Plan ref = pl;
    ref.max_items = ref.max_flags = ref.max_pairs = 0;
    tile_lists(ref);
    for (size_t si = 0; si < pl.slices.size(); ++si)
        if (ref.items[si].size() != pl.n_items[si] || ref.n_probe[si] != pl.n_probe[si])
            return "IOC_V2_ITEMS_CHECK: slice " + std::to_string(si) + ": " + std::to_string(pl.n_items[si]) + " tiles, " + std::to_string(pl.n_probe[si]) +
                   " of the probe planned; the host's list has " + std::to_string(ref.items[si].size()) + " and " + std::to_string(ref.n_probe[si]);
    for (uint32_t k2 = 0; k2 < pl.ncouples; ++k2)
        if (ref.cps[k2].flag0 != pl.cps[k2].flag0) return "IOC_V2_ITEMS_CHECK: flag0 of couple " + std::to_string(k2) + " differs";
    if (ref.max_items != pl.max_items || ref.max_flags != pl.max_flags || ref.max_pairs != pl.max_pairs)
        return "IOC_V2_ITEMS_CHECK: max_items / max_flags / max_pairs differ from the host lists'";
    pl.items = std::move(ref.items);
    return std::string();
}

// ---- version 1 ----------------------------------------------------------------------------------------------------------

// waves per pair: few pairs -> wide workgroups (latency), many pairs -> narrow ones (no fill/drain waste)
struct WavePlan {
    uint32_t waves;
    bool few_pairs;  // a handful of long pairs (the later alignment rounds of a batch): 4-wave workgroups, several per pair (v1_slice)
};
// (max_n, max_m: the longest query and reference of the call's np device pairs)
inline WavePlan plan_waves(uint32_t max_n, uint32_t max_m, uint32_t np, bool carry, const AlnPlanOpts& o)
{
    uint32_t waves = ALN_MAXW;
    if (o.waves_set) {
        const int v = o.waves;
        if (v >= 1 && v <= ALN_MAXW) waves = uint32_t(v);
    } else {
        while (waves > 1 && uint64_t(np) * waves > 4096) waves >>= 1;
        if (carry) {
            while (waves > 1 && uint64_t(waves / 2) * 64 * ALN_C >= max_m) waves >>= 1;
        } else {
            // row bands x column strips run as a pipeline: it needs a few strips per band to fill, and
            // whole tiles per band
            const uint32_t strips = (max_m + 64 * FW_C - 1) / (64 * FW_C), tiles = (max_n + TILE - 1) / TILE;
            while (waves > 1 && (strips < 2 * waves || tiles < 2 * waves)) waves >>= 1;
        }
    }
    const bool few_pairs = !carry && !o.waves_set && np <= 64 && waves >= 4 && !o.no_cross_tail;
    return WavePlan{few_pairs ? 4u : waves, few_pairs};
}

// checkpoint arena: slices of pairs (in `order`, from n_v2 on) whose checkpoints fit the budget together, one kernel per slice
struct V1Plan {
    std::vector<AlnCk> cko;
    std::vector<std::pair<uint32_t, uint32_t>> slices;  // [first, count) in `order`
    uint64_t arena = 0;                                 // int2 units
    uint32_t max_cnt = 0;
    std::vector<uint64_t> ops_end, slice_ops;           // (emitting call) per pair: the end of its region of operation bytes; per slice: its bytes
    uint64_t ops_most = 0;
};
inline uint64_t v1_row_units(const AlnPairDev& d) { return uint64_t((d.n - 1) / TILE) * row_pitch(d.m); }

inline V1Plan plan_v1(const std::vector<AlnPairDev>& dp, const uint32_t* order, uint32_t n_v2, uint64_t budget, bool emit)
{
    const uint32_t np = uint32_t(dp.size());
    V1Plan pl;
    pl.cko.resize(np);
    if (emit) pl.ops_end.assign(np, 0);
    for (uint32_t first = n_v2; first < np;) {
        uint64_t used = 0, ops_used = 0;
        uint32_t cnt = 0;
        while (first + cnt < np) {
            const AlnPairDev& d = dp[order[first + cnt]];
            const uint64_t u = v1_row_units(d) + uint64_t((d.m - 1) / TILE) * col_pitch(d.n);
            const uint64_t ops_u = emit ? uint64_t(d.n) + d.m : 0u;
            if (cnt > 0 && (used + u) * 8ull + ops_used + ops_u > budget) break;
            if (cnt > 0 && (d.pad != 0) != (dp[order[first]].pad != 0)) break;  // one kernel per slice
            // (rows first: their pitch is a multiple of 16 int2, `used` stays 16-byte aligned for the int4 stores)
            pl.cko[order[first + cnt]] = AlnCk{used, used + v1_row_units(d)};
            used += u;
            ops_used += ops_u;
            if (emit) pl.ops_end[order[first + cnt]] = ops_used;
            ++cnt;
        }
        pl.slice_ops.push_back(ops_used);
        pl.ops_most = std::max(pl.ops_most, ops_used);
        pl.arena = std::max(pl.arena, used);
        pl.slices.emplace_back(first, cnt);
        pl.max_cnt = std::max(pl.max_cnt, cnt);
        first += cnt;
    }
    return pl;
}
