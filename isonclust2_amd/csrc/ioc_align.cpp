// ioc_align.cpp — host semi-global aligner for the sahlin / furious fallback.
//
// The reference calls parasail (src/cluster.cpp:408-423, 461-515): parasail_sg_trace_scan_16 / _32 with
// match 2, mismatch -2, gap open from setGapOpen(e1+e2) (2..5), gap extend 1, then
// parasail_result_get_traceback(..., '|', ' ', ' ') and getAlnRatio over the `comp` string.  parasail is
// a third-party library absent from /root/reference (.gitmodules:4-6, version unrecoverable): this is a
// from-scratch Gotoh aligner with the published semantics of that call (all four sequence ends free;
// a gap of length n costs open + (n-1)*extend; traceback covers the end-gap columns).  Parity with
// parasail's tie-breaking is UNPINNED except for the reference's single AlnRatioTest vector
// (test/isONclust2_test.cpp:137-181), which tests/test_align_host.py checks.
// The fallback stays on the host by design (BASELINE.json north_star).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "isonclust2_hip.h"
#include "ioc_align_sink.h"
#include "ioc_pile_call.h"
#include "ioc_pile_sites.h"
#include "ioc_read_blocks.h"
#include "ioc_read_inserts.h"
#include "ioc_read_ends.h"
#include "ioc_insert_windows.h"
#include "ioc_window_variants.h"
#include "ioc_sink_plan.h"
#include "ioc_iso_splice.h"
#include "ioc_read_correct.h"
#include "ioc_iso_correct.h"
#include "ioc_site_split.h"

namespace {

// direction bits of the traceback matrix, 1 byte per cell
enum : uint8_t { H_DIAG = 0, H_FROM_E = 1, H_FROM_F = 2, H_MASK = 3, E_EXT = 4, F_EXT = 8 };

// The aligner behind ioc_host_align and ioc_host_align_ops: one DP, one walk.  `comp` receives one byte per alignment column,
// forward order, NUL-terminated — OPS: the operation bytes ('=' 'X' 'I' 'D', free end gaps 'i' 'd'), else the comparison
// string ('|' where the operation is '=', ' ' everywhere else).  Returns the length, or a negative ioc_status.
// `cor` (ioc_host_align_corridor alone, null otherwise): only the cells (i, cor->jlo[i] .. cor->jhi[i]) of row i >= 1 are computed,
// every other cell off row 0 and column 0 counts as "no score"; what comes out is the best alignment among the paths that stay
// inside the computed cells, with the exit bound of its certificate (HostCorridor).
struct HostCorridor {
    std::vector<int> jlo, jhi;  // [0 .. n + 1]: the computed columns of a row (jlo > jhi: none); row n + 1 stands for "no such row"
    bool skipped(int i, int j) const { return j < jlo[size_t(i)] || j > jhi[size_t(i)]; }
    int64_t exit_bound = INT64_MIN;  // the largest H_C(y) + match x min(n - i, m - j) over the exit cells y = (i, j)
    int end_i = 0, end_j = 0;
};

template <bool OPS>
int host_align(const char* query, int32_t qlen, const char* ref, int32_t rlen, int32_t match, int32_t mismatch, int32_t gap_open,
               int32_t gap_extend, char* comp, int32_t comp_cap, int32_t* score_out, HostCorridor* cor = nullptr)
{
    // what a column of each kind is written as
    constexpr char C_EQ = OPS ? '=' : '|', C_X = OPS ? 'X' : ' ', C_I = OPS ? 'I' : ' ', C_D = OPS ? 'D' : ' ', C_EI = OPS ? 'i' : ' ',
                   C_ED = OPS ? 'd' : ' ';
    if (!query || !ref || !comp || qlen < 0 || rlen < 0) return IOC_ERR_ARG;
    if (comp_cap < qlen + rlen + 1) return IOC_ERR_CAPACITY;
    const int n = qlen, m = rlen;
    if (uint64_t(n + 1) * uint64_t(m + 1) > (1ull << 33)) return IOC_ERR_CAPACITY;
    const int NEG = INT32_MIN / 4;
    std::vector<uint8_t> tb(size_t(n + 1) * size_t(m + 1), 0);
    std::vector<int> H(size_t(m) + 1, 0), F(size_t(m) + 1, NEG), Hprev(size_t(m) + 1, 0);
    // free leading gaps on both sequences: first row and first column are 0
    int best = NEG, bi = n, bj = m;
    for (int i = 1; i <= n; ++i) {
        std::swap(H, Hprev);
        H[0] = 0;
        int E = NEG;
        const char qc = query[i - 1];
        uint8_t* row = tb.data() + size_t(i) * size_t(m + 1);
        for (int j = 1; j <= m; ++j) {
            if (cor && cor->skipped(i, j)) {
                H[j] = F[j] = E = NEG;
                continue;
            }
            // E: gap in the query (horizontal move), F: gap in the reference (vertical move)
            const int e_open = H[j - 1] - gap_open, e_ext = E - gap_extend;
            uint8_t d = 0;
            if (e_ext > e_open) {
                E = e_ext;
                d |= E_EXT;
            } else {
                E = e_open;
            }
            const int f_open = Hprev[j] - gap_open, f_ext = F[j] - gap_extend;
            if (f_ext > f_open) {
                F[j] = f_ext;
                d |= F_EXT;
            } else {
                F[j] = f_open;
            }
            const int diag = Hprev[j - 1] + (qc == ref[j - 1] ? match : mismatch);
            int h = diag;
            uint8_t from = H_DIAG;
            if (E > h) {
                h = E;
                from = H_FROM_E;
            }
            if (F[j] > h) {
                h = F[j];
                from = H_FROM_F;
            }
            H[j] = h;
            row[j] = uint8_t(d | from);
            if (cor) {
                // ("no score" stays where it is: sums of it do not drift towards the scores)
                if (E < NEG / 2) E = NEG;
                if (F[j] < NEG / 2) F[j] = NEG;
                if (h < NEG / 2) {
                    H[j] = NEG;
                    continue;
                }
                // an exit cell: a computed cell whose right, lower or lower-right neighbour exists and is skipped
                const bool right = j < m && cor->skipped(i, j + 1), below = i < n && cor->skipped(i + 1, j),
                           corner = i < n && j < m && cor->skipped(i + 1, j + 1);
                if (right || below || corner) cor->exit_bound = std::max(cor->exit_bound, int64_t(h) + int64_t(match) * std::min(n - i, m - j));
            }
        }
        // free trailing gap on the reference: best of the last column
        if (H[m] > best) {
            best = H[m];
            bi = i;
            bj = m;
        }
    }
    // free trailing gap on the query: best of the last row
    if (n == 0) std::fill(H.begin(), H.end(), 0);
    for (int j = 0; j <= m; ++j) {
        const int v = (n == 0) ? 0 : H[j];
        if (v > best) {
            best = v;
            bi = n;
            bj = j;
        }
    }
    if (score_out) *score_out = best;
    if (cor) {
        cor->end_i = bi;
        cor->end_j = bj;
    }
    // traceback from (bi, bj); trailing end gaps first (they are the tail of the strings)
    std::string rev;
    rev.reserve(size_t(n + m));
    for (int j = m; j > bj; --j) rev.push_back(C_ED);
    for (int i = n; i > bi; --i) rev.push_back(C_EI);
    int i = bi, j = bj, state = 0;  // 0 = H, 1 = E, 2 = F
    while (i > 0 && j > 0) {
        const uint8_t t = tb[size_t(i) * size_t(m + 1) + size_t(j)];
        if (state == 0) {
            const uint8_t from = t & H_MASK;
            if (from == H_DIAG) {
                rev.push_back(query[i - 1] == ref[j - 1] ? C_EQ : C_X);
                --i;
                --j;
            } else if (from == H_FROM_E) {
                state = 1;
            } else {
                state = 2;
            }
        } else if (state == 1) {
            rev.push_back(C_D);
            if (!(t & E_EXT)) state = 0;
            --j;
        } else {
            rev.push_back(C_I);
            if (!(t & F_EXT)) state = 0;
            --i;
        }
    }
    for (; j > 0; --j) rev.push_back(C_ED);
    for (; i > 0; --i) rev.push_back(C_EI);
    const int len = int(rev.size());
    if (len + 1 > comp_cap) return IOC_ERR_CAPACITY;
    for (int k = 0; k < len; ++k) comp[k] = rev[size_t(len - 1 - k)];
    comp[len] = 0;
    return len;
}

}  // namespace

extern "C" {

// Semi-global alignment of query (rows) against ref (columns).  Writes the comparison string of the
// whole alignment ('|' identical bases, ' ' otherwise, end-gap columns included) into comp (capacity
// comp_cap >= qlen + rlen + 1) and returns its length, or a negative ioc_status.
int ioc_host_align(const char* query, int32_t qlen, const char* ref, int32_t rlen, int32_t match,
                   int32_t mismatch, int32_t gap_open, int32_t gap_extend, char* comp, int32_t comp_cap,
                   int32_t* score_out)
{
    return host_align<false>(query, qlen, ref, rlen, match, mismatch, gap_open, gap_extend, comp, comp_cap, score_out);
}

// The same cells and the same walk, one operation byte per column in place of '|' / ' ': '=' equal bases, 'X' different bases,
// 'I' a query base against a gap (the walk's F state), 'D' a reference base against a gap (E state); 'i' / 'd' the same in a
// free end gap.  Order of the end gaps: leading 'i's, leading 'd's, the walk, trailing 'i's, trailing 'd's.
int ioc_host_align_ops(const char* query, int32_t qlen, const char* ref, int32_t rlen, int32_t match, int32_t mismatch,
                       int32_t gap_open, int32_t gap_extend, char* ops, int32_t ops_cap, int32_t* score_out)
{
    return host_align<true>(query, qlen, ref, rlen, match, mismatch, gap_open, gap_extend, ops, ops_cap, score_out);
}

// The aligner restricted to a corridor of tiles, and the certificate of what it finds: the host's statement of what version 2 of
// the GPU aligner computes under a corridor.  Band b holds the rows (r0, r0 + band_rows[b]] with r0 the heights
// before it (they must add up to qlen or more), strip p the columns (p strip_cols, (p + 1) strip_cols]; tile (b, p) is computed iff
// plo[b] <= p <= phi[b] (phi is cut to the pair's last strip).  Row 0 and column 0 always hold their zeros.
// out[0 .. 8): restricted score, end row, end column | the parent bound match x (max(n, m) - Beff - 1) (INT32_MAX: some skipped
// cell is on the diagonal), the start bound, the exit bound (INT32_MIN each: no such cell) | tiles skipped, tiles of the grid.
// The restricted alignment IS the alignment whenever out[0] > min(out[3], max(out[4], out[5])).
// `ops` (may be null): the restricted alignment's operation bytes, as ioc_host_align_ops writes them; returns their length (0
// without `ops`) or a negative ioc_status.
int ioc_host_align_corridor(const char* query, int32_t qlen, const char* ref, int32_t rlen, int32_t match, int32_t mismatch, int32_t gap_open,
                            int32_t gap_extend, const int32_t* band_rows, int32_t nbands, int32_t strip_cols, const int32_t* plo, const int32_t* phi,
                            char* ops, int32_t ops_cap, int32_t* out)
{
    if (!query || !ref || !band_rows || !plo || !phi || !out || qlen < 1 || rlen < 1 || nbands < 1 || strip_cols < 1 || match < 0) return IOC_ERR_ARG;
    const int n = qlen, m = rlen, W = strip_cols, nstrips = (m + W - 1) / W;
    HostCorridor cor;
    cor.jlo.assign(size_t(n) + 2, 1);
    cor.jhi.assign(size_t(n) + 2, 0);
    int64_t beff = INT64_MAX, tiles = 0, skipped = 0;
    int64_t start = INT64_MIN;
    int r0 = 0;
    for (int b = 0; b < nbands && r0 < n; ++b) {
        if (band_rows[b] < 1 || plo[b] < 0) return IOC_ERR_ARG;
        const int r1 = int(std::min<int64_t>(n, int64_t(r0) + band_rows[b])), lo = plo[b], hi = std::min(phi[b], nstrips - 1);
        if (lo > hi) return IOC_ERR_ARG;
        for (int i = r0 + 1; i <= r1; ++i) {
            cor.jlo[size_t(i)] = lo * W + 1;
            cor.jhi[size_t(i)] = int(std::min<int64_t>(m, (int64_t(hi) + 1) * W));
        }
        tiles += nstrips;
        skipped += lo + (nstrips - 1 - hi);
        // (the least |row - column| of a skipped cell, short by one on either side: plan_corridor's)
        if (lo > 0) beff = std::min<int64_t>(beff, int64_t(r0) - int64_t(lo) * W);
        if ((int64_t(hi) + 1) * W < m) beff = std::min<int64_t>(beff, (int64_t(hi) + 1) * W - r1);
        r0 = r1;
    }
    if (r0 < n) return IOC_ERR_ARG;
    // the start bound: a path whose first cell off row 0 and column 0 is skipped leaves (0, j) or (i, 0) by a step down or right
    // or diagonally, and has min(n, m - j) or min(n - i, m) diagonal steps at most
    for (int j = 0; j < m; ++j)
        if (cor.skipped(1, j + 1) || (j >= 1 && cor.skipped(1, j))) start = std::max(start, int64_t(match) * std::min(n, m - j));
    for (int i = 0; i < n; ++i)
        if (cor.skipped(i + 1, 1) || (i >= 1 && cor.skipped(i, 1))) start = std::max(start, int64_t(match) * std::min(n - i, m));
    int32_t score = 0;
    std::vector<char> own;
    if (!ops) {
        own.resize(size_t(n) + size_t(m) + 1);
        ops = own.data();
        ops_cap = int32_t(own.size());
    }
    const int len = host_align<true>(query, qlen, ref, rlen, match, mismatch, gap_open, gap_extend, ops, ops_cap, &score, &cor);
    if (len < 0) return len;
    auto i32 = [](int64_t v) { return int32_t(std::max<int64_t>(INT32_MIN, std::min<int64_t>(INT32_MAX, v))); };
    out[0] = score;
    out[1] = cor.end_i;
    out[2] = cor.end_j;
    out[3] = beff == INT64_MAX ? INT32_MIN : beff <= 0 ? INT32_MAX : i32(int64_t(match) * std::max<int64_t>(0, int64_t(std::max(n, m)) - beff - 1));
    out[4] = i32(start);
    out[5] = i32(cor.exit_bound);
    out[6] = i32(skipped);
    out[7] = i32(tiles);
    return own.empty() ? len : 0;
}

// Run-length text of an operation string ("12=1X3I", end gaps as runs of 'i' / 'd'), NUL-terminated.  Returns its length,
// IOC_ERR_CAPACITY when cap cannot hold it with the terminator, IOC_ERR_ARG for a byte that is no operation.
int64_t ioc_host_ops_to_cigar(const char* ops, int64_t len, char* out, int64_t cap)
{
    if (len < 0 || (len > 0 && !ops) || !out || cap < 1) return IOC_ERR_ARG;
    int64_t w = 0;
    for (int64_t a = 0; a < len;) {
        const char op = ops[a];
        if (!strchr("=XIDid", op) || op == 0) return IOC_ERR_ARG;
        int64_t b = a;
        while (b < len && ops[b] == op) ++b;
        const std::string run = std::to_string(b - a) + op;
        if (w + int64_t(run.size()) + 1 > cap) return IOC_ERR_CAPACITY;
        memcpy(out + w, run.data(), run.size());
        w += int64_t(run.size());
        a = b;
    }
    out[w] = 0;
    return w;
}

// The statistics of an operation string: counts per byte, the maximal runs of 'I' and of 'D', and the end gaps on either side of
// the walk (the bytes from the first to the last of "=XID").  The definition the device's reduction (k_ops_stats) is tested against.
int ioc_host_ops_stats(const char* ops, int64_t len, ioc_aln_stats* out)
{
    if (len < 0 || len > INT32_MAX || (len > 0 && !ops) || !out) return IOC_ERR_ARG;
    ioc_aln_stats s{};
    int64_t first = len, last = -1;  // the walk's first and last byte
    for (int64_t a = 0; a < len; ++a) {
        const char op = ops[a];
        if (!strchr("=XIDid", op) || op == 0) return IOC_ERR_ARG;
        if (op == 'i' || op == 'd') continue;
        if (first == len) first = a;
        last = a;
    }
    s.length = int32_t(len);
    for (int64_t a = 0; a < len;) {
        const char op = ops[a];
        int64_t b = a;
        while (b < len && ops[b] == op) ++b;
        const int32_t run = int32_t(b - a);
        switch (op) {
        case '=': s.matches += run; break;
        case 'X': s.mismatches += run; break;
        case 'I': s.ins += run, s.ins_runs += 1, s.longest_ins = std::max(s.longest_ins, run); break;
        case 'D': s.del += run, s.del_runs += 1, s.longest_del = std::max(s.longest_del, run); break;
        case 'i': a < first ? s.lead_i += run : a > last ? s.trail_i += run : 0; break;
        default: a < first ? s.lead_d += run : a > last ? s.trail_d += run : 0; break;  // ('d')
        }
        a = b;
    }
    s.columns = s.matches + s.mismatches + s.ins + s.del;
    *out = s;
    return IOC_OK;
}

// The pileup of one operation string on its reference (ioc_pileup_col, isonclust2_hip.h), ADDED to cols[0 .. rlen].  The
// definition the device's reduction (k_ops_pileup) is tested against.  A string that is refused leaves cols untouched.
int ioc_host_ops_pileup(const char* ops, int64_t len, const char* query, int32_t qlen, int32_t rlen, ioc_pileup_col* cols)
{
    if (len < 0 || len > INT32_MAX || (len > 0 && !ops) || qlen < 0 || rlen < 0 || (qlen > 0 && !query) || !cols) return IOC_ERR_ARG;
    int64_t q = 0, r = 0;
    for (int64_t a = 0; a < len; ++a) {
        const char op = ops[a];
        if (!strchr("=XIDid", op) || op == 0) return IOC_ERR_ARG;
        q += op == '=' || op == 'X' || op == 'I' || op == 'i';
        r += op == '=' || op == 'X' || op == 'D' || op == 'd';
    }
    if (q != qlen || r != rlen) return IOC_ERR_ARG;
    q = r = 0;
    for (int64_t a = 0; a < len; ++a) {
        switch (ops[a]) {
        case 'd': ++r; break;
        case 'i': ++q; break;
        case 'D': cols[r++].del += 1; break;
        case 'I':
            cols[r].ins_bases += 1;
            if (a == 0 || ops[a - 1] != 'I') cols[r].ins_runs += 1;
            ++q;
            break;
        default: {  // ('=' 'X')
            ioc_pileup_col& c = cols[r++];
            switch (query[q++]) {
            case 'A': c.a += 1; break;
            case 'C': c.c += 1; break;
            case 'G': c.g += 1; break;
            case 'T': c.t += 1; break;
            default: c.other += 1; break;
            }
        }
        }
    }
    return IOC_OK;
}

// What the 'I' bytes of one string insert (ioc_pileup_ins, isonclust2_hip.h), ADDED to ins[0 .. rlen]: the walk and the refusals
// of ioc_host_ops_pileup.  The definition the ins variant of k_ops_pileup is tested against.
int ioc_host_ops_pileup_ins(const char* ops, int64_t len, const char* query, int32_t qlen, int32_t rlen, ioc_pileup_ins* ins)
{
    if (len < 0 || len > INT32_MAX || (len > 0 && !ops) || qlen < 0 || rlen < 0 || (qlen > 0 && !query) || !ins) return IOC_ERR_ARG;
    int64_t q = 0, r = 0;
    for (int64_t a = 0; a < len; ++a) {
        const char op = ops[a];
        if (!strchr("=XIDid", op) || op == 0) return IOC_ERR_ARG;
        q += op == '=' || op == 'X' || op == 'I' || op == 'i';
        r += op == '=' || op == 'X' || op == 'D' || op == 'd';
    }
    if (q != qlen || r != rlen) return IOC_ERR_ARG;
    q = r = 0;
    int64_t j = 0;  // the index of an 'I' in its run
    for (int64_t a = 0; a < len; ++a) {
        const char op = ops[a];
        if (op == 'I') {
            if (j < IOC_PILE_INS_SLOTS)
                ins[r].slot[j][PileAcc::channel(uint8_t(query[q]))] += 1;
            else
                ins[r].longer += 1;
            ++j, ++q;
            continue;
        }
        j = 0;
        q += op == '=' || op == 'X' || op == 'i';
        r += op == '=' || op == 'X' || op == 'D' || op == 'd';
    }
    return IOC_OK;
}

// The consensus call of one reference from its two tables (isonclust2_hip.h has the rules; pile_call_row, ioc_pile_call.h, decides
// a row for this function and for the kernels of ioc_pile_call.hip alike).
int64_t ioc_host_pileup_call(const ioc_pileup_col* cols, const ioc_pileup_ins* ins, const char* frame, int32_t rlen, int32_t min_depth,
                             char* out_seq, char* out_qual, int64_t cap, ioc_polish_stats* st)
{
    if (min_depth < 1 || rlen < 0 || !cols || !ins || (rlen > 0 && !frame)) return IOC_ERR_ARG;
    const int64_t bound = int64_t(rlen) + int64_t(IOC_PILE_INS_SLOTS) * (int64_t(rlen) + 1);
    if (cap < bound) return IOC_ERR_CAPACITY;
    if (!out_seq || !out_qual) return IOC_ERR_ARG;
    ioc_polish_stats s{};
    int64_t at = 0;
    for (int32_t p = 0; p <= rlen; ++p) {
        const unsigned long long d_ins = p < rlen ? pile_depth(cols[p]) : rlen > 0 ? pile_depth(cols[rlen - 1]) : 0ull;
        const PileRowCall row = pile_call_row(cols[p], ins[p], d_ins, p < rlen, p < rlen ? uint8_t(frame[p]) : uint8_t(0), min_depth);
        for (uint32_t x = 0; x < row.n; ++x) {
            out_seq[at] = char((row.seq >> (8u * x)) & 0xFFu);
            out_qual[at++] = char((row.qual >> (8u * x)) & 0xFFu);
        }
        s.n_ins += int32_t(row.n_ins), s.n_sub += int32_t(row.n_sub), s.n_del += int32_t(row.n_del), s.n_low += int32_t(row.n_low);
    }
    s.out_len = int32_t(at);
    if (st) *st = s;
    return at;
}

// The weight a quality byte gives its base in the weighted pileup: the Phred value it writes, at least 1 and at most 93.
uint32_t ioc_host_qual_weight(uint8_t b) { return pile_qual_weight(b); }

// The weighted pileup of one operation string (isonclust2_hip.h has the rules): the walk and the refusals of ioc_host_ops_pileup,
// sums of weights ADDED to wcols[0 .. rlen] and, where wins is given, to wins[0 .. rlen].  The definition the weighted variant of
// k_ops_pileup is tested against.
int ioc_host_ops_pileup_weighted(const char* ops, int64_t len, const char* query, const char* qual, int32_t qlen, int32_t rlen,
                                 ioc_pileup_col* wcols, ioc_pileup_ins* wins)
{
    if (len < 0 || len > INT32_MAX || (len > 0 && !ops) || qlen < 0 || rlen < 0 || (qlen > 0 && (!query || !qual)) || !wcols) return IOC_ERR_ARG;
    int64_t q = 0, r = 0;
    for (int64_t a = 0; a < len; ++a) {
        const char op = ops[a];
        if (!strchr("=XIDid", op) || op == 0) return IOC_ERR_ARG;
        q += op == '=' || op == 'X' || op == 'I' || op == 'i';
        r += op == '=' || op == 'X' || op == 'D' || op == 'd';
    }
    if (q != qlen || r != rlen) return IOC_ERR_ARG;
    q = r = 0;
    int64_t j = 0;  // the index of an 'I' in its run
    for (int64_t a = 0; a < len; ++a) {
        const char op = ops[a];
        if (op == 'I') {
            const uint32_t w = pile_qual_weight(uint8_t(qual[q]));
            if (wins && j < IOC_PILE_INS_SLOTS)
                wins[r].slot[j][PileAcc::channel(uint8_t(query[q]))] += w;
            else if (wins)
                wins[r].longer += w;
            ++j, ++q;
            continue;
        }
        j = 0;
        switch (op) {
        case 'd': ++r; break;
        case 'i': ++q; break;
        case 'D': {
            const uint32_t wa = q > 0 ? pile_qual_weight(uint8_t(qual[q - 1])) : 0u, wb = q < qlen ? pile_qual_weight(uint8_t(qual[q])) : 0u;
            wcols[r++].del += wa == 0u ? (wb == 0u ? 1u : wb) : wb == 0u ? wa : std::min(wa, wb);
            break;
        }
        default: {  // ('=' 'X')
            ioc_pileup_col& c = wcols[r++];
            const uint32_t w = pile_qual_weight(uint8_t(qual[q]));
            switch (query[q++]) {
            case 'A': c.a += w; break;
            case 'C': c.c += w; break;
            case 'G': c.g += w; break;
            case 'T': c.t += w; break;
            default: c.other += w; break;
            }
        }
        }
    }
    return IOC_OK;
}

// The weighted consensus call of one reference: the depths of the table of counts gate, the tables of weights decide
// (pile_call_row with both gates, as the weighted mode of the kernels of ioc_pile_call.hip has it).
int64_t ioc_host_pileup_call_weighted(const ioc_pileup_col* cols, const ioc_pileup_col* wcols, const ioc_pileup_ins* wins, const char* frame,
                                      int32_t rlen, int32_t min_depth, char* out_seq, char* out_qual, int64_t cap, ioc_polish_stats* st)
{
    if (min_depth < 1 || rlen < 0 || !cols || !wcols || !wins || (rlen > 0 && !frame)) return IOC_ERR_ARG;
    const int64_t bound = int64_t(rlen) + int64_t(IOC_PILE_INS_SLOTS) * (int64_t(rlen) + 1);
    if (cap < bound) return IOC_ERR_CAPACITY;
    if (!out_seq || !out_qual) return IOC_ERR_ARG;
    ioc_polish_stats s{};
    int64_t at = 0;
    for (int32_t p = 0; p <= rlen; ++p) {
        const int32_t pi = p < rlen ? p : rlen - 1;  // the row the insertions in front of p are held against
        const unsigned long long dw_ins = pi >= 0 ? pile_depth(wcols[pi]) : 0ull, dc_ins = pi >= 0 ? pile_depth(cols[pi]) : 0ull;
        const PileRowCall row = pile_call_row(wcols[p], wins[p], dw_ins, p < rlen, p < rlen ? uint8_t(frame[p]) : uint8_t(0), min_depth, dc_ins,
                                              p < rlen ? pile_depth(cols[p]) : 0ull);
        for (uint32_t x = 0; x < row.n; ++x) {
            out_seq[at] = char((row.seq >> (8u * x)) & 0xFFu);
            out_qual[at++] = char((row.qual >> (8u * x)) & 0xFFu);
        }
        s.n_ins += int32_t(row.n_ins), s.n_sub += int32_t(row.n_sub), s.n_del += int32_t(row.n_del), s.n_low += int32_t(row.n_low);
    }
    s.out_len = int32_t(at);
    if (st) *st = s;
    return at;
}

// The projection of one operation string on its reference (isonclust2_hip.h has the rules): what ioc_host_ops_pileup adds to a
// row, kept per read — the definition k_ops_project (ioc_pile_sites.hip) is tested against.
int ioc_host_ops_project(const char* ops, int64_t len, const char* query, int32_t qlen, int32_t rlen, uint8_t* base, uint8_t* insf)
{
    if (len < 0 || len > INT32_MAX || (len > 0 && !ops) || qlen < 0 || rlen < 0 || (qlen > 0 && !query) || !base || !insf) return IOC_ERR_ARG;
    int64_t q = 0, r = 0;
    for (int64_t a = 0; a < len; ++a) {
        const char op = ops[a];
        if (!strchr("=XIDid", op) || op == 0) return IOC_ERR_ARG;
        q += op == '=' || op == 'X' || op == 'I' || op == 'i';
        r += op == '=' || op == 'X' || op == 'D' || op == 'd';
    }
    if (q != qlen || r != rlen) return IOC_ERR_ARG;
    memset(base, IOC_ALLELE_NONE, size_t(rlen) + 1);
    memset(insf, 0, size_t(rlen) + 1);
    q = r = 0;
    for (int64_t a = 0; a < len; ++a) {
        switch (ops[a]) {
        case 'd': ++r; break;
        case 'i': ++q; break;
        case 'D': base[r++] = uint8_t(IOC_ALLELE_DEL); break;
        case 'I':
            if (a == 0 || ops[a - 1] != 'I') insf[r] = 1;
            ++q;
            break;
        default: base[r++] = uint8_t(PileAcc::channel(uint8_t(query[q++]))); break;  // ('=' 'X')
        }
    }
    return IOC_OK;
}

// The insertion part of a read's projection (isonclust2_hip.h has the rules): which bases the read inserts in front of every row,
// slot-major — the definition k_ops_project_ins (ioc_plane_pile.hip) is tested against.  The walk and the refusals of
// ioc_host_ops_pileup_ins.
int ioc_host_ops_project_ins(const char* ops, int64_t len, const char* query, int32_t qlen, int32_t rlen, uint8_t* slots)
{
    if (len < 0 || len > INT32_MAX || (len > 0 && !ops) || qlen < 0 || rlen < 0 || (qlen > 0 && !query) || !slots) return IOC_ERR_ARG;
    int64_t q = 0, r = 0;
    for (int64_t a = 0; a < len; ++a) {
        const char op = ops[a];
        if (!strchr("=XIDid", op) || op == 0) return IOC_ERR_ARG;
        q += op == '=' || op == 'X' || op == 'I' || op == 'i';
        r += op == '=' || op == 'X' || op == 'D' || op == 'd';
    }
    if (q != qlen || r != rlen) return IOC_ERR_ARG;
    const size_t rows = size_t(rlen) + 1;
    memset(slots, 0, size_t(IOC_PILE_INS_SLOTS) * rows);
    q = r = 0;
    int64_t j = 0;  // the index of an 'I' in its run
    for (int64_t a = 0; a < len; ++a) {
        const char op = ops[a];
        if (op == 'I') {
            if (j < IOC_PILE_INS_SLOTS) slots[size_t(j) * rows + size_t(r)] = uint8_t(1u + PileAcc::channel(uint8_t(query[q])));
            ++j, ++q;
            continue;
        }
        j = 0;
        q += op == '=' || op == 'X' || op == 'i';
        r += op == '=' || op == 'X' || op == 'D' || op == 'd';
    }
    return IOC_OK;
}

// One read's planes ADDED to the two tables of its reference (isonclust2_hip.h has the rules) — the definition k_plane_pile
// (ioc_plane_pile.hip) is tested against.  Both tables are checked before either is touched.
int ioc_host_planes_pile(const uint8_t* base, const uint8_t* slots, int32_t rlen, ioc_pileup_col* cols, ioc_pileup_ins* ins)
{
    if (rlen < 0 || !base || !slots || !cols || !ins) return IOC_ERR_ARG;
    const size_t rows = size_t(rlen) + 1;
    for (size_t r = 0; r < rows; ++r)
        if (base[r] > IOC_ALLELE_DEL && base[r] != IOC_ALLELE_NONE) return IOC_ERR_ARG;
    for (size_t x = 0; x < size_t(IOC_PILE_INS_SLOTS) * rows; ++x)
        if (slots[x] > 5) return IOC_ERR_ARG;
    for (size_t r = 0; r < rows; ++r) {
        uint32_t* const word = reinterpret_cast<uint32_t*>(&cols[r]);  // (a c g t other del: the record's first six words, PILE_A .. PILE_DEL)
        if (base[r] != IOC_ALLELE_NONE) word[base[r]] += 1;
        for (size_t j = 0; j < size_t(IOC_PILE_INS_SLOTS); ++j) {
            const uint8_t s = slots[j * rows + r];
            if (s == 0) continue;
            ins[r].slot[j][s - 1] += 1;
            cols[r].ins_bases += 1;
            if (j == 0) cols[r].ins_runs += 1;
        }
    }
    return IOC_OK;
}

// The weight part of a read's projection (isonclust2_hip.h has the rules): the weight of every vote of the read, a byte per
// (plane, row) — the definition k_ops_project_weights (ioc_group_pile_weighted.hip) is tested against.  The walk, the weights and
// the refusals of ioc_host_ops_pileup_weighted.
int ioc_host_ops_project_weights(const char* ops, int64_t len, const char* query, const char* qual, int32_t qlen, int32_t rlen, uint8_t* wbase, uint8_t* wslots)
{
    if (len < 0 || len > INT32_MAX || (len > 0 && !ops) || qlen < 0 || rlen < 0 || (qlen > 0 && (!query || !qual)) || !wbase || !wslots) return IOC_ERR_ARG;
    int64_t q = 0, r = 0;
    for (int64_t a = 0; a < len; ++a) {
        const char op = ops[a];
        if (!strchr("=XIDid", op) || op == 0) return IOC_ERR_ARG;
        q += op == '=' || op == 'X' || op == 'I' || op == 'i';
        r += op == '=' || op == 'X' || op == 'D' || op == 'd';
    }
    if (q != qlen || r != rlen) return IOC_ERR_ARG;
    const size_t rows = size_t(rlen) + 1;
    memset(wbase, 0, rows);
    memset(wslots, 0, size_t(IOC_PILE_INS_SLOTS) * rows);
    q = r = 0;
    int64_t j = 0;  // the index of an 'I' in its run
    for (int64_t a = 0; a < len; ++a) {
        const char op = ops[a];
        if (op == 'I') {
            if (j < IOC_PILE_INS_SLOTS) wslots[size_t(j) * rows + size_t(r)] = uint8_t(pile_qual_weight(uint8_t(qual[q])));
            ++j, ++q;
            continue;
        }
        j = 0;
        switch (op) {
        case 'd': ++r; break;
        case 'i': ++q; break;
        case 'D': {
            const uint32_t wa = q > 0 ? pile_qual_weight(uint8_t(qual[q - 1])) : 0u, wb = q < qlen ? pile_qual_weight(uint8_t(qual[q])) : 0u;
            wbase[r++] = uint8_t(wa == 0u ? (wb == 0u ? 1u : wb) : wb == 0u ? wa : std::min(wa, wb));
            break;
        }
        default: wbase[r++] = uint8_t(pile_qual_weight(uint8_t(qual[q++]))); break;  // ('=' 'X')
        }
    }
    return IOC_OK;
}

// One read's planes and weight planes ADDED to the two tables of weights of its reference (isonclust2_hip.h has the rules) — the
// definition k_group_pile_weighted (ioc_group_pile_weighted.hip) is tested against.  The planes are checked before either table
// is touched.
int ioc_host_planes_pile_weighted(const uint8_t* base, const uint8_t* slots, const uint8_t* wbase, const uint8_t* wslots, int32_t rlen, ioc_pileup_col* wcols,
                                  ioc_pileup_ins* wins)
{
    if (rlen < 0 || !base || !slots || !wbase || !wslots || !wcols || !wins) return IOC_ERR_ARG;
    const size_t rows = size_t(rlen) + 1;
    for (size_t r = 0; r < rows; ++r)
        if (base[r] > IOC_ALLELE_DEL && base[r] != IOC_ALLELE_NONE) return IOC_ERR_ARG;
    for (size_t x = 0; x < size_t(IOC_PILE_INS_SLOTS) * rows; ++x)
        if (slots[x] > 5) return IOC_ERR_ARG;
    for (size_t r = 0; r < rows; ++r) {
        uint32_t* const word = reinterpret_cast<uint32_t*>(&wcols[r]);  // (a c g t other del: the record's first six words, PILE_A .. PILE_DEL)
        if (base[r] != IOC_ALLELE_NONE) word[base[r]] += wbase[r];
        for (size_t j = 0; j < size_t(IOC_PILE_INS_SLOTS); ++j) {
            const uint8_t s = slots[j * rows + r];
            if (s != 0) wins[r].slot[j][s - 1] += wslots[j * rows + r];
        }
    }
    return IOC_OK;
}

// The sites of one reference from its table of counts (isonclust2_hip.h has the rules; pile_sites_row, ioc_pile_sites.h, decides a
// row for this function and for the kernels of ioc_pile_sites.hip alike).
int64_t ioc_host_pileup_sites(const ioc_pileup_col* cols, int32_t rlen, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_sites,
                              ioc_pile_site* out, int64_t* n_found)
{
    if (min_depth < 1 || min_alt < 1 || min_pct < 1 || min_pct > 50 || max_sites < 1 || rlen < 0 || !cols || !out) return IOC_ERR_ARG;
    const PileSiteRule rule{min_depth, min_alt, min_pct};
    int64_t found = 0, written = 0;
    for (int32_t p = 0; p <= rlen; ++p) {
        const unsigned long long d_ins = p < rlen ? pile_depth(cols[p]) : rlen > 0 ? pile_depth(cols[rlen - 1]) : 0ull;
        const PileRowSites row = pile_sites_row(cols[p], d_ins, p < rlen, p, rule);
        if (row.has_ins && found++ < max_sites) out[written++] = row.ins;
        if (row.has_base && found++ < max_sites) out[written++] = row.base;
    }
    if (n_found) *n_found = found;
    return written;
}

// The alleles of one read, given by its projection, at the sites of its reference (pile_site_allele, ioc_pile_sites.h, as
// k_site_alleles has it).
int ioc_host_site_alleles(const uint8_t* base, const uint8_t* insf, int32_t rlen, const ioc_pile_site* sites, int32_t n_sites, uint8_t* out)
{
    if (rlen < 0 || n_sites < 0 || !base || !insf || (n_sites > 0 && (!sites || !out))) return IOC_ERR_ARG;
    for (int32_t s = 0; s < n_sites; ++s) {
        const ioc_pile_site& t = sites[s];
        if (t.row < 0 || t.row > rlen || (t.kind != IOC_SITE_BASE && t.kind != IOC_SITE_INS) || (t.kind == IOC_SITE_BASE && t.row == rlen)) return IOC_ERR_ARG;
    }
    const uint8_t b_last = rlen > 0 ? base[rlen - 1] : uint8_t(IOC_ALLELE_NONE);
    for (int32_t s = 0; s < n_sites; ++s) out[s] = pile_site_allele(sites[s].kind, sites[s].row == rlen, base[sites[s].row], insf[sites[s].row], b_last);
    return IOC_OK;
}

// The split of one segment's reads by its linked sites (isonclust2_hip.h has the rules; the mark, the phase and the group rule are
// ioc_site_split.h's, as the kernels of ioc_site_split.hip have them).  The plain triple loop: sites x sites x reads.
int ioc_host_alleles_split(const ioc_pile_site* sites, int32_t n_sites, const uint8_t* alleles, int32_t n_reads, int32_t min_link, int32_t min_margin,
                           int32_t rounds, int64_t* out_link, int8_t* out_phase, uint8_t* out_group, int32_t* out_vote, ioc_split_seg* out_seg)
{
    if (min_link < 1 || min_margin < 1 || rounds < 0 || rounds > 64 || n_sites < 0 || n_reads < 0 || !out_seg || (n_reads > 0 && !out_group) ||
        (n_sites > 0 && !sites) || (n_sites > 0 && n_reads > 0 && !alleles))
        return IOC_ERR_ARG;
    const size_t ns = size_t(n_sites), nr = size_t(n_reads);
    auto m = [&](size_t i, size_t s) { return split_mark(alleles[i * ns + s], sites[s].minor, sites[s].major); };
    auto d = [&](size_t s, size_t t) {
        int64_t v = 0;
        for (size_t i = 0; i < nr; ++i) v += int64_t(m(i, s) * m(i, t));
        return v;
    };
    std::vector<int64_t> link(ns, 0);
    std::vector<int8_t> phase(ns, 0);
    std::vector<int32_t> vote(nr, 0);
    std::vector<uint8_t> group(nr, uint8_t(IOC_SPLIT_NONE));
    int32_t seed = -1;
    for (size_t s = 0; s < ns; ++s) {
        for (size_t t = 0; t < ns; ++t) {
            const int64_t v = t != s ? std::llabs(d(s, t)) : 0;
            if (v >= min_link) link[s] += v;
        }
        if (link[s] > (seed < 0 ? 0 : link[size_t(seed)])) seed = int32_t(s);  // (the first of the largest; a largest of 0 is none)
    }
    auto cast_votes = [&]() {
        for (size_t i = 0; i < nr; ++i) {
            int64_t v = 0;
            for (size_t t = 0; t < ns; ++t) v += int64_t(phase[t]) * m(i, t);
            vote[i] = int32_t(v);
            group[i] = split_group(v, min_margin);
        }
    };
    if (seed >= 0) {
        for (size_t t = 0; t < ns; ++t) phase[t] = t == size_t(seed) ? int8_t(1) : split_phase(d(size_t(seed), t), min_link);
        cast_votes();
        for (int32_t r = 0; r < rounds; ++r) {
            for (size_t t = 0; t < ns; ++t) {
                int64_t dg = 0;
                for (size_t i = 0; i < nr; ++i) dg += (group[i] == 1 ? 1 : group[i] == 0 ? -1 : 0) * m(i, t);
                phase[t] = split_phase(dg, min_link);
            }
            cast_votes();
        }
    }
    ioc_split_seg rec{seed, 0, n_reads, 0, 0, 0, seed >= 0 ? link[size_t(seed)] : 0};
    for (size_t t = 0; t < ns; ++t) rec.n_linked += phase[t] != 0;
    for (size_t i = 0; i < nr; ++i) (group[i] == 1 ? rec.n_group1 : group[i] == 0 ? rec.n_group0 : rec.n_none) += 1;
    for (size_t t = 0; t < ns; ++t) {
        if (out_link) out_link[t] = link[t];
        if (out_phase) out_phase[t] = phase[t];
    }
    for (size_t i = 0; i < nr; ++i) {
        out_group[i] = group[i];
        if (out_vote) out_vote[i] = vote[i];
    }
    *out_seg = rec;
    return IOC_OK;
}

// The rows of a read decided and the guard's verdict on each, the runs of "fill" and of "remove" measured end to end: for
// ioc_host_read_correct and for ioc_host_read_correct_long.
static void host_read_decide(const uint8_t* base, int32_t rlen, const ioc_pileup_col* cols, const char* frame, const ReadRule& rule, std::vector<uint32_t>& dec,
                             std::vector<uint8_t>& guarded)
{
    const size_t rows = size_t(rlen) + 1;
    dec.assign(rows, uint32_t(READ_NONE)), guarded.assign(rows, 0);
    for (int32_t p = 0; p < rlen; ++p) dec[size_t(p)] = read_base_decide(cols[p], base[p], uint8_t(frame[p]), rule);
    for (size_t a = 0; a < size_t(rlen);) {
        const uint32_t kind = read_kind(dec[a]);
        size_t b = a + 1;
        if (kind == READ_FILL || kind == READ_REMOVE) {
            while (b < size_t(rlen) && read_kind(dec[b]) == kind) ++b;
            if (b - a > size_t(rule.max_run)) std::fill(guarded.begin() + int64_t(a), guarded.begin() + int64_t(b), uint8_t(1));
        }
        a = b;
    }
}

// One read corrected against the tables of its reference (isonclust2_hip.h has the rules; read_base_decide and read_correct_row,
// ioc_read_correct.h, decide and form a row for this function and for k_read_correct alike).  The plain loop: the rows are decided,
// the runs of "fill" and of "remove" are measured end to end (host_read_decide) — k_read_correct and tools/read_correct_check.cpp do
// the same with read_run_exceeds over masks of 64 rows — and the rows are written.
int64_t ioc_host_read_correct(const uint8_t* base, const uint8_t* slots, int32_t rlen, const ioc_pileup_col* cols, const ioc_pileup_ins* ins,
                              const char* frame, int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_run, char* out_seq, char* out_qual,
                              int64_t cap, ioc_correct_stats* st)
{
    const ReadRule rule{min_depth, min_alt, min_pct, max_run};
    if (!rule.ok() || rlen < 0 || !base || !slots || !cols || !ins || (rlen > 0 && !frame)) return IOC_ERR_ARG;
    const int64_t bound = int64_t(rlen) + int64_t(IOC_PILE_INS_SLOTS) * (int64_t(rlen) + 1);
    if (cap < bound) return IOC_ERR_CAPACITY;
    if (!out_seq || !out_qual) return IOC_ERR_ARG;
    const size_t rows = size_t(rlen) + 1;
    std::vector<uint32_t> dec;
    std::vector<uint8_t> guarded;
    host_read_decide(base, rlen, cols, frame, rule, dec, guarded);
    ioc_correct_stats s{};
    int64_t at = 0;
    for (int32_t p = 0; p <= rlen; ++p) {
        const int32_t pi = p < rlen ? p : rlen - 1;  // the row the insertions in front of p are held against, and the span's
        const unsigned long long D = pi >= 0 ? pile_depth(cols[pi]) : 0ull;
        const bool spans = pi >= 0 && read_covers(base[pi]);
        unsigned long long own_slots = 0;
        for (size_t j = 0; j < size_t(IOC_PILE_INS_SLOTS); ++j) own_slots |= (unsigned long long)slots[j * rows + size_t(p)] << (8u * j);
        const ReadRowOut row = read_correct_row(cols[p], ins[p], D, spans, base[p], own_slots, dec[size_t(p)], guarded[size_t(p)] != 0, rule);
        for (uint32_t x = 0; x < row.n; ++x) {
            out_seq[at] = char((row.seq >> (8u * x)) & 0xFFu);
            out_qual[at++] = char((row.qual >> (8u * x)) & 0xFFu);
        }
        s.n_sub += int32_t(row.n_sub), s.n_fill += int32_t(row.n_fill), s.n_remove += int32_t(row.n_remove), s.n_ins_add += int32_t(row.n_ins_add);
        s.n_ins_drop += int32_t(row.n_ins_drop), s.n_low += int32_t(row.n_low), s.n_guarded += int32_t(row.n_guarded);
    }
    s.out_len = int32_t(at);
    if (st) *st = s;
    return at;
}

// One read corrected against the tables of its isoform, a long insertion carried through (isonclust2_hip.h has the rules;
// iso_correct_row, ioc_iso_correct.h, forms a row for this function and for the kernels of ioc_iso_correct.hip alike).  The loop of
// ioc_host_read_correct, in two passes as the kernels make them: the rows are formed and counted — an unresolved pair ends there —
// and then written.
int64_t ioc_host_read_correct_long(const uint8_t* base, const uint8_t* slots, const uint8_t* ilen, const uint32_t* qpos, int32_t rlen, const ioc_pileup_col* cols,
                                   const ioc_pileup_ins* ins, const char* frame, const char* query, int32_t qlen, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                                   int32_t max_run, char* out_seq, char* out_qual, int64_t cap, ioc_iso_correct_stats* st)
{
    const ReadRule rule{min_depth, min_alt, min_pct, max_run};
    if (!rule.ok() || rlen < 0 || qlen < 0 || !base || !slots || !ilen || !qpos || !cols || !ins || (rlen > 0 && !frame) || (qlen > 0 && !query)) return IOC_ERR_ARG;
    const int64_t bound = int64_t(rlen) + int64_t(IOC_PILE_INS_SLOTS) * (int64_t(rlen) + 1) + qlen;
    if (cap < bound) return IOC_ERR_CAPACITY;
    if (!out_seq || !out_qual) return IOC_ERR_ARG;
    const size_t rows = size_t(rlen) + 1;
    std::vector<uint32_t> dec;
    std::vector<uint8_t> guarded;
    host_read_decide(base, rlen, cols, frame, rule, dec, guarded);
    std::vector<IsoRowOut> made(rows);
    ioc_iso_correct_stats s{};
    bool unresolved = false;
    int64_t long_bases = 0;
    for (int32_t p = 0; p <= rlen; ++p) {
        const int32_t pi = p < rlen ? p : rlen - 1;  // (as ioc_host_read_correct: the row the insertions in front of p are held against)
        const unsigned long long D = pi >= 0 ? pile_depth(cols[pi]) : 0ull;
        const bool spans = pi >= 0 && read_covers(base[pi]);
        unsigned long long own_slots = 0;
        for (size_t j = 0; j < size_t(IOC_PILE_INS_SLOTS); ++j) own_slots |= (unsigned long long)slots[j * rows + size_t(p)] << (8u * j);
        const IsoRowOut& m = made[size_t(p)] = iso_correct_row(cols[p], ins[p], D, spans, base[p], own_slots, ilen[p], qpos[p], uint32_t(qlen), dec[size_t(p)],
                                                              guarded[size_t(p)] != 0, rule);
        unresolved = unresolved || m.unresolved;
        s.out_len += int32_t(m.bytes());
        s.n_sub += int32_t(m.row.n_sub), s.n_fill += int32_t(m.row.n_fill), s.n_remove += int32_t(m.row.n_remove), s.n_ins_add += int32_t(m.row.n_ins_add);
        s.n_ins_drop += int32_t(m.row.n_ins_drop), s.n_low += int32_t(m.row.n_low), s.n_guarded += int32_t(m.row.n_guarded);
        s.n_long_runs += m.long_len > 0, long_bases += m.long_len;
    }
    s.n_long_bases = int32_t(std::min<int64_t>(long_bases, INT32_MAX));
    if (unresolved || long_bases > qlen) {  // (runs that together are longer than the read overlap: not this read's planes, and past the bound)
        s = ioc_iso_correct_stats{};
        s.flags = IOC_ISOC_UNRESOLVED;
        if (st) *st = s;
        return 0;
    }
    int64_t at = 0;
    for (const IsoRowOut& m : made) {
        for (uint32_t x = 0; x < m.long_len; ++x) out_seq[at] = query[m.long_from + x], out_qual[at++] = '!';
        for (uint32_t x = 0; x < m.row.n; ++x) {
            out_seq[at] = char((m.row.seq >> (8u * x)) & 0xFFu);
            out_qual[at++] = char((m.row.qual >> (8u * x)) & 0xFFu);
        }
    }
    if (st) *st = s;
    return at;
}

// The exon blocks of one segment and every read's isoform (isonclust2_hip.h has the rules; blocks_row_variable, blocks_state and
// blocks_key_agrees, ioc_read_blocks.h, decide for this function and for the kernels of ioc_read_blocks.hip alike).  The plain
// loops: every read's long gaps, the row table, the runs of variable rows, a state per read and kept block, and the supported keys
// in ascending unsigned order.
int ioc_host_planes_blocks(const uint8_t* base, int32_t n_reads, int32_t rlen, int32_t min_gap, int32_t min_depth, int32_t min_alt, int32_t min_pct,
                           int32_t min_block, int32_t max_blocks, ioc_block_row* out_rows, ioc_pile_block* out_blocks, ioc_read_blocks* out_reads,
                           ioc_blocks_seg* out_seg)
{
    const BlocksRule rule{min_gap, min_depth, min_alt, min_pct, min_block, max_blocks};
    if (!rule.ok() || n_reads < 0 || rlen < 0 || !out_seg || (n_reads > 0 && (!base || !out_reads)) || (rlen > 0 && !out_blocks)) return IOC_ERR_ARG;
    const size_t rows = size_t(rlen) + 1, n = size_t(n_reads);
    std::vector<ioc_block_row> table(rows, ioc_block_row{0, 0});
    std::vector<ioc_read_blocks> reads(n, ioc_read_blocks{});
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* b = base + i * rows;
        ioc_read_blocks& rd = reads[i];
        for (int32_t p = 0; p < rlen; ++p)
            if (blocks_covers(b[p])) {
                ++table[size_t(p)].depth;
                if (rd.end_row == 0) rd.first_row = p;
                rd.end_row = p + 1;
            }
        for (int32_t a = 0; a < rlen;) {
            int32_t e = a + 1;
            if (b[a] == uint8_t(IOC_ALLELE_DEL)) {
                while (e < rlen && b[e] == uint8_t(IOC_ALLELE_DEL)) ++e;
                if (e - a >= min_gap) {
                    ++rd.n_gaps, rd.gap_rows += e - a;
                    for (int32_t p = a; p < e; ++p) ++table[size_t(p)].in_gap;
                }
            }
            a = e;
        }
    }
    std::vector<ioc_pile_block> blocks;
    int32_t n_found = 0;
    for (int32_t a = 0; a < rlen;) {
        int32_t e = a + 1;
        if (blocks_row_variable(rule, table[size_t(a)].depth, table[size_t(a)].in_gap)) {
            while (e < rlen && blocks_row_variable(rule, table[size_t(e)].depth, table[size_t(e)].in_gap)) ++e;
            if (e - a >= min_block) {
                if (n_found < max_blocks) blocks.push_back(ioc_pile_block{a, e, 0, 0, 0, 0, {0, 0}});
                ++n_found;
            }
        }
        a = e;
    }
    const uint32_t nb = uint32_t(blocks.size());
    const unsigned long long full = blocks_full_mask(nb);
    std::vector<unsigned long long> mask(n, 0);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* b = base + i * rows;
        for (uint32_t k = 0; k < nb; ++k) {
            uint32_t c = 0, s = 0;
            for (int32_t p = blocks[k].first; p < blocks[k].end; ++p) c += blocks_covers(b[p]), s += b[p] == uint8_t(IOC_ALLELE_DEL);
            const uint32_t st = blocks_state(uint32_t(blocks[k].end - blocks[k].first), c, s);
            reads[i].key |= uint64_t(st) << (2u * k);
            mask[i] |= blocks_state_mask(k, st);
            ++(st == IOC_BLOCK_KEEP ? blocks[k].n_keep : st == IOC_BLOCK_SKIP ? blocks[k].n_skip : st == IOC_BLOCK_PART ? blocks[k].n_part : blocks[k].n_none);
        }
    }
    std::vector<uint64_t> complete, keys;  // the keys of the complete reads, sorted; the supported ones, ascending and unsigned
    for (size_t i = 0; i < n; ++i)
        if (mask[i] == full) complete.push_back(reads[i].key);
    std::sort(complete.begin(), complete.end());
    for (size_t a = 0; a < complete.size();) {
        size_t e = a;
        while (e < complete.size() && complete[e] == complete[a]) ++e;
        if (e - a >= size_t(min_alt)) keys.push_back(complete[a]);
        a = e;
    }
    ioc_blocks_seg seg{int32_t(nb), n_found, int32_t(keys.size()), n_reads, 0, 0, 0, 0};
    for (size_t i = 0; i < n; ++i) {
        ioc_read_blocks& rd = reads[i];
        rd.group = -1;
        if (mask[i] == full) {
            const auto it = std::lower_bound(keys.begin(), keys.end(), rd.key);
            if (it != keys.end() && *it == rd.key)
                rd.group = int32_t(it - keys.begin()), rd.how = IOC_ISO_DIRECT, ++seg.n_direct;
            else
                rd.how = IOC_ISO_RARE, ++seg.n_rare;
            continue;
        }
        int32_t agreeing = 0, which = -1;
        for (size_t k = 0; k < keys.size() && mask[i] != 0ull; ++k)
            if (blocks_key_agrees(rd.key, keys[k], mask[i])) ++agreeing, which = int32_t(k);
        if (agreeing == 1)
            rd.group = which, rd.how = IOC_ISO_ASSIGNED, ++seg.n_assigned;
        else
            rd.how = IOC_ISO_AMBIGUOUS, ++seg.n_ambiguous;
    }
    if (out_rows) std::copy(table.begin(), table.end(), out_rows);
    std::copy(blocks.begin(), blocks.end(), out_blocks);
    std::copy(reads.begin(), reads.end(), out_reads);
    *out_seg = seg;
    return IOC_OK;
}

// The length part of a read's projection (isonclust2_hip.h has the rules): how many bases the read inserts in front of every row,
// a byte each — the definition k_ops_project_ilen (ioc_read_inserts.hip) is tested against.  The walk of ioc_host_ops_project.
int ioc_host_ops_project_ilen(const char* ops, int64_t len, int32_t rlen, uint8_t* ilen)
{
    if (len < 0 || len > INT32_MAX || (len > 0 && !ops) || rlen < 0 || !ilen) return IOC_ERR_ARG;
    int64_t r = 0;
    for (int64_t a = 0; a < len; ++a) {
        const char op = ops[a];
        if (!strchr("=XIDid", op) || op == 0) return IOC_ERR_ARG;
        r += op == '=' || op == 'X' || op == 'D' || op == 'd';
    }
    if (r != rlen) return IOC_ERR_ARG;
    memset(ilen, 0, size_t(rlen) + 1);
    r = 0;
    for (int64_t a = 0; a < len;) {
        int64_t e = a + 1;
        if (ops[a] == 'I') {
            while (e < len && ops[e] == 'I') ++e;
            ilen[r] = inserts_len_byte((unsigned long long)(e - a));
        } else {
            r += ops[a] != 'i';
        }
        a = e;
    }
    return IOC_OK;
}

// The isoforms of a segment's reads from two-word keys (isonclust2_hip.h has the rules: step 9 of ioc_host_planes_inserts, which
// ioc_host_insert_window_variants takes again over key2): the supported pairs of words in ascending unsigned order, and every
// read's group and how it came to it.  pre_key NULL: the major word, its mask and pre_full are 0.
namespace {
struct KeyCounts { int32_t n_groups, n_direct, n_assigned, n_rare, n_ambiguous; };
KeyCounts host_key_isoforms(const uint64_t* pre_key, const uint64_t* pre_mask, uint64_t pre_full, const uint64_t* key, const uint64_t* mask, uint64_t full, size_t n,
                            int32_t min_alt, int32_t* group, int32_t* how)
{
    if (!pre_key) pre_full = 0;
    auto pk = [&](size_t i) { return pre_key ? pre_key[i] : uint64_t(0); };
    auto pm = [&](size_t i) { return pre_key ? pre_mask[i] : uint64_t(0); };
    typedef std::pair<uint64_t, uint64_t> Key;  // (the block stage's word, this stage's: compared in that order, unsigned)
    std::vector<Key> complete, keys;
    auto is_complete = [&](size_t i) { return mask[i] == full && pm(i) == pre_full; };
    for (size_t i = 0; i < n; ++i)
        if (is_complete(i)) complete.push_back(Key(pk(i), key[i]));
    std::sort(complete.begin(), complete.end());
    for (size_t a = 0; a < complete.size();) {
        size_t e = a;
        while (e < complete.size() && complete[e] == complete[a]) ++e;
        if (e - a >= size_t(min_alt)) keys.push_back(complete[a]);
        a = e;
    }
    KeyCounts kc{int32_t(keys.size()), 0, 0, 0, 0};
    for (size_t i = 0; i < n; ++i) {
        group[i] = -1, how[i] = 0;
        if (is_complete(i)) {
            const auto it = std::lower_bound(keys.begin(), keys.end(), Key(pk(i), key[i]));
            if (it != keys.end() && *it == Key(pk(i), key[i]))
                group[i] = int32_t(it - keys.begin()), how[i] = IOC_ISO_DIRECT, ++kc.n_direct;
            else
                how[i] = IOC_ISO_RARE, ++kc.n_rare;
            continue;
        }
        int32_t agreeing = 0, which = -1;
        for (size_t k = 0; k < keys.size() && (mask[i] | pm(i)) != 0ull; ++k)
            if (inserts_key_agrees(pk(i), key[i], keys[k].first, keys[k].second, pm(i), mask[i])) ++agreeing, which = int32_t(k);
        if (agreeing == 1)
            group[i] = which, how[i] = IOC_ISO_ASSIGNED, ++kc.n_assigned;
        else
            how[i] = IOC_ISO_AMBIGUOUS, ++kc.n_ambiguous;
    }
    return kc;
}
}  // namespace

int ioc_host_key_isoforms(const uint64_t* pre_key, const uint64_t* pre_mask, uint64_t pre_full, const uint64_t* key, const uint64_t* mask, uint64_t full,
                          int32_t n_reads, int32_t min_alt, int32_t* out_group, int32_t* out_how, int32_t* out_counts)
{
    if (n_reads < 0 || min_alt < 1 || !out_counts || (n_reads > 0 && (!key || !mask || !out_group || !out_how)) || (n_reads > 0 && !pre_key != !pre_mask)) return IOC_ERR_ARG;
    const KeyCounts kc = host_key_isoforms(pre_key, pre_mask, pre_full, key, mask, full, size_t(n_reads), min_alt, out_group, out_how);
    out_counts[0] = kc.n_groups, out_counts[1] = kc.n_direct, out_counts[2] = kc.n_assigned, out_counts[3] = kc.n_rare, out_counts[4] = kc.n_ambiguous;
    return IOC_OK;
}

// The insertion sites of one segment and every read's combined isoform (isonclust2_hip.h has the rules; InsertsRule::variable,
// inserts_state, inserts_key_agrees and inserts_key_less, ioc_read_inserts.h, decide for this function and for the kernels of
// ioc_read_inserts.hip alike).  The plain loops: every read's spans and windowed sums, the row table, the runs of variable
// junctions, a state per read and kept site, and the supported pairs of words in ascending unsigned order.
int ioc_host_planes_inserts(const uint8_t* base, const uint8_t* ilen, int32_t n_reads, int32_t rlen, int32_t min_ins, int32_t slack, int32_t min_depth,
                            int32_t min_alt, int32_t min_pct, int32_t max_sites, const uint64_t* pre_key, const uint64_t* pre_mask, uint64_t pre_full,
                            ioc_insert_row* out_rows, ioc_pile_insert* out_sites, ioc_read_inserts* out_reads, ioc_inserts_seg* out_seg)
{
    const InsertsRule rule{min_ins, slack, min_depth, min_alt, min_pct, max_sites};
    if (!rule.ok() || n_reads < 0 || rlen < 0 || !out_seg || (n_reads > 0 && (!base || !ilen || !out_reads)) || (rlen > 1 && !out_sites) ||
        (n_reads > 0 && !pre_key != !pre_mask))
        return IOC_ERR_ARG;
    const size_t rows = size_t(rlen) + 1, n = size_t(n_reads);
    if (!pre_key) pre_full = 0;
    auto spans = [&](size_t i, int32_t p) { return p >= 1 && p <= rlen - 1 && blocks_covers(base[i * rows + size_t(p) - 1]) && blocks_covers(base[i * rows + size_t(p)]); };
    auto window = [&](size_t i, int32_t p) {
        uint32_t w = 0;
        for (long long q = inserts_win_lo(p, slack); q <= inserts_win_hi(p, slack, rlen); ++q) w += ilen[i * rows + size_t(q)];
        return w;
    };
    auto near = [&](size_t i, int32_t p) { return spans(i, p) && window(i, p) >= uint32_t(min_ins); };
    std::vector<ioc_insert_row> table(rows, ioc_insert_row{0, 0});
    std::vector<ioc_read_inserts> reads(n, ioc_read_inserts{});
    for (size_t i = 0; i < n; ++i)
        for (int32_t p = 1; p <= rlen - 1; ++p) {
            if (!spans(i, p)) continue;
            ++table[size_t(p)].span, reads[i].ins_bases += ilen[i * rows + size_t(p)];
            if (near(i, p)) ++table[size_t(p)].in_ins, ++reads[i].n_near;
        }
    std::vector<ioc_pile_insert> sites;
    int32_t n_found = 0;
    for (int32_t a = 1; a <= rlen - 1;) {
        int32_t e = a + 1;
        if (rule.variable(table[size_t(a)].span, table[size_t(a)].in_ins)) {
            while (e <= rlen - 1 && rule.variable(table[size_t(e)].span, table[size_t(e)].in_ins)) ++e;
            if (n_found < max_sites) sites.push_back(ioc_pile_insert{a, e, 0, 0, 0, 0, 0, 0});
            ++n_found;
        }
        a = e;
    }
    const uint32_t ns = uint32_t(sites.size());
    const unsigned long long full = blocks_full_mask(ns);
    std::vector<unsigned long long> mask(n, 0);
    for (size_t i = 0; i < n; ++i)
        for (uint32_t k = 0; k < ns; ++k) {
            ioc_pile_insert& t = sites[k];
            uint32_t c = 0, s = 0, longest = 0;
            for (int32_t p = t.first; p < t.end; ++p) c += spans(i, p), s += near(i, p), longest = std::max(longest, window(i, p));
            const uint32_t st = inserts_state(uint32_t(t.end - t.first), c, s);
            reads[i].key |= uint64_t(st) << (2u * k);
            mask[i] |= blocks_state_mask(k, st);
            ++(st == IOC_INS_CARRY ? t.n_carry : st == IOC_INS_LACK ? t.n_lack : t.n_none);
            if (st == IOC_INS_CARRY) t.len_min = t.n_carry == 1u ? longest : std::min(t.len_min, longest), t.len_max = std::max(t.len_max, longest);
        }
    std::vector<uint64_t> key(n), msk(mask.begin(), mask.end());
    std::vector<int32_t> group(n), how(n);
    for (size_t i = 0; i < n; ++i) key[i] = reads[i].key;
    const KeyCounts kc = host_key_isoforms(pre_key, pre_mask, pre_full, key.data(), msk.data(), full, n, min_alt, group.data(), how.data());
    for (size_t i = 0; i < n; ++i) reads[i].group = group[i], reads[i].how = how[i];
    const ioc_inserts_seg seg{int32_t(ns), n_found, kc.n_groups, n_reads, kc.n_direct, kc.n_assigned, kc.n_rare, kc.n_ambiguous};
    if (out_rows) std::copy(table.begin(), table.end(), out_rows);
    std::copy(sites.begin(), sites.end(), out_sites);
    std::copy(reads.begin(), reads.end(), out_reads);
    *out_seg = seg;
    return IOC_OK;
}

// The position part of a read's projection (isonclust2_hip.h has the rules): where every row lies in the read, a 32-bit word each —
// the definition k_ops_project_qpos (ioc_insert_windows.hip) is tested against.  The walk of ioc_host_ops_project_ilen.
int ioc_host_ops_project_qpos(const char* ops, int64_t len, int32_t rlen, uint32_t* qpos)
{
    if (len < 0 || len > INT32_MAX || (len > 0 && !ops) || rlen < 0 || !qpos) return IOC_ERR_ARG;
    int64_t r = 0;
    for (int64_t a = 0; a < len; ++a) {
        const char op = ops[a];
        if (!strchr("=XIDid", op) || op == 0) return IOC_ERR_ARG;
        r += op == '=' || op == 'X' || op == 'D' || op == 'd';
    }
    if (r != rlen) return IOC_ERR_ARG;
    std::fill(qpos, qpos + size_t(rlen) + 1, 0u);
    uint32_t q = 0;
    r = 0;
    for (int64_t a = 0; a < len; ++a) {
        const char op = ops[a];
        q += op == '=' || op == 'X' || op == 'I' || op == 'i';
        if (op == '=' || op == 'X' || op == 'D' || op == 'd') qpos[++r] = q;
    }
    return IOC_OK;
}

// The global alignment of two short strings with linear gaps (isonclust2_hip.h has the rules; win_dir and win_max3,
// ioc_insert_windows.h, decide for this function and for k_win_align alike): the whole matrix, then the walk.
int64_t ioc_host_align_global_ops(const char* query, int32_t qlen, const char* ref, int32_t rlen, int32_t match, int32_t mismatch, int32_t gap, char* ops,
                                  int64_t cap, int32_t* out_score)
{
    if (qlen < 0 || rlen < 0 || !WinRule::score_ok(match, mismatch, gap) || (qlen > 0 && !query) || (rlen > 0 && !ref) || cap < 0 || (cap > 0 && !ops))
        return IOC_ERR_ARG;
    if (cap < int64_t(qlen) + rlen || (int64_t(qlen) + 1) * (int64_t(rlen) + 1) > (int64_t(1) << 26)) return IOC_ERR_CAPACITY;
    const size_t W = size_t(rlen) + 1;
    std::vector<int32_t> H((size_t(qlen) + 1) * W);
    for (size_t j = 0; j < W; ++j) H[j] = -int32_t(j) * gap;
    for (int32_t i = 1; i <= qlen; ++i) {
        H[size_t(i) * W] = -i * gap;
        for (int32_t j = 1; j <= rlen; ++j)
            H[size_t(i) * W + size_t(j)] = win_max3(H[size_t(i - 1) * W + size_t(j - 1)] + (query[i - 1] == ref[j - 1] ? match : mismatch),
                                                    H[size_t(i) * W + size_t(j - 1)] - gap, H[size_t(i - 1) * W + size_t(j)] - gap);
    }
    std::string back;
    for (int32_t i = qlen, j = rlen; i > 0 || j > 0;) {
        uint32_t d = i == 0 ? uint32_t(WIN_D) : uint32_t(WIN_I);
        if (i > 0 && j > 0)
            d = win_dir(H[size_t(i - 1) * W + size_t(j - 1)] + (query[i - 1] == ref[j - 1] ? match : mismatch), H[size_t(i) * W + size_t(j - 1)] - gap,
                        H[size_t(i - 1) * W + size_t(j)] - gap);
        if (d == WIN_DIAG)
            back.push_back(query[i - 1] == ref[j - 1] ? '=' : 'X'), --i, --j;
        else if (d == WIN_D)
            back.push_back('D'), --j;
        else
            back.push_back('I'), --i;
    }
    std::copy(back.rbegin(), back.rend(), ops);
    if (out_score) *out_score = H[size_t(qlen) * W + size_t(rlen)];
    return int64_t(back.size());
}

// The windows of one segment's carriers at its kept sites (isonclust2_hip.h has the rules; win_lo, win_hi, win_class, win_voter_less
// and win_median_rank, ioc_insert_windows.h, decide for this function and for the kernels of ioc_insert_windows.hip alike).
int ioc_host_insert_windows(const uint8_t* base, const uint32_t* qpos, const int32_t* qlen, int32_t n_reads, int32_t rlen, const ioc_pile_insert* sites,
                            int32_t n_sites, const uint64_t* keys, int32_t slack, int32_t max_win, ioc_insert_window* out_win, uint8_t* out_class,
                            uint32_t* out_start, uint32_t* out_len)
{
    const WinRule rule{slack, max_win, 0, 0, 0};
    if (!rule.bounds_ok() || n_reads < 0 || rlen < 0 || n_sites < 0 || n_sites > IOC_INSERTS_MAX || (n_sites > 0 && (!sites || !out_win)) ||
        (n_reads > 0 && n_sites > 0 && (!base || !qpos || !qlen || !keys)) || !out_start != !out_len)
        return IOC_ERR_ARG;
    for (int32_t k = 0; k < n_sites; ++k)
        if (!win_site_ok(sites[k].first, sites[k].end, rlen)) return IOC_ERR_ARG;
    for (int32_t i = 0; i < n_reads && n_sites > 0; ++i)
        if (qlen[i] < 0) return IOC_ERR_ARG;
    const size_t rows = size_t(rlen) + 1, n = size_t(n_reads), S = size_t(n_sites);
    for (size_t k = 0; k < S; ++k) {
        const long long lo = win_lo(sites[k].first, slack), hi = win_hi(sites[k].end, slack, rlen);
        ioc_insert_window w{int32_t(lo), int32_t(hi), -1, 0, 0, 0, 0, 0};
        std::vector<std::pair<uint32_t, uint32_t>> voters;  // (window length, read)
        for (size_t i = 0; i < n; ++i) {
            uint32_t len = 0;
            const uint32_t cls = win_class(uint32_t(keys[i] >> (2 * k)) & 3u, base[i * rows + size_t(lo) - 1], base[i * rows + size_t(hi) - 1],
                                           qpos[i * rows + size_t(lo)], qpos[i * rows + size_t(hi)], uint32_t(qlen[i]), max_win, &len);
            w.n_voters += cls == IOC_WIN_VOTER, w.n_short += cls == IOC_WIN_SHORT, w.n_long += cls == IOC_WIN_LONG;
            if (cls == IOC_WIN_VOTER) voters.push_back({len, uint32_t(i)});
            if (out_class) out_class[i * S + k] = uint8_t(cls);
            if (out_start) out_start[i * S + k] = cls == IOC_WIN_VOTER ? qpos[i * rows + size_t(lo)] : 0u, out_len[i * S + k] = len;
        }
        if (!voters.empty()) {
            std::sort(voters.begin(), voters.end(), [](const auto& a, const auto& b) { return win_voter_less(a.first, a.second, b.first, b.second); });
            const auto& t = voters[win_median_rank(uint32_t(voters.size()))];
            w.template_pair = int32_t(t.second), w.tlen = int32_t(t.first);
        }
        out_win[k] = w;
    }
    return IOC_OK;
}

// The agreement of an alignment (isonclust2_hip.h has the rule; winvar_agreement, ioc_window_variants.h, decides for this function
// and for k_win_agree alike).
int ioc_host_ops_agreement(const char* ops, int64_t len, int32_t* out)
{
    if (len < 0 || len > INT32_MAX || (len > 0 && !ops) || !out) return IOC_ERR_ARG;
    uint32_t eq = 0, x = 0, d = 0, in = 0;
    for (int64_t a = 0; a < len; ++a) {
        const char op = ops[a];
        if (!strchr("=XIDid", op) || op == 0) return IOC_ERR_ARG;
        eq += op == '=', x += op == 'X', d += op == 'D', in += op == 'I';
    }
    *out = winvar_agreement(eq, x, d, in);
    return IOC_OK;
}

// The variants of one segment's kept sites (isonclust2_hip.h has the rules; winvar_near, winvar_round_b, winvar_splits,
// winvar_variant and winvar_state, ioc_window_variants.h, decide for this function and for the kernels of ioc_window_variants.hip
// alike).  The plain loops: the windows, round A, round B, the decision, a consensus per slot by the calls that exist, and key2.
int ioc_host_insert_window_variants(const uint8_t* base, const uint32_t* qpos, const int32_t* qlen, int32_t n_reads, int32_t rlen, const ioc_pile_insert* sites,
                                    int32_t n_sites, const uint64_t* keys, const char* reads, const int64_t* read_off, int32_t slack, int32_t max_win, int32_t match,
                                    int32_t mismatch, int32_t gap, int32_t polish_min_depth, int32_t min_agree, int32_t min_alt, int32_t min_pct,
                                    ioc_insert_window* out_win, ioc_window_variant* out_var, uint8_t* out_variant, int32_t* out_agree, char* out_seq, char* out_qual,
                                    int64_t cap, int64_t* out_off, ioc_polish_stats* out_stats, uint64_t* out_key2, uint64_t* out_mask2)
{
    const WinRule wrule{slack, max_win, match, mismatch, gap};
    const WinVarRule rule{min_agree, min_alt, min_pct};
    const bool live = n_reads > 0 && n_sites > 0, call = out_seq != nullptr;
    if (!wrule.ok() || !rule.ok() || polish_min_depth < 1 || n_reads < 0 || rlen < 0 || n_sites < 0 || n_sites > IOC_INSERTS_MAX || cap < 0 || !out_seq != !out_qual ||
        (call && (!out_off || (n_sites > 0 && !out_stats))) || (n_sites > 0 && (!sites || !out_win || !out_var)) ||
        (live && (!base || !qpos || !qlen || !out_variant || !reads || !read_off)) ||
        (n_reads > 0 && (!keys || !out_key2 || !out_mask2)))
        return IOC_ERR_ARG;
    for (int32_t i = 0; i < n_reads && live; ++i)
        if (qlen[i] < 0 || read_off[i + 1] - read_off[i] != int64_t(qlen[i])) return IOC_ERR_ARG;
    const size_t n = size_t(n_reads), S = size_t(n_sites);
    std::vector<ioc_insert_window> win(S);
    std::vector<uint8_t> cls(n * S);
    std::vector<uint32_t> start(n * S), len(n * S);
    if (const int st = ioc_host_insert_windows(base, qpos, qlen, n_reads, rlen, sites, n_sites, keys, slack, max_win, win.data(), cls.data(), start.data(), len.data()))
        return st;
    if (call && cap < 2 * int64_t(S) * pile_call_most(max_win)) return IOC_ERR_CAPACITY;

    std::vector<ioc_window_variant> var(S, ioc_window_variant{0, -1, 0, 0, 0, 0, 0, 0});
    std::vector<uint8_t> variant(n * S, uint8_t(IOC_WINVAR_NONE));
    std::vector<int32_t> agree(n * S * 2, INT32_MIN);
    std::vector<uint64_t> key2(n), mask2(n, 0);
    std::string seq, qual;
    std::vector<int64_t> off{0};
    std::vector<ioc_polish_stats> stats;
    auto window = [&](size_t i, size_t k) { return reads + read_off[i] + start[i * S + k]; };
    // one round at site k: every listed voter against the template t; the flag of each, and its alignment's bytes kept for the call
    std::vector<std::string> kept[2];
    auto round = [&](size_t k, const std::vector<size_t>& who, size_t t, int which, std::vector<uint8_t>& flag) {
        const int32_t tlen = int32_t(len[t * S + k]);
        kept[which].assign(n, std::string());
        for (const size_t i : who) {
            const int32_t ql = int32_t(len[i * S + k]);
            std::string& ops = kept[which][i];
            ops.assign(size_t(ql) + size_t(tlen), 0);
            const int64_t L = ioc_host_align_global_ops(window(i, k), ql, window(t, k), tlen, match, mismatch, gap, &ops[0], int64_t(ops.size()), nullptr);
            ops.resize(size_t(L));
            int32_t a = 0;
            ioc_host_ops_agreement(ops.data(), L, &a);
            agree[(i * S + k) * 2 + size_t(which)] = a;
            flag[i] = winvar_near(a, uint32_t(ql), uint32_t(tlen), min_agree) ? WINVAR_NEAR : WINVAR_FAR;
        }
    };
    // a slot's consensus: the voters listed, as round `which` aligned them to the template t, projected, piled and called
    auto consensus = [&](size_t k, const std::vector<size_t>& who, size_t t, int which) {
        const int32_t tlen = int32_t(len[t * S + k]);
        const size_t rows = size_t(tlen) + 1;
        std::vector<ioc_pileup_col> cols(rows, ioc_pileup_col{});
        std::vector<ioc_pileup_ins> ins(rows, ioc_pileup_ins{});
        std::vector<uint8_t> pb(rows), pf(rows), ps(size_t(IOC_PILE_INS_SLOTS) * rows);
        for (const size_t i : who) {
            const int32_t ql = int32_t(len[i * S + k]);
            const std::string& ops = kept[which][i];
            const int64_t L = int64_t(ops.size());
            ioc_host_ops_project(ops.data(), L, window(i, k), ql, tlen, pb.data(), pf.data());
            ioc_host_ops_project_ins(ops.data(), L, window(i, k), ql, tlen, ps.data());
            ioc_host_planes_pile(pb.data(), ps.data(), tlen, cols.data(), ins.data());
        }
        std::string s(size_t(pile_call_most(tlen)), 0), q(s.size(), 0);
        ioc_polish_stats st{};
        const int64_t L = ioc_host_pileup_call(cols.data(), ins.data(), window(t, k), tlen, polish_min_depth, &s[0], &q[0], int64_t(s.size()), &st);
        seq.append(s.data(), size_t(L)), qual.append(q.data(), size_t(L));
        off.push_back(int64_t(seq.size())), stats.push_back(st);
    };
    auto no_call = [&]() { off.push_back(int64_t(seq.size())), stats.push_back(ioc_polish_stats{}); };
    for (size_t i = 0; i < n; ++i) key2[i] = keys[i];
    for (size_t k = 0; k < S; ++k) {
        const ioc_insert_window& w = win[k];
        ioc_window_variant& v = var[k];
        std::vector<size_t> voters, far, va, vb;
        for (size_t i = 0; i < n; ++i)
            if (cls[i * S + k] == IOC_WIN_VOTER) voters.push_back(i);
        std::vector<uint8_t> fa(n, WINVAR_UNSEEN), fb(n, WINVAR_UNSEEN);
        if (w.tlen > 0) round(k, voters, size_t(w.template_pair), 0, fa);
        for (const size_t i : voters)
            if (fa[i] == WINVAR_FAR) far.push_back(i);
        v.n_far = uint32_t(far.size());
        if (winvar_round_b(rule, w.n_voters, v.n_far)) {
            std::vector<std::pair<uint32_t, uint32_t>> order;  // (window length, read)
            for (const size_t i : far) order.push_back({len[i * S + k], uint32_t(i)});
            std::sort(order.begin(), order.end(), [](const auto& a, const auto& b) { return win_voter_less(a.first, a.second, b.first, b.second); });
            const auto& t = order[win_median_rank(uint32_t(order.size()))];
            v.template_pair_b = int32_t(t.second), v.tlen_b = int32_t(t.first);
            round(k, far, size_t(t.second), 1, fb);
            for (const size_t i : far) ++(fb[i] == WINVAR_NEAR ? v.n_b : v.n_other);
        }
        v.split = winvar_splits(rule, w.n_voters, v.n_far, v.n_b) ? 1 : 0;
        for (size_t i = 0; i < n; ++i) {
            const uint8_t x = winvar_variant(cls[i * S + k], v.split != 0, fa[i], fb[i]);
            variant[i * S + k] = x;
            if (x == IOC_WINVAR_A) va.push_back(i);
            if (x == IOC_WINVAR_B) vb.push_back(i);
            const uint32_t st = winvar_state(uint32_t(keys[i] >> (2 * k)) & 3u, cls[i * S + k], v.split != 0, x);
            key2[i] = (key2[i] & ~(uint64_t(3) << (2 * k))) | uint64_t(st) << (2 * k);
        }
        v.n_a = uint32_t(va.size());
        if (!call) continue;
        if (w.tlen > 0) consensus(k, va, size_t(w.template_pair), 0); else no_call();
        if (v.split) consensus(k, vb, size_t(v.template_pair_b), 1); else no_call();
    }
    for (size_t i = 0; i < n; ++i) mask2[i] = blocks_key_mask(key2[i], uint32_t(S));
    if (call && int64_t(seq.size()) > cap) return IOC_ERR_CAPACITY;  // (the bound above holds it: pile_call_most a slot)
    std::copy(win.begin(), win.end(), out_win);
    std::copy(var.begin(), var.end(), out_var);
    if (out_variant) std::copy(variant.begin(), variant.end(), out_variant);
    if (out_agree) std::copy(agree.begin(), agree.end(), out_agree);
    if (call) {
        std::copy(seq.begin(), seq.end(), out_seq), std::copy(qual.begin(), qual.end(), out_qual);
        std::copy(off.begin(), off.end(), out_off), std::copy(stats.begin(), stats.end(), out_stats);
    }
    std::copy(key2.begin(), key2.end(), out_key2);
    std::copy(mask2.begin(), mask2.end(), out_mask2);
    return IOC_OK;
}

// The full-length sequence of one isoform: ioc_host_pileup_call's walk with the windows of the sites it carries in place of their
// rows (isonclust2_hip.h has the rules; splice_state and splice_row, ioc_iso_splice.h, decide for this function and for the kernels
// of ioc_iso_splice.hip alike).  The body both definitions share: site b carries iff carries[b], its template length is tlen[b] and
// its bytes are from[b] .. to[b] of seq / qual; the arguments are checked by then.
static int64_t isoform_splice_walk(const ioc_pileup_col* cols, const ioc_pileup_ins* ins, const char* frame, int32_t rlen, int32_t min_depth,
                                   const ioc_insert_window* win, int32_t n_sites, const uint8_t* carries, const int32_t* tlen, const int64_t* from, const int64_t* to,
                                   const char* win_seq, const char* win_qual, char* out_seq, char* out_qual, ioc_polish_stats* st, ioc_splice_site* out_sites,
                                   ioc_splice_stats* out_sstats)
{
    IocSpliceIv plan[IOC_SPLICE_PLAN_MAX];
    uint32_t n_plan = 0;
    ioc_splice_stats ss{};
    int32_t last_hi = 0;
    for (int32_t b = 0; b < n_sites; ++b) {
        const int32_t state = splice_state_of(carries[b] != 0, tlen[b], win[b].lo, last_hi);
        out_sites[b] = ioc_splice_site{state, -1, 0, 0};
        ss.n_uncalled += state == IOC_SPLICE_UNCALLED, ss.n_overlap += state == IOC_SPLICE_OVERLAP;
        if (state != IOC_SPLICE_DONE) continue;
        plan[n_plan++] = IocSpliceIv{win[b].lo, win[b].hi, int32_t(to[b] - from[b]), b, from[b]};
        last_hi = win[b].hi;
        ++ss.n_done, ss.rows_replaced += win[b].hi - win[b].lo, ss.spliced_bytes += int32_t(to[b] - from[b]);
    }
    ioc_polish_stats s{};
    int64_t at = 0;
    for (int32_t p = 0; p <= rlen; ++p) {
        const int32_t what = splice_row(plan, n_plan, p);
        if (what == IOC_SPLICE_ROW_GONE) continue;
        if (what >= 0) {
            const IocSpliceIv& iv = plan[what];
            out_sites[iv.site].at = int32_t(at), out_sites[iv.site].len = iv.len;
            for (int32_t x = 0; x < iv.len; ++x) out_seq[at] = win_seq[iv.off + x], out_qual[at++] = win_qual[iv.off + x];
            continue;
        }
        const unsigned long long d_ins = p < rlen ? pile_depth(cols[p]) : rlen > 0 ? pile_depth(cols[rlen - 1]) : 0ull;
        const PileRowCall row = pile_call_row(cols[p], ins[p], d_ins, p < rlen, p < rlen ? uint8_t(frame[p]) : uint8_t(0), min_depth);
        for (uint32_t x = 0; x < row.n; ++x) {
            out_seq[at] = char((row.seq >> (8u * x)) & 0xFFu);
            out_qual[at++] = char((row.qual >> (8u * x)) & 0xFFu);
        }
        s.n_ins += int32_t(row.n_ins), s.n_sub += int32_t(row.n_sub), s.n_del += int32_t(row.n_del), s.n_low += int32_t(row.n_low);
    }
    s.out_len = int32_t(at);
    if (st) *st = s;
    if (out_sstats) *out_sstats = ss;
    return at;
}

int64_t ioc_host_isoform_splice(const ioc_pileup_col* cols, const ioc_pileup_ins* ins, const char* frame, int32_t rlen, int32_t min_depth, uint64_t key,
                                const ioc_insert_window* win, int32_t n_sites, const char* win_seq, const char* win_qual, const int64_t* win_off,
                                char* out_seq, char* out_qual, int64_t cap, ioc_polish_stats* st, ioc_splice_site* out_sites, ioc_splice_stats* out_sstats)
{
    if (min_depth < 1 || rlen < 0 || !cols || !ins || (rlen > 0 && !frame) || n_sites < 0 || n_sites > IOC_INSERTS_MAX || !win_off ||
        (n_sites > 0 && (!win || !out_sites)))
        return IOC_ERR_ARG;
    for (int32_t b = 0; b < n_sites; ++b)
        if (win[b].lo < 1 || win[b].lo >= win[b].hi || win[b].hi > rlen || win[b].tlen < 0 || win_off[b + 1] < win_off[b] ||
            win_off[b + 1] - win_off[b] > INT32_MAX)
            return IOC_ERR_ARG;
    const int64_t win_bytes = win_off[n_sites] - win_off[0];
    if (win_bytes > 0 && (!win_seq || !win_qual)) return IOC_ERR_ARG;
    const int64_t bound = int64_t(rlen) + int64_t(IOC_PILE_INS_SLOTS) * (int64_t(rlen) + 1) + win_bytes;
    if (cap < bound) return IOC_ERR_CAPACITY;
    if (!out_seq || !out_qual) return IOC_ERR_ARG;
    uint8_t carries[IOC_INSERTS_MAX];
    int32_t tlen[IOC_INSERTS_MAX];
    for (int32_t b = 0; b < n_sites; ++b) carries[b] = ((key >> (2 * b)) & 3u) == uint64_t(IOC_INS_CARRY), tlen[b] = win[b].tlen;
    return isoform_splice_walk(cols, ins, frame, rlen, min_depth, win, n_sites, carries, tlen, win_off, win_off + 1, win_seq, win_qual, out_seq, out_qual, st, out_sites,
                               out_sstats);
}

// The same by variant: a site's state under key2 chooses one of its two slots (splice_variant_which and splice_variant_tlen,
// ioc_iso_splice.h, which the slot-aware plan kernel asks as well); everything behind that choice is the walk above.
int64_t ioc_host_isoform_splice_variants(const ioc_pileup_col* cols, const ioc_pileup_ins* ins, const char* frame, int32_t rlen, int32_t min_depth, uint64_t key,
                                         const ioc_insert_window* win, const ioc_window_variant* var, int32_t n_sites, const char* slot_seq, const char* slot_qual,
                                         const int64_t* slot_off, char* out_seq, char* out_qual, int64_t cap, ioc_polish_stats* st, ioc_splice_site* out_sites,
                                         ioc_splice_stats* out_sstats)
{
    if (min_depth < 1 || rlen < 0 || !cols || !ins || (rlen > 0 && !frame) || n_sites < 0 || n_sites > IOC_INSERTS_MAX || !slot_off ||
        (n_sites > 0 && (!win || !var || !out_sites)))
        return IOC_ERR_ARG;
    for (int32_t b = 0; b < n_sites; ++b) {
        if (win[b].lo < 1 || win[b].lo >= win[b].hi || win[b].hi > rlen || win[b].tlen < 0 || (var[b].split != 0 && var[b].split != 1) || var[b].tlen_b < 0)
            return IOC_ERR_ARG;
        for (int32_t y = 2 * b; y < 2 * b + 2; ++y)
            if (slot_off[y + 1] < slot_off[y] || slot_off[y + 1] - slot_off[y] > INT32_MAX) return IOC_ERR_ARG;
    }
    const int64_t slot_bytes = slot_off[2 * n_sites] - slot_off[0];
    if (slot_bytes > 0 && (!slot_seq || !slot_qual)) return IOC_ERR_ARG;
    const int64_t bound = int64_t(rlen) + int64_t(IOC_PILE_INS_SLOTS) * (int64_t(rlen) + 1) + slot_bytes;
    if (cap < bound) return IOC_ERR_CAPACITY;
    if (!out_seq || !out_qual) return IOC_ERR_ARG;
    uint8_t carries[IOC_INSERTS_MAX];
    int32_t tlen[IOC_INSERTS_MAX];
    int64_t from[IOC_INSERTS_MAX], to[IOC_INSERTS_MAX];
    for (int32_t b = 0; b < n_sites; ++b) {
        const int32_t which = splice_variant_which(uint32_t(key >> (2 * b)) & 3u);
        carries[b] = which >= 0, tlen[b] = which >= 0 ? splice_variant_tlen(which, win[b], var[b]) : 0;
        from[b] = slot_off[2 * b + std::max(which, 0)], to[b] = slot_off[2 * b + std::max(which, 0) + 1];
    }
    return isoform_splice_walk(cols, ins, frame, rlen, min_depth, win, n_sites, carries, tlen, from, to, slot_seq, slot_qual, out_seq, out_qual, st, out_sites, out_sstats);
}

// setGapOpen, src/cluster.cpp:425-440
int32_t ioc_host_gap_open(double e)
{
    if (e <= 0.01) return 5;
    if (e <= 0.04) return 4;
    if (e <= 0.1) return 3;
    return 2;
}

// the kernel family of a pair by its scoring parameters: aln_route (ioc_align_sink.h), which the GPU aligner's prepare_pairs asks too
int ioc_host_align_route(int32_t match, int32_t mismatch, int32_t gap_extend, int32_t gap_open)
{
    return aln_route(match, mismatch, gap_extend, gap_open);
}

// The extent of one read on its reference (isonclust2_hip.h has the rules): the rows its base plane covers — the bytes "=XD" of
// the walk of ioc_host_ops_project — and the 'i' bytes before the first and behind the last byte of "=XID", as ioc_host_ops_stats
// counts them.
int ioc_host_ops_extent(const char* ops, int64_t len, int32_t rlen, ioc_read_extent* out)
{
    if (len < 0 || len > INT32_MAX || (len > 0 && !ops) || rlen < 0 || !out) return IOC_ERR_ARG;
    int64_t r = 0, first = len, last = -1;  // the walk's first and last byte
    for (int64_t a = 0; a < len; ++a) {
        const char op = ops[a];
        if (!strchr("=XIDid", op) || op == 0) return IOC_ERR_ARG;
        r += op == '=' || op == 'X' || op == 'D' || op == 'd';
        if (op == 'i' || op == 'd') continue;
        if (first == len) first = a;
        last = a;
    }
    if (r != rlen) return IOC_ERR_ARG;
    ioc_read_extent e{0, 0, 0, 0};
    r = 0;
    for (int64_t a = 0; a < len; ++a) {
        const char op = ops[a];
        if (op == 'i') a < first ? ++e.head : a > last ? ++e.tail : 0;  // (a string without a walk byte: all leading)
        if (op == '=' || op == 'X' || op == 'D') {
            if (e.end_row == 0) e.first_row = int32_t(r);
            e.end_row = int32_t(r) + 1;
        }
        r += op != 'i' && op != 'I';
    }
    *out = e;
    return IOC_OK;
}

// The alternative ends of one segment (isonclust2_hip.h has the rules; EndsRule::row, ends_distance, ends_near_word and ends_key,
// ioc_read_ends.h, decide for this function and for the kernels of ioc_read_ends.hip alike).  The plain loops: the two histograms,
// their windowed sums, the runs of start and of stop rows, every read's nearest sites, the sites' counts and peaks, and the
// supported triples in ascending order.
int ioc_host_reads_ends(const ioc_read_extent* extents, const int32_t* pre_group, int32_t n_reads, int32_t rlen, int32_t slack, int32_t min_over,
                        int32_t min_depth, int32_t min_alt, int32_t min_pct, int32_t max_sites, int32_t max_variants, ioc_end_row* out_rows,
                        ioc_end_site* out_starts, ioc_end_site* out_stops, ioc_end_variant* out_variants, ioc_read_ends* out_reads, ioc_ends_seg* out_seg)
{
    const EndsRule rule{slack, min_over, min_depth, min_alt, min_pct, max_sites, max_variants};
    if (!rule.ok() || n_reads < 0 || rlen < 0 || !out_seg || !out_starts || !out_stops || (n_reads > 0 && (!extents || !out_reads || !out_variants)))
        return IOC_ERR_ARG;
    const size_t rows = size_t(rlen) + 1, n = size_t(n_reads);
    for (size_t i = 0; i < n; ++i)
        if (!ends_extent_ok(extents[i], rlen) || (pre_group && pre_group[i] < -1)) return IOC_ERR_ARG;
    auto pre = [&](size_t i) { return pre_group ? pre_group[i] : 0; };
    std::vector<ioc_end_row> table(rows, ioc_end_row{0, 0, 0, 0});
    uint32_t N = 0;
    for (size_t i = 0; i < n; ++i)
        if (ends_takes_part(extents[i])) ++N, ++table[size_t(extents[i].first_row)].starts, ++table[size_t(extents[i].end_row)].stops;
    for (int64_t p = 0; p <= rlen; ++p)
        for (int64_t q = std::max<int64_t>(p - slack, 0); q <= std::min<int64_t>(p + slack, rlen); ++q)
            table[size_t(p)].w_starts += table[size_t(q)].starts, table[size_t(p)].w_stops += table[size_t(q)].stops;
    std::vector<ioc_end_site> sites[2];
    int32_t n_found[2] = {0, 0};
    for (int kind = 0; kind < 2; ++kind) {
        auto is_row = [&](int64_t p) { return rule.row(N, kind ? table[size_t(p)].w_stops : table[size_t(p)].w_starts); };
        auto count = [&](int64_t p) { return kind ? table[size_t(p)].stops : table[size_t(p)].starts; };
        for (int64_t a = 0; a <= rlen;) {
            int64_t e = a + 1;
            if (is_row(a)) {
                while (e <= rlen && is_row(e)) ++e;
                if (n_found[kind] < max_sites) {
                    unsigned long long peak = 0;
                    for (int64_t p = a; p < e; ++p) peak = std::max(peak, ends_peak_word(count(p), uint32_t(rlen), uint32_t(p)));
                    sites[kind].push_back(ioc_end_site{int32_t(a), int32_t(e), 0, 0, ends_peak_row(peak, uint32_t(rlen)), ends_peak_count(peak), kind, 0});
                }
                ++n_found[kind];
            }
            a = e;
        }
    }
    std::vector<ioc_read_ends> reads(n, ioc_read_ends{-1, -1, -1, 0});
    std::vector<unsigned long long> placed;  // the keys of the placed reads, sorted; then the supported ones, ascending
    for (size_t i = 0; i < n; ++i) {
        const ioc_read_extent& x = extents[i];
        if (!ends_takes_part(x)) continue;
        for (int kind = 0; kind < 2; ++kind) {
            uint32_t best = ENDS_FAR;
            for (size_t b = 0; b < sites[kind].size(); ++b)
                best = std::min(best, ends_near_word(ends_distance(sites[kind][b].first, sites[kind][b].end, kind ? x.end_row : x.first_row), uint32_t(b), slack));
            const int32_t site = ends_near_site(best);
            (kind ? reads[i].stop_site : reads[i].start_site) = site;
            if (site >= 0) ++sites[kind][size_t(site)].n_reads, sites[kind][size_t(site)].n_over += (kind ? x.tail : x.head) >= min_over;
        }
        if (ends_placed(pre(i), reads[i].start_site, reads[i].stop_site)) placed.push_back(ends_key(pre(i), reads[i].start_site, reads[i].stop_site));
    }
    const size_t n_placed = placed.size();
    std::sort(placed.begin(), placed.end());
    std::vector<unsigned long long> keys;
    std::vector<ioc_end_variant> variants;
    int32_t variants_found = 0;
    for (size_t a = 0; a < placed.size();) {
        size_t e = a;
        while (e < placed.size() && placed[e] == placed[a]) ++e;
        if (e - a >= size_t(min_alt)) {
            if (variants_found < max_variants) {
                keys.push_back(placed[a]);
                variants.push_back(ioc_end_variant{int32_t(placed[a] >> 32), int32_t((placed[a] >> 8) & 0xFFu), int32_t(placed[a] & 0xFFu), uint32_t(e - a)});
            }
            ++variants_found;
        }
        a = e;
    }
    for (size_t i = 0; i < n; ++i) {
        if (!ends_placed(pre(i), reads[i].start_site, reads[i].stop_site)) continue;
        const auto it = std::lower_bound(keys.begin(), keys.end(), ends_key(pre(i), reads[i].start_site, reads[i].stop_site));
        if (it != keys.end() && *it == ends_key(pre(i), reads[i].start_site, reads[i].stop_site)) reads[i].variant = int32_t(it - keys.begin());
    }
    if (out_rows) std::copy(table.begin(), table.end(), out_rows);
    std::copy(sites[0].begin(), sites[0].end(), out_starts);
    std::copy(sites[1].begin(), sites[1].end(), out_stops);
    std::copy(variants.begin(), variants.end(), out_variants);
    std::copy(reads.begin(), reads.end(), out_reads);
    *out_seg = ioc_ends_seg{int32_t(N), int32_t(sites[0].size()), n_found[0], int32_t(sites[1].size()), n_found[1], int32_t(variants.size()), variants_found, int32_t(n_placed)};
    return IOC_OK;
}

// getAlnRatio, src/cluster.cpp:442-459
double ioc_host_aln_ratio(const char* comp, int32_t comp_len, double e, uint32_t slen, uint32_t k)
{
    if (!comp || comp_len < 0 || uint32_t(comp_len) < k || slen == 0) return 0.0;
    double aligned = 0;
    const double limit = std::floor((1.0 - e) * k);
    int nm = 0;
    for (uint32_t t = 0; t < k; ++t) nm += comp[t] == '|';
    // windows [i, i+k) for i = 0 .. len-k-1 (the reference's loop stops when j reaches end())
    for (int32_t i = 0; i + int32_t(k) < comp_len; ++i) {
        if (nm >= limit) aligned++;
        nm -= comp[i] == '|';
        nm += comp[i + int32_t(k)] == '|';
    }
    return aligned / slen;
}

}  // extern "C"
