// ioc_insert_windows.h — the sequence of an inserted exon (ioc_host_insert_windows, ioc_host_align_global_ops, isonclust2_hip.h):
// the small decisions shared between the definitions on the host (ioc_align.cpp) and the kernels of ioc_insert_windows.hip — what
// a call refuses, a site's anchors, a read's class at a site, the order of two voters, the direction of a cell and where its two
// bits lie.  tools/insert_windows_check.cpp drives these on the CPU under the sanitizers, lane by lane as the kernels do; the tests
// hold the definitions against restatements in Python.
#pragma once

#include <cstdint>

#include "isonclust2_hip.h"
#include "ioc_read_inserts.h"

#define IOC_WIN_WAVES 4            // waves per workgroup of k_win_bounds and k_win_template, an item each
#define IOC_WIN_PARAM_MOST (1 << 20)  // |match|, |mismatch| and gap of a window alignment: 1024 steps of it stay inside 2^30
#define IOC_WIN_ROWS_PER_WORD 16   // two direction bits a cell: the rows of a column that share a 32-bit word

struct WinRule {  // what a window call is run with, and what it refuses
    int32_t slack, max_win, match, mismatch, gap;
    IOC_PILE_HD bool bounds_ok() const { return slack >= 0 && slack <= IOC_INS_SLACK_MAX && max_win >= 1 && max_win <= IOC_WIN_MAX; }
    static IOC_PILE_HD bool score_ok(int32_t match, int32_t mismatch, int32_t gap)
    {
        return gap >= 0 && gap <= IOC_WIN_PARAM_MOST && match >= -IOC_WIN_PARAM_MOST && match <= IOC_WIN_PARAM_MOST && mismatch >= -IOC_WIN_PARAM_MOST &&
               mismatch <= IOC_WIN_PARAM_MOST;
    }
    IOC_PILE_HD bool ok() const { return bounds_ok() && score_ok(match, mismatch, gap); }
};

// a kept site of a segment of rlen rows that a window can be cut at
IOC_PILE_HD bool win_site_ok(long long first, long long end, long long rlen) { return first >= 1 && first < end && end <= rlen; }
// the anchors of a site: the window rows are [lo, hi)
IOC_PILE_HD long long win_lo(long long first, int32_t slack) { return first - slack > 1 ? first - slack : 1; }
IOC_PILE_HD long long win_hi(long long end, int32_t slack, long long rlen) { return end + slack < rlen ? end + slack : rlen; }

// A read's class at a site: its state there, the bytes of its base plane at rows lo - 1 and hi - 1, the words of its position plane
// at lo and hi, its read's length.  *len: the window's length where the class is IOC_WIN_VOTER.
IOC_PILE_HD uint32_t win_class(uint32_t state, uint8_t b_lo, uint8_t b_hi, uint32_t q_lo, uint32_t q_hi, uint32_t qlen, int32_t max_win, uint32_t* len)
{
    *len = 0;
    if (state != uint32_t(IOC_INS_CARRY)) return IOC_WIN_NONE;
    if (!blocks_covers(b_lo) || !blocks_covers(b_hi)) return IOC_WIN_SHORT;
    if (q_hi < q_lo || q_hi > qlen || q_hi - q_lo < 1u || q_hi - q_lo > uint32_t(max_win)) return IOC_WIN_LONG;
    *len = q_hi - q_lo;
    return IOC_WIN_VOTER;
}
// the order of the voters of a site: (window length, index), ascending
IOC_PILE_HD bool win_voter_less(uint32_t a_len, uint32_t a_idx, uint32_t b_len, uint32_t b_idx) { return a_len < b_len || (a_len == b_len && a_idx < b_idx); }
IOC_PILE_HD uint32_t win_median_rank(uint32_t n_voters) { return (n_voters - 1u) / 2u; }  // (n_voters >= 1)

// The direction of cell (i, j), 1 <= i, 1 <= j, from the three candidates: the diagonal first, then 'D', then 'I'.
enum : uint32_t { WIN_DIAG = 0, WIN_D = 1, WIN_I = 2 };
IOC_PILE_HD int32_t win_max3(int32_t dg, int32_t d, int32_t in) { return dg >= d ? (dg >= in ? dg : in) : (d >= in ? d : in); }
IOC_PILE_HD uint32_t win_dir(int32_t dg, int32_t d, int32_t in)
{
    const int32_t best = win_max3(dg, d, in);
    return dg == best ? WIN_DIAG : d == best ? WIN_D : WIN_I;
}
// where the two bits of cell (i, j) lie in an alignment's block of direction words: tlen columns, ceil(qlen / 16) words each
IOC_PILE_HD uint64_t win_dir_words(uint32_t qlen, uint32_t tlen) { return uint64_t((qlen + IOC_WIN_ROWS_PER_WORD - 1u) / IOC_WIN_ROWS_PER_WORD) * tlen; }
IOC_PILE_HD uint64_t win_dir_word(uint32_t i, uint32_t j, uint32_t tlen) { return uint64_t((i - 1u) / IOC_WIN_ROWS_PER_WORD) * tlen + (j - 1u); }
IOC_PILE_HD uint32_t win_dir_shift(uint32_t i) { return 2u * ((i - 1u) % IOC_WIN_ROWS_PER_WORD); }

// One alignment of k_win_align: a voter's window against its site's template, both where they lie in the pool; the voter's planes
// in the template's frame are tlen + 1 bytes from `plane` on, its direction words win_dir_words(qlen, tlen) from `dir` on.
struct IocWinItem {
    uint64_t q_off, t_off, plane, dir;
    uint32_t qlen, tlen;
};
// a (pair, site) entry of k_win_bounds' table: where the pair's window begins in its read, and its class and length
struct IocWinSlot {
    uint32_t start, cls_len;  // cls_len: class << 30 | min(length, 2^30 - 1)
};
IOC_PILE_HD uint32_t win_slot_pack(uint32_t cls, uint32_t len) { return cls << 30 | (len < (1u << 30) ? len : (1u << 30) - 1u); }
IOC_PILE_HD uint32_t win_slot_class(uint32_t cls_len) { return cls_len >> 30; }
IOC_PILE_HD uint32_t win_slot_len(uint32_t cls_len) { return cls_len & ((1u << 30) - 1u); }
