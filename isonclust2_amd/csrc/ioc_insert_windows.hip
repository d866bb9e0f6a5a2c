// ioc_insert_windows.hip — the sequence of an inserted exon: the windows of the carriers at every kept insertion site, the template
// among them and every voter's alignment to it (ioc_planes_insert_windows, ioc_align_pairs_blocks_inserts_seq; the definitions are
// ioc_host_ops_project_qpos, ioc_host_insert_windows and ioc_host_align_global_ops, ioc_align.cpp).
//
//   k_ops_project_qpos  beside k_ops_project_ilen (ioc_read_inserts.hip), over the same bytes of a slice and of the same shape: one
//                       wave per pair walks its string with PileAcc.  The lane of a byte that consumes a reference row r stores, at
//                       row r + 1 of the pair's position plane, the query bytes up to and including its own.  A row is consumed by
//                       one byte: plain 32-bit stores, one writer per word, no atomics; row 0 keeps the caller's 0.
//   k_win_bounds        a wave per pair, a lane per kept site of its segment: the anchors, two words of the position plane and two
//                       bytes of the base plane where the pair carries, and the pair's class and window (win_class).
//   k_win_template      a wave per site over the segment's members, 64 at a time: the three counts by ballot, then every voter's
//                       rank as the number of voters with a smaller (length, pair) — the voters of a chunk are handed round the
//                       wave one by one, unsigned compares —, and the voter of rank (n - 1) / 2 is the template (win_lower_median,
//                       ioc_win_stage.h, which k_win_template_far of ioc_window_variants.hip ranks the far voters with).  Quadratic
//                       in a site's voters, as the block stage's rank kernels are.
//   k_win_align         a wave per (voter, site), one wave a workgroup.  The fill: a lane per template column in strips of 64, the
//                       rows skewed down the lanes (lane l is at row t - l + 1 in step t), the left neighbour's value by a shuffle
//                       and the diagonal kept from the step before; a strip's last column goes to the next strip through 513 words
//                       of LDS, in place (an entry is read 63 steps before it is written again).  The voter's window lies in LDS,
//                       512 bytes.  Two direction bits a cell, 16 rows to a word, a word per column and 16 rows in global memory.
//                       The walk back is serial and the same in every lane: the wave holds the words of 64 columns of the current
//                       16 rows (a 256-byte load), takes a cell's word with a shuffle and loads again where the walk leaves them.
//                       It writes the voter's base plane and slot planes in the template's frame as ioc_host_ops_project and
//                       ioc_host_ops_project_ins define them for the alignment's bytes: a row's base byte at the step that consumes
//                       the row, a run's first six bases where the run closes.  One writer per byte, no atomics.
// Every plane word and byte, table entry, record, pool byte and direction word is held against the sizes passed.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ioc_insert_windows.h"
#include "ioc_internal.h"
#include "ioc_ops_pileup.h"
#include "ioc_wave.h"
#include "ioc_win_stage.h"

namespace {

constexpr uint32_t WAVES = IOC_WIN_WAVES;
constexpr int OP_WAVES = 4;  // pairs per workgroup of k_ops_project_qpos (nothing is shared between them)
typedef unsigned long long u64;

__global__ void __launch_bounds__(64 * OP_WAVES)
k_ops_project_qpos(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ end, const uint32_t* __restrict__ len,
                   const uint32_t* __restrict__ room, const uint32_t* __restrict__ ord, uint32_t cnt, const int64_t* __restrict__ row_base,
                   const uint64_t* __restrict__ plane, uint32_t* __restrict__ qpos_planes, uint64_t plane_rows)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t x = blockIdx.x * OP_WAVES + (threadIdx.x >> 6);
    if (x >= cnt) return;  // (whole waves: there is no barrier below)
    const uint32_t pid = ord[x];
    const uint64_t L = len[pid], e = end[pid];
    if (L == 0 || L > room[pid] || L > e) return;  // came back without an answer: left to its re-run (as k_ops_project has it)
    if (row_base[pid] < 0) return;                 // (piled and projected by an earlier run of this call already)
    const uint64_t po = plane[pid];

    const uint8_t* first = buf + (e - L);
    const uint32_t head = uint32_t(reinterpret_cast<uintptr_t>(first) & 3u);
    const uint32_t* words = reinterpret_cast<const uint32_t*>(first - head);
    const uint32_t span = head + uint32_t(L);
    const uint32_t nwords = (span + 3u) / 4u, nchunks = (nwords + 63u) / 64u;

    PileAcc acc;
    uint32_t w = lane < nwords ? words[lane] : 0u;
    for (uint32_t c = 0; c < nchunks; ++c) {
        const uint32_t nx = (c + 1u) * 64u + lane;
        const uint32_t w_next = nx < nwords ? words[nx] : 0u;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t pos = c * 256u + j * 64u + lane;
            const uint32_t v = uint32_t(__shfl(int(w), int(16u * j + (lane >> 2)), 64));
            const uint32_t b = (pos >= head && pos < span) ? (v >> (8u * (lane & 3u))) & 0xFFu : 0u;
            acc.begin(__ballot(b == uint32_t('=')), __ballot(b == uint32_t('X')), __ballot(b == uint32_t('I')), __ballot(b == uint32_t('D')),
                      __ballot(b == uint32_t('i')), __ballot(b == uint32_t('d')));
            if ((acc.m_ref >> lane) & 1ull) {  // the byte that consumes row acc.row(lane): the query bytes up to and including it
                const uint64_t at_row = po + acc.row(lane) + 1u;
                if (at_row < plane_rows) qpos_planes[at_row] = acc.qpos(lane) + uint32_t((acc.m_qry >> lane) & 1ull);
            }
            acc.end();
        }
        w = w_next;
    }
}

__global__ void __launch_bounds__(64 * WAVES)
k_win_bounds(IocWinDev v, int32_t slack, int32_t max_win)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;  // (the entry points refuse such a pair)
    const long long rlen = v.segs[g].rlen;
    const u64 sb = u64(v.site_off[g]), se = u64(v.site_off[g + 1u]);
    const u64 x = sb + lane;
    if (x >= se || x >= v.n_sites || lane >= uint32_t(IOC_INSERTS_MAX) || lane >= v.stride) return;  // (no ballot or shuffle below)
    const long long first = v.sites[x].first, end = v.sites[x].end;
    uint32_t cls = IOC_WIN_NONE, start = 0, len = 0;
    const uint32_t state = uint32_t(v.keys[i] >> (2u * lane)) & 3u;
    if (win_site_ok(first, end, rlen) && state == uint32_t(IOC_INS_CARRY)) {
        const u64 po = v.plane[i], lo = u64(win_lo(first, slack)), hi = u64(win_hi(end, slack, rlen));
        uint8_t b_lo = uint8_t(IOC_ALLELE_NONE), b_hi = uint8_t(IOC_ALLELE_NONE);
        uint32_t q_lo = 0, q_hi = 0;
        if (po + hi < v.plane_rows) b_lo = v.base_planes[po + lo - 1u], b_hi = v.base_planes[po + hi - 1u], q_lo = v.qpos_planes[po + lo], q_hi = v.qpos_planes[po + hi];
        cls = win_class(state, b_lo, b_hi, q_lo, q_hi, v.qlen[i], max_win, &len);
        if (cls == uint32_t(IOC_WIN_VOTER)) start = q_lo;
    }
    const u64 at = u64(i) * v.stride + lane;
    if (at < v.n_slots) v.slots[at] = IocWinSlot{start, win_slot_pack(cls, len)};
}

__global__ void __launch_bounds__(64 * WAVES)
k_win_template(IocWinDev v, int32_t slack)
{
    const uint32_t lane = threadIdx.x & 63u;
    const u64 x = u64(blockIdx.x) * WAVES + (threadIdx.x >> 6);
    if (x >= v.n_sites) return;
    const uint32_t g = uint32_t(v.site_seg[x]);
    if (g >= v.n_segs) return;
    const u64 k64 = x - u64(v.site_off[g]);
    if (k64 >= u64(IOC_INSERTS_MAX) || k64 >= v.stride) return;
    const uint32_t k = uint32_t(k64);
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u];
    // what lane holds of member m: its pair, and its class and length at the site
    auto member = [&](uint32_t m, uint32_t& pair) -> uint32_t {
        pair = 0xFFFFFFFFu;
        if (m >= me) return 0u;
        pair = v.members[m];
        const u64 at = u64(pair) * v.stride + k;
        return pair < v.n_pairs && at < v.n_slots ? v.slots[at].cls_len : 0u;
    };
    uint32_t n_voters = 0, n_short = 0, n_long = 0;
    for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
        uint32_t pair;
        const uint32_t cl = win_slot_class(member(m0 + lane, pair));
        n_voters += uint32_t(__popcll(__ballot(cl == uint32_t(IOC_WIN_VOTER))));
        n_short += uint32_t(__popcll(__ballot(cl == uint32_t(IOC_WIN_SHORT))));
        n_long += uint32_t(__popcll(__ballot(cl == uint32_t(IOC_WIN_LONG))));
    }
    const WinMedian t = win_lower_median(mb, me, n_voters, [&](uint32_t m, uint32_t& pair, uint32_t& len) {
        const uint32_t cl = member(m, pair);
        len = win_slot_len(cl);
        return win_slot_class(cl) == uint32_t(IOC_WIN_VOTER);
    });
    const int32_t t_pair = t.pair, t_len = t.len;
    if (lane == 0) {
        const long long first = v.sites[x].first, end = v.sites[x].end, rlen = v.segs[g].rlen;
        const bool ok = win_site_ok(first, end, rlen);
        v.win[x] = ioc_insert_window{ok ? int32_t(win_lo(first, slack)) : 0, ok ? int32_t(win_hi(end, slack, rlen)) : 0, t_pair, t_len, n_voters, n_short, n_long, 0u};
    }
}

enum : int { WIN_PHASE_BOTH = 0, WIN_PHASE_FILL = 1, WIN_PHASE_WALK = 2 };

__global__ void __launch_bounds__(64)
k_win_align(const IocWinItem* __restrict__ items, uint32_t n_items, const uint8_t* __restrict__ pool, uint64_t pool_bytes, uint8_t* __restrict__ base_planes,
            uint8_t* __restrict__ slot_planes, uint64_t plane_bytes, uint32_t* __restrict__ dir, uint64_t n_dir_words, int32_t match, int32_t mismatch,
            int32_t gap, int phase)
{
    __shared__ uint8_t qs[IOC_WIN_MAX];
    __shared__ int32_t edge[IOC_WIN_MAX + 1];
    if (blockIdx.x >= n_items) return;  // (whole workgroups, a wave each)
    const IocWinItem it = items[blockIdx.x];
    const uint32_t lane = threadIdx.x, qlen = it.qlen, tlen = it.tlen;
    if (qlen < 1u || qlen > uint32_t(IOC_WIN_MAX) || tlen < 1u || tlen > uint32_t(IOC_WIN_MAX)) return;
    if (it.q_off + qlen > pool_bytes || it.t_off + tlen > pool_bytes) return;
    if (it.dir + win_dir_words(qlen, tlen) > n_dir_words || it.plane + tlen + 1u > plane_bytes) return;
    uint32_t* const words = dir + it.dir;

    for (uint32_t a = lane; a < qlen; a += 64u) qs[a] = pool[it.q_off + a];
    for (uint32_t a = lane; a <= qlen; a += 64u) edge[a] = -int32_t(a) * gap;  // H[a][0]
    __syncthreads();

    for (uint32_t j0 = 0; j0 < tlen && phase != WIN_PHASE_WALK; j0 += 64u) {
        const uint32_t j = j0 + lane + 1u, ncols = min(64u, tlen - j0);
        const bool col = j <= tlen;
        const uint32_t tb = col ? pool[it.t_off + j - 1u] : 0u;
        int32_t h = -int32_t(j) * gap, diag = -int32_t(j - 1u) * gap;  // H[0][j], H[0][j - 1]
        uint32_t word = 0;
        for (uint32_t t = 0; t + 1u < qlen + ncols; ++t) {
            int32_t left = __shfl_up(h, 1, 64);  // lane - 1's value of the step before: H[i][j - 1]
            const uint32_t i = t + 1u - lane;    // (wraps below row 1: not active then)
            const bool active = col && t >= lane && i <= qlen;
            if (active) {
                if (lane == 0u) left = edge[i];
                const int32_t dg = diag + (uint32_t(qs[i - 1u]) == tb ? match : mismatch), d = left - gap, in = h - gap;
                word |= win_dir(dg, d, in) << win_dir_shift(i);
                diag = left, h = win_max3(dg, d, in);
                if (lane == 63u) edge[i] = h;  // H[i][j0 + 64], the next strip's left edge
                if (i % uint32_t(IOC_WIN_ROWS_PER_WORD) == 0u || i == qlen) {
                    words[win_dir_word(i, j, tlen)] = word;  // (inside the item's block: i <= qlen, j <= tlen)
                    word = 0;
                }
            }
        }
        __syncthreads();  // (a wave: the strip's edge and direction words are written before the next strip and the walk read them)
    }
    if (phase == WIN_PHASE_FILL) return;

    // the walk back, the same in every lane: (i, j) the cell, run the 'I's met since the last byte that was none — they stand in
    // front of row j and begin at query base i
    uint32_t i = qlen, j = tlen, run = 0;
    uint32_t held = 0, held_rb = 0xFFFFFFFFu, held_top = 0;  // lane l: the word of column held_top - l of the 16 rows held_rb
    auto close_run = [&]() {
        if (lane < run && lane < uint32_t(IOC_PILE_INS_SLOTS) && i + lane < qlen)
            slot_planes[u64(lane) * plane_bytes + it.plane + j] = uint8_t(1u + PileAcc::channel(qs[i + lane]));
        run = 0;
    };
    while (i > 0u || j > 0u) {
        uint32_t d = i == 0u ? uint32_t(WIN_D) : uint32_t(WIN_I);
        if (i > 0u && j > 0u) {
            const uint32_t rb = (i - 1u) / uint32_t(IOC_WIN_ROWS_PER_WORD);
            if (rb != held_rb || j > held_top || j + 63u < held_top) {
                held_rb = rb, held_top = j;
                held = lane < j ? words[u64(rb) * tlen + (j - lane - 1u)] : 0u;
            }
            d = (shfl32(held, held_top - j) >> win_dir_shift(i)) & 3u;
        }
        if (d != uint32_t(WIN_DIAG) && d != uint32_t(WIN_D)) {  // 'I'
            ++run, --i;
            continue;
        }
        close_run();
        if (lane == 0u) base_planes[it.plane + j - 1u] = d == uint32_t(WIN_DIAG) ? uint8_t(PileAcc::channel(qs[i - 1u])) : uint8_t(IOC_ALLELE_DEL);
        if (d == uint32_t(WIN_DIAG)) --i;
        --j;
    }
    close_run();
}

}  // namespace

static_assert(sizeof(ioc_insert_window) == 32 && sizeof(IocWinSlot) == 8 && sizeof(IocWinItem) == 40, "the records are laid out as the host lays them out");

// The bytes of a slice's operation strings in [buf, ..): pair pid's position plane is qpos_planes + plane[pid] .. + its reference
// length, set to 0 by the caller.  The arguments of iock_ops_project_ilen.
hipError_t iock_ops_project_qpos(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room, const uint32_t* ord,
                                 uint32_t cnt, const int64_t* row_base, const uint64_t* plane, uint32_t* qpos_planes, uint64_t plane_rows)
{
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ops_project_qpos, dim3((cnt + OP_WAVES - 1) / OP_WAVES), dim3(64 * OP_WAVES), 0, st, buf, end, len, room, ord, cnt, row_base, plane,
                       qpos_planes, plane_rows);
    return hipGetLastError();
}

hipError_t iock_win_bounds_template(hipStream_t st, const IocWinDev& v, int32_t slack, int32_t max_win, hipEvent_t* each)
{
    auto grid = [](uint64_t items) { return dim3(uint32_t((items + WAVES - 1u) / WAVES)); };
    int step = 0;
    auto mark = [&]() { if (each) (void)hipEventRecord(each[step++], st); };
    mark();
    if (v.n_pairs && v.n_sites) hipLaunchKernelGGL(k_win_bounds, grid(v.n_pairs), dim3(64 * WAVES), 0, st, v, slack, max_win);
    mark();
    if (v.n_sites) hipLaunchKernelGGL(k_win_template, grid(v.n_sites), dim3(64 * WAVES), 0, st, v, slack);
    mark();
    return hipGetLastError();
}

hipError_t iock_win_align(hipStream_t st, const IocWinItem* items, uint32_t n_items, const uint8_t* pool, uint64_t pool_bytes, uint8_t* base_planes,
                          uint8_t* slot_planes, uint64_t plane_bytes, uint32_t* dir, uint64_t n_dir_words, int32_t match, int32_t mismatch, int32_t gap,
                          int phase)
{
    if (n_items == 0) return hipSuccess;
    hipLaunchKernelGGL(k_win_align, dim3(n_items), dim3(64), 0, st, items, n_items, pool, pool_bytes, base_planes, slot_planes, plane_bytes, dir, n_dir_words, match,
                       mismatch, gap, phase);
    return hipGetLastError();
}
