// ioc_iso_splice.hip — the full-length sequence of every isoform: the consensus call of a group-segment's tables with the windows of
// the insertion sites it carries spliced in, where tables and windows lie (ioc_planes_isoforms_full; the definition is
// ioc_host_isoform_splice, ioc_align.cpp, and the row logic both share is ioc_iso_splice.h).
//
//   k_splice_plan       a wave per group-segment, a lane per kept site of its segment: the state of every site under the
//                       group-segment's key (splice_state; OVERLAP depends on the last DONE site, so the wave walks the sites in
//                       turn, a broadcast a site), the site records, the splice record and the plan — the DONE sites' intervals
//                       [lo, hi) with where their window's bytes lie, at most 32, ascending.
//   k_splice_plan<true>  the same over the variant stage's slots (ioc_host_isoform_splice_variants): the lane loads its variant record
//                       too and both ends of the slot its key2 state takes, 2 b for CARRY and 2 b + 1 for CARRY_B; the walk and what
//                       it writes are the same, so the call passes below serve both.
//   k_splice_call<false> the shape of k_pile_call: a workgroup per group-segment, chunks of IOC_PILE_CALL_CHUNK rows, a lane per
//                       row.  The plan sits in LDS; a row inside an interval counts nothing, the row lo of one counts its window's
//                       length (up to 7 IOC_WIN_MAX + 6 bytes, so the sums are 32-bit words all the way, never the 7 bytes a row
//                       has in k_pile_call), any other row is decided as always (pile_call_seg_row, ioc_pile_call.h).  seg_len[x] and the record.
//   (iock_pile_scan)    out_off = the exclusive scan of seg_len: the scan kernel of ioc_pile_call.hip.
//   k_splice_call<true> decides again and writes: the wave scan and the workgroup scan give every lane where its bytes begin; the
//                       lane of a row lo writes nothing itself, it notes the place in LDS and in the site's record (`at`), and once
//                       the rows are through the whole workgroup copies every window's bytes, strided.
//
// No atomics: every output byte has one writer and its place is a function of the tables and the plan.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ioc_internal.h"
#include "ioc_iso_splice.h"
#include "ioc_pile_call.h"
#include "ioc_wave.h"

namespace {

constexpr uint32_t CHUNK = IOC_PILE_CALL_CHUNK;  // rows per step of a workgroup = its threads
constexpr uint32_t WAVES = CHUNK / 64u;
constexpr uint32_t PLAN_MAX = IOC_SPLICE_PLAN_MAX;
static_assert(CHUNK % 64u == 0 && WAVES >= 1 && WAVES <= 16 && PLAN_MAX <= 64u && PLAN_MAX <= CHUNK, "whole waves, a lane per site");

// a wave per group-segment, a lane per site.  VARIANTS (ioc_planes_isoforms_full_variants): keys are key2, the lane loads its variant
// record as well, and win_off is the slots' — the lane's bytes are those of the slot its state takes.
template <bool VARIANTS>
__global__ void __launch_bounds__(CHUNK)
k_splice_plan(IocSpliceDev v)
{
    const uint32_t lane = threadIdx.x & 63u, x = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (x >= v.n_gsegs) return;  // (whole waves; no barrier below)
    const uint32_t g = uint32_t(v.gseg_seg[x]);
    const long long s0 = v.site_off[g];
    const long long ns_all = v.site_off[g + 1u] - s0;
    const uint32_t ns = ns_all < 0 ? 0u : ns_all > (long long)PLAN_MAX ? PLAN_MAX : uint32_t(ns_all);
    const unsigned long long key = v.keys[x];
    const bool mine = lane < ns && uint64_t(s0) + lane < v.n_sites;
    ioc_insert_window w{};
    ioc_window_variant wv{};
    long long off = 0, end = 0;
    if (VARIANTS) {
        if (mine) {  // (lane < 32: the shift stays inside the key; slot_off has 2 n_sites + 1 entries)
            w = v.win[s0 + lane], wv = v.var[s0 + lane];
            const int32_t which = splice_variant_which(uint32_t(key >> (2u * lane)) & 3u);
            const uint64_t slot = 2u * (uint64_t(s0) + lane) + uint32_t(which > 0);
            off = v.win_off[slot], end = v.win_off[slot + 1u];
        }
    } else if (mine)
        w = v.win[s0 + lane], off = v.win_off[s0 + lane], end = v.win_off[s0 + lane + 1];
    int32_t state = IOC_SPLICE_LACK, last_hi = 0;
    uint32_t idx = 0, n_done = 0;
    for (uint32_t b = 0; b < ns; ++b) {  // (uniform: every lane of the wave takes every step)
        int32_t s = lane == b && mine ? (VARIANTS ? splice_state_variants(key, b, w, wv, last_hi) : splice_state(key, b, w, last_hi)) : IOC_SPLICE_LACK;
        s = __shfl(s, int(b), 64);
        const int32_t hi = __shfl(w.hi, int(b), 64);
        if (lane == b) state = s, idx = n_done;
        if (s == IOC_SPLICE_DONE) last_hi = hi, ++n_done;
    }
    const bool done = state == IOC_SPLICE_DONE;
    const int32_t len = done ? int32_t(end - off) : 0;
    const uint32_t n_unc = uint32_t(__popcll(__ballot(state == IOC_SPLICE_UNCALLED))), n_ovl = uint32_t(__popcll(__ballot(state == IOC_SPLICE_OVERLAP)));
    const uint32_t rows = wave_sum(done ? uint32_t(w.hi - w.lo) : 0u), bytes = wave_sum(uint32_t(len));
    if (lane < ns) {
        const uint64_t at = uint64_t(v.splice_off[x]) + lane;
        if (at < v.n_splice) {
            // (`at` of a DONE site is the write pass's: one writer a word)
            v.splice[at].state = state, v.splice[at].len = len, v.splice[at].reserved = 0;
            if (!done) v.splice[at].at = -1;
        }
    }
    if (done) v.plan[uint64_t(x) * PLAN_MAX + idx] = IocSpliceIv{w.lo, w.hi, len, int32_t(lane), off};
    if (lane == 0) {
        v.plan_n[x] = n_done;
        ioc_splice_stats ss{};
        ss.n_done = int32_t(n_done), ss.n_uncalled = int32_t(n_unc), ss.n_overlap = int32_t(n_ovl), ss.rows_replaced = int32_t(rows), ss.spliced_bytes = int32_t(bytes);
        v.sstats[x] = ss;
    }
}

template <bool EMIT>
__global__ void __launch_bounds__(CHUNK)
k_splice_call(IocSpliceDev v, const ioc_pileup_col* __restrict__ cols, const ioc_pileup_ins* __restrict__ ins, uint64_t n_rows,
              const uint8_t* __restrict__ frames, uint64_t frame_bytes, int32_t min_depth, long long* __restrict__ seg_len,
              ioc_polish_stats* __restrict__ stats, const long long* __restrict__ out_off, uint8_t* __restrict__ out_seq, uint8_t* __restrict__ out_qual,
              uint64_t out_bytes)
{
    __shared__ IocSpliceIv plan[PLAN_MAX];
    __shared__ unsigned long long win_at[PLAN_MAX];
    __shared__ uint32_t part[2][WAVES * 5u];
    const uint32_t x = blockIdx.x;
    if (x >= v.n_gsegs) return;  // (whole workgroups)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const IocPileSeg s = v.gsegs[x];
    const uint32_t rows = uint32_t(s.rlen) + 1u, nchunks = (rows + CHUNK - 1u) / CHUNK;
    const uint32_t np = v.plan_n[x] < PLAN_MAX ? v.plan_n[x] : PLAN_MAX;
    if (tid < np) plan[tid] = v.plan[uint64_t(x) * PLAN_MAX + tid];
    __syncthreads();

    if (!EMIT) {
        uint32_t n = 0, k_ins = 0, k_sub = 0, k_del = 0, k_low = 0;
        for (uint32_t c = 0; c < nchunks; ++c) {
            const uint32_t p = c * CHUNK + tid;
            if (p >= rows) break;
            const int32_t what = splice_row(plan, np, int32_t(p));
            if (what == IOC_SPLICE_ROW_GONE) continue;
            if (what >= 0) {
                n += uint32_t(plan[what].len);
                continue;
            }
            const PileRowCall r = pile_call_seg_row<false>(s, p, cols, ins, nullptr, n_rows, frames, frame_bytes, min_depth);
            n += r.n, k_ins += r.n_ins, k_sub += r.n_sub, k_del += r.n_del, k_low += r.n_low;
        }
        // (the bytes of a group-segment fit 32 bits like the record's out_len: the entries refuse a longer bound)
        const uint32_t t5[5] = {wave_sum(n), wave_sum(k_ins), wave_sum(k_sub), wave_sum(k_del), wave_sum(k_low)};
        if (lane == 0)
            for (uint32_t y = 0; y < 5u; ++y) part[0][wave * 5u + y] = t5[y];
        __syncthreads();
        if (tid == 0) {
            uint32_t t[5] = {0, 0, 0, 0, 0};
            for (uint32_t w = 0; w < WAVES; ++w)
                for (uint32_t y = 0; y < 5u; ++y) t[y] += part[0][w * 5u + y];
            seg_len[x] = (long long)t[0];
            ioc_polish_stats st{};
            st.out_len = int32_t(t[0]), st.n_ins = int32_t(t[1]), st.n_sub = int32_t(t[2]), st.n_del = int32_t(t[3]), st.n_low = int32_t(t[4]);
            stats[x] = st;
        }
        return;
    }

    const unsigned long long first = (unsigned long long)out_off[x];
    unsigned long long carry = first;
    for (uint32_t c = 0; c < nchunks; ++c) {  // (every lane of the workgroup takes every step: there are barriers in it)
        const uint32_t p = c * CHUNK + tid;
        const int32_t what = p < rows ? splice_row(plan, np, int32_t(p)) : IOC_SPLICE_ROW_GONE;
        PileRowCall r{};
        if (p < rows && what == IOC_SPLICE_ROW_CALL) r = pile_call_seg_row<false>(s, p, cols, ins, nullptr, n_rows, frames, frame_bytes, min_depth);
        const uint32_t n = what >= 0 ? uint32_t(plan[what].len) : r.n;
        const uint32_t incl = wave_scan_incl(n, lane);
        uint32_t* tot = part[c & 1u];  // (two sets: a wave may be a step ahead of another one's reads)
        if (lane == 63u) tot[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < WAVES; ++w) {
            const uint32_t t = tot[w];
            before += w < wave ? t : 0u;
            all += t;
        }
        unsigned long long at = carry + before + (incl - n);
        if (what >= 0) {  // (the window's bytes are the whole workgroup's, below)
            win_at[what] = at;
            const uint64_t rec = uint64_t(v.splice_off[x]) + uint32_t(plan[what].site);
            if (rec < v.n_splice) v.splice[rec].at = int32_t(at - first);
        }
        for (uint32_t y = 0; y < r.n; ++y, ++at)
            if (at < out_bytes) {
                out_seq[at] = uint8_t(r.seq >> (8u * y));
                out_qual[at] = uint8_t(r.qual >> (8u * y));
            }
        carry += all;
    }
    __syncthreads();
    for (uint32_t i = 0; i < np; ++i) {
        const IocSpliceIv iv = plan[i];
        const unsigned long long at = win_at[i];
        for (uint32_t y = tid; y < uint32_t(iv.len); y += CHUNK) {
            const uint64_t from = uint64_t(iv.off) + y;
            if (from < v.win_bytes && at + y < out_bytes) {
                out_seq[at + y] = v.wseq[from];
                out_qual[at + y] = v.wqual[from];
            }
        }
    }
}

}  // namespace

// k_splice_plan over the view's group-segments: the site records, the splice records and the plans; the slot-aware instantiation
// where the view has variant records
hipError_t iock_splice_plan(hipStream_t st, const IocSpliceDev& v)
{
    if (v.n_gsegs == 0) return hipSuccess;
    if (v.var)
        hipLaunchKernelGGL((k_splice_plan<true>), dim3((v.n_gsegs + WAVES - 1u) / WAVES), dim3(CHUNK), 0, st, v);
    else
        hipLaunchKernelGGL((k_splice_plan<false>), dim3((v.n_gsegs + WAVES - 1u) / WAVES), dim3(CHUNK), 0, st, v);
    return hipGetLastError();
}

// k_splice_call over the view's group-segments, whose tables are cols / ins (n_rows records each) and whose frames lie in `frames`.
// emit false: seg_len[x] and stats[x]; emit true: the bytes, from out_off[x] on of out_seq / out_qual (out_bytes bytes each; nothing
// is written behind them), and `at` of the DONE sites' records.
hipError_t iock_splice_call(hipStream_t st, const IocSpliceDev& v, bool emit, const ioc_pileup_col* cols, const ioc_pileup_ins* ins, uint64_t n_rows,
                            const uint8_t* frames, uint64_t frame_bytes, int32_t min_depth, int64_t* seg_len, ioc_polish_stats* stats, const int64_t* out_off,
                            uint8_t* out_seq, uint8_t* out_qual, uint64_t out_bytes)
{
    static_assert(sizeof(long long) == sizeof(int64_t), "offsets");
    if (v.n_gsegs == 0) return hipSuccess;
    if (emit)
        hipLaunchKernelGGL((k_splice_call<true>), dim3(v.n_gsegs), dim3(CHUNK), 0, st, v, cols, ins, n_rows, frames, frame_bytes, min_depth,
                           static_cast<long long*>(nullptr), static_cast<ioc_polish_stats*>(nullptr), reinterpret_cast<const long long*>(out_off), out_seq,
                           out_qual, out_bytes);
    else
        hipLaunchKernelGGL((k_splice_call<false>), dim3(v.n_gsegs), dim3(CHUNK), 0, st, v, cols, ins, n_rows, frames, frame_bytes, min_depth,
                           reinterpret_cast<long long*>(seg_len), stats, static_cast<const long long*>(nullptr), static_cast<uint8_t*>(nullptr),
                           static_cast<uint8_t*>(nullptr), uint64_t(0));
    return hipGetLastError();
}
