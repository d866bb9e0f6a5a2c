// ioc_pile_sites.hip — the variable sites of many references and every read's alleles at them, where the pileup lies
// (ioc_pileup_sites, ioc_align_pairs_alleles; the definitions are ioc_host_ops_project, ioc_host_pileup_sites and
// ioc_host_site_alleles, ioc_align.cpp).
//
//   k_ops_project       beside k_ops_pileup, over the same bytes of a slice: one wave per pair walks the pair's string as
//                       k_ops_pileup does (ioc_ops_pileup.hip: chunks of 64 aligned dwords, four steps of 64 bytes, PileAcc) and,
//                       where that kernel adds 1 to a word of the shared table, stores one byte into the pair's OWN planes: the
//                       channel (or 5 for 'D') at its row of the base plane, 1 at the row of the first 'I' of a run in the ins
//                       plane.  Every byte has one writer — a row of a pair is consumed by one byte of its string — so there
//                       are no atomics, and a re-run that repeats a pair rewrites the bytes it wrote.  No LDS, no scratch.
//   k_pile_sites<false> counts: one workgroup per segment in chunks of IOC_PILE_CALL_CHUNK rows, a lane per row (pile_sites_row,
//                       ioc_pile_sites.h — the function the definition uses); n_found[g] and what the segment keeps.
//   k_sites_scan        one wave: site_off[0 .. n_segs] = the exclusive scan of what the segments keep, 64 a step, a running carry.
//   k_pile_sites<true>  decides again and writes the records: a wave scan and a workgroup scan place a row's 0, 1 or 2 records,
//                       a running carry runs down the segment's chunks, emission stops at max_sites.
//   k_site_alleles      one wave per pair: lane s reads site s of the pair's segment and the one byte (two, at an insertion
//                       site in front of the last row) of the pair's planes that answers it.
// As in ioc_pile_call.hip every output has one writer and its place is a function of the table alone.  (The scans repeat that
// file's few lines rather than share them: its kernels stay the code they are.)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ioc_internal.h"
#include "ioc_pile_sites.h"
#include "ioc_wave.h"

namespace {

constexpr int OP_WAVES = 4;                      // pairs per workgroup of k_ops_project and k_site_alleles
constexpr uint32_t CHUNK = IOC_PILE_CALL_CHUNK;  // rows per step of a workgroup of k_pile_sites = its threads
constexpr uint32_t WAVES = CHUNK / 64u;
static_assert(CHUNK % 64u == 0 && WAVES >= 1 && WAVES <= 16, "whole waves");

__global__ void __launch_bounds__(64 * OP_WAVES)
k_ops_project(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ end, const uint32_t* __restrict__ len,
              const uint32_t* __restrict__ room, const uint32_t* __restrict__ ord, uint32_t cnt, const int64_t* __restrict__ row_base,
              const uint32_t* __restrict__ q_off, const uint64_t* __restrict__ plane, const uint8_t* __restrict__ pool, uint64_t pool_bytes,
              uint8_t* __restrict__ base_planes, uint8_t* __restrict__ ins_planes, uint64_t plane_bytes)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t x = blockIdx.x * OP_WAVES + (threadIdx.x >> 6);
    if (x >= cnt) return;  // (whole waves: there is no barrier below)
    const uint32_t pid = ord[x];
    const uint64_t L = len[pid], e = end[pid];
    if (L == 0 || L > room[pid] || L > e) return;  // came back without an answer: left to its re-run (as k_ops_pileup has it)
    if (row_base[pid] < 0) return;                 // (piled and projected by an earlier run of this call already)
    const uint64_t qo = q_off[pid], po = plane[pid];

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
            // (a byte outside the planes, a base outside the pool: only a string that does not belong to its pair could ask for one)
            const uint64_t at_row = po + acc.row(lane);
            if (at_row < plane_bytes) {
                if (acc.is_base(lane)) {
                    const uint64_t at = qo + acc.qpos(lane);
                    if (at < pool_bytes) base_planes[at_row] = uint8_t(PileAcc::channel(pool[at]));
                } else if (acc.is_del(lane)) {
                    base_planes[at_row] = uint8_t(IOC_ALLELE_DEL);
                } else if (acc.run_start(lane)) {
                    ins_planes[at_row] = 1;
                }
            }
            acc.end();
        }
        w = w_next;
    }
}

// row p of segment s (p <= s.rlen), or nothing where its record lies outside the table
__device__ __forceinline__ PileRowSites decide(const IocPileSeg& s, uint32_t p, const ioc_pileup_col* __restrict__ cols, uint64_t n_rows,
                                               const PileSiteRule& rule)
{
    const uint32_t rlen = uint32_t(s.rlen);
    const uint64_t row = uint64_t(s.row0) + p;
    if (row >= n_rows) return PileRowSites{};
    const bool has_base = p < rlen;
    const unsigned long long d_ins = has_base ? pile_depth(cols[row]) : rlen > 0u ? pile_depth(cols[row - 1u]) : 0ull;
    return pile_sites_row(cols[row], d_ins, has_base, int32_t(p), rule);
}

template <bool EMIT>
__global__ void __launch_bounds__(CHUNK)
k_pile_sites(const IocPileSeg* __restrict__ segs, uint32_t n_segs, const ioc_pileup_col* __restrict__ cols, uint64_t n_rows, PileSiteRule rule,
             uint32_t max_sites, long long* __restrict__ n_found, long long* __restrict__ seg_len, const long long* __restrict__ site_off,
             ioc_pile_site* __restrict__ out, uint64_t sites_cap)
{
    __shared__ uint32_t part[2][WAVES];
    const uint32_t g = blockIdx.x;
    if (g >= n_segs) return;  // (whole workgroups)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const IocPileSeg s = segs[g];
    const uint32_t rows = uint32_t(s.rlen) + 1u, nchunks = (rows + CHUNK - 1u) / CHUNK;

    if (!EMIT) {
        uint32_t n = 0;  // (at most 2 per row and rlen <= 2^30, the entries see to that: 32 bits)
        for (uint32_t c = 0; c < nchunks; ++c) {
            const uint32_t p = c * CHUNK + tid;
            if (p >= rows) break;
            n += decide(s, p, cols, n_rows, rule).n();
        }
        const uint32_t v = wave_sum(n);
        if (lane == 0) part[0][wave] = v;
        __syncthreads();
        if (tid == 0) {
            uint32_t t = 0;
            for (uint32_t w = 0; w < WAVES; ++w) t += part[0][w];
            n_found[g] = (long long)t;
            seg_len[g] = (long long)(t < max_sites ? t : max_sites);
        }
        return;
    }

    const unsigned long long off = (unsigned long long)site_off[g];
    uint32_t carry = 0;  // records of the segment's earlier chunks
    for (uint32_t c = 0; c < nchunks; ++c) {  // (every lane of the workgroup takes every step: there are barriers in it)
        const uint32_t p = c * CHUNK + tid;
        PileRowSites r{};
        if (p < rows) r = decide(s, p, cols, n_rows, rule);
        const uint32_t mine = r.n(), incl = wave_scan_incl(mine, lane);
        uint32_t* tot = part[c & 1u];  // (two sets: a wave may be a step ahead of another one's reads)
        if (lane == 63u) tot[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < WAVES; ++w) {
            const uint32_t t = tot[w];
            before += w < wave ? t : 0u;
            all += t;
        }
        const uint32_t k0 = carry + before + (incl - mine), k1 = k0 + uint32_t(r.has_ins);
        if (r.has_ins && k0 < max_sites && off + k0 < sites_cap) out[off + k0] = r.ins;
        if (r.has_base && k1 < max_sites && off + k1 < sites_cap) out[off + k1] = r.base;
        carry += all;
    }
}

// site_off[0 .. n_segs]: the exclusive scan of seg_len; one wave, 64 segments a step
__global__ void __launch_bounds__(64)
k_sites_scan(const long long* __restrict__ seg_len, uint32_t n_segs, long long* __restrict__ site_off)
{
    const uint32_t lane = threadIdx.x;
    unsigned long long carry = 0;
    if (lane == 0) site_off[0] = 0;
    for (uint32_t base = 0; base < n_segs; base += 64u) {
        const uint32_t g = base + lane;
        unsigned long long v = g < n_segs ? (unsigned long long)seg_len[g] : 0ull;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const unsigned long long up = shfl_up64(v, d);
            if (lane >= d) v += up;
        }
        if (g < n_segs) site_off[g + 1u] = (long long)(carry + v);
        carry += shfl64(v, 63u);
    }
}

__global__ void __launch_bounds__(64 * OP_WAVES)
k_site_alleles(uint32_t n_pairs, const int32_t* __restrict__ seg_of_pair, const IocPileSeg* __restrict__ segs, uint32_t n_segs,
               const uint64_t* __restrict__ plane, const uint8_t* __restrict__ base_planes, const uint8_t* __restrict__ ins_planes,
               uint64_t plane_bytes, const ioc_pile_site* __restrict__ sites, const long long* __restrict__ site_off,
               const long long* __restrict__ allele_off, uint8_t* __restrict__ alleles, uint64_t alleles_cap)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * OP_WAVES + (threadIdx.x >> 6);
    if (i >= n_pairs) return;
    const uint32_t g = uint32_t(seg_of_pair[i]);
    if (g >= n_segs) return;
    const uint32_t rlen = uint32_t(segs[g].rlen);
    const uint64_t po = plane[i], s0 = uint64_t(site_off[g]), n = uint64_t(site_off[g + 1u]) - s0, a0 = uint64_t(allele_off[i]);
    if (po + rlen >= plane_bytes) return;  // (the pair's planes, rlen + 1 bytes each, lie inside what was passed)
    const uint8_t b_last = rlen > 0u ? base_planes[po + rlen - 1u] : uint8_t(IOC_ALLELE_NONE);
    for (uint64_t s = lane; s < n; s += 64u) {
        const ioc_pile_site t = sites[s0 + s];
        const uint32_t row = uint32_t(t.row);
        if (row > rlen || a0 + s >= alleles_cap) continue;
        alleles[a0 + s] = pile_site_allele(t.kind, row == rlen, base_planes[po + row], ins_planes[po + row], b_last);
    }
}

}  // namespace

// Beside iock_ops_pileup*, over the same slice and the same columns: pair pid is projected into base_planes / ins_planes
// (plane_bytes bytes each) from byte plane[pid] on — reference length + 1 bytes of each, which the caller has set to
// IOC_ALLELE_NONE / 0 once.
hipError_t iock_ops_project(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room,
                            const uint32_t* ord, uint32_t cnt, const int64_t* row_base, const uint32_t* q_off, const uint64_t* plane,
                            const uint8_t* pool, uint64_t pool_bytes, uint8_t* base_planes, uint8_t* ins_planes, uint64_t plane_bytes)
{
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ops_project, dim3((cnt + OP_WAVES - 1) / OP_WAVES), dim3(64 * OP_WAVES), 0, st, buf, end, len, room, ord, cnt, row_base,
                       q_off, plane, pool, pool_bytes, base_planes, ins_planes, plane_bytes);
    return hipGetLastError();
}

// The sites of the segments segs[0 .. n_segs) (device; row0 and rlen are read) from `cols` (n_rows records): site_off[0 .. n_segs]
// and n_found[0 .. n_segs) (device), the records in out (sites_cap of them; nothing is written behind them).  seg_len: n_segs
// words of scratch.
hipError_t iock_pile_sites(hipStream_t st, const IocPileSeg* segs, uint32_t n_segs, const ioc_pileup_col* cols, uint64_t n_rows, int32_t min_depth,
                           int32_t min_alt, int32_t min_pct, int32_t max_sites, int64_t* n_found, int64_t* seg_len, int64_t* site_off,
                           ioc_pile_site* out, uint64_t sites_cap)
{
    static_assert(sizeof(long long) == sizeof(int64_t), "offsets");
    if (n_segs == 0) return hipSuccess;
    const PileSiteRule rule{min_depth, min_alt, min_pct};
    hipLaunchKernelGGL(k_pile_sites<false>, dim3(n_segs), dim3(CHUNK), 0, st, segs, n_segs, cols, n_rows, rule, uint32_t(max_sites),
                       reinterpret_cast<long long*>(n_found), reinterpret_cast<long long*>(seg_len), static_cast<const long long*>(nullptr),
                       static_cast<ioc_pile_site*>(nullptr), uint64_t(0));
    hipLaunchKernelGGL(k_sites_scan, dim3(1), dim3(64), 0, st, reinterpret_cast<const long long*>(seg_len), n_segs,
                       reinterpret_cast<long long*>(site_off));
    hipLaunchKernelGGL(k_pile_sites<true>, dim3(n_segs), dim3(CHUNK), 0, st, segs, n_segs, cols, n_rows, rule, uint32_t(max_sites),
                       static_cast<long long*>(nullptr), static_cast<long long*>(nullptr), reinterpret_cast<const long long*>(site_off), out,
                       sites_cap);
    return hipGetLastError();
}

// Pair i of n_pairs (the caller's order) gets its alleles at the kept sites of segment seg_of_pair[i], from its planes at
// plane[i], into alleles[allele_off[i] ..) (alleles_cap bytes; nothing is written behind them).
hipError_t iock_site_alleles(hipStream_t st, uint32_t n_pairs, const int32_t* seg_of_pair, const IocPileSeg* segs, uint32_t n_segs,
                             const uint64_t* plane, const uint8_t* base_planes, const uint8_t* ins_planes, uint64_t plane_bytes,
                             const ioc_pile_site* sites, const int64_t* site_off, const int64_t* allele_off, uint8_t* alleles,
                             uint64_t alleles_cap)
{
    if (n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_site_alleles, dim3((n_pairs + OP_WAVES - 1) / OP_WAVES), dim3(64 * OP_WAVES), 0, st, n_pairs, seg_of_pair, segs, n_segs,
                       plane, base_planes, ins_planes, plane_bytes, sites, reinterpret_cast<const long long*>(site_off),
                       reinterpret_cast<const long long*>(allele_off), alleles, alleles_cap);
    return hipGetLastError();
}
