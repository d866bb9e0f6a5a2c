// ioc_ops_stats.hip — the statistics of the alignments of an emitting slice, reduced where the walks left their bytes
// (ioc_align_pairs_stats; the definition is ioc_host_ops_stats, ioc_align.cpp).
//
// One wave per pair.  The pair's operation string stands at buf[end - len .. end), at any byte alignment; the wave reads it in
// chunks of 64 dwords from the aligned-down address (one dword per lane: 256 consecutive bytes per load instruction), the next
// chunk's load in flight while this one is counted.  A chunk is counted in four steps of 64 bytes: lane l of step j takes the byte
// at position 64 j + l of the chunk — byte l % 4 of the dword lane 16 j + l / 4 holds (one cross-lane read) — so that bit l of a
// ballot IS position l, and everything that depends on the order of the bytes is bit arithmetic on 64-bit masks in scalar
// registers: counts are popcounts, run starts are mask & ~(mask << 1 | carry), the longest run comes from the trailing and leading
// ones of each mask and the length of the run still open, the walk's first and last column from ctz / clz of the walk mask.
// Bytes outside the string (the head before it, the tail behind it) are masked to 0, which is no operation: they count nowhere
// and end every run.  No LDS, no atomics, no scratch; the record leaves through plain stores of lane 0.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ioc_internal.h"

namespace {

constexpr int OS_WAVES = 4;  // pairs per workgroup (nothing is shared between them)

// the maximal runs of one byte value, over the masks of consecutive 64-byte steps
struct RunStat {
    uint32_t bytes = 0, runs = 0, longest = 0;
    uint32_t open = 0;  // length of the run that ends at the last byte seen so far (0: that byte is something else)
    __host__ __device__ __forceinline__ void step(unsigned long long m)
    {
        if (m == 0ull) {
            open = 0;
            return;
        }
        bytes += uint32_t(__builtin_popcountll(m));
        runs += uint32_t(__builtin_popcountll(m & ~((m << 1) | (open ? 1ull : 0ull))));
        if (m == ~0ull) {
            open += 64u;
            longest = longest > open ? longest : open;
            return;
        }
        // the run that comes in from the step before, continued by the ones at the bottom of the mask; the longest run inside the
        // mask (x &= x << 1 shortens every run by one)
        uint32_t in = open + uint32_t(__builtin_ctzll(~m)), n = 0;
        for (unsigned long long x = m; x; x &= x << 1) ++n;
        in = in > n ? in : n;
        longest = longest > in ? longest : in;
        open = uint32_t(__builtin_clzll(~m));
    }
};

// What a wave knows of its string so far; one step per 64 bytes, bit l of a mask = the l-th of them.  Everything here is the
// same in every lane (the masks are ballots).
struct OpsAcc {
    uint32_t n_eq = 0, n_x = 0;
    RunStat ins, del;
    bool walk_seen = false;
    uint32_t lead_i = 0, lead_d = 0, trail_i = 0, trail_d = 0;  // trail_*: the 'i' / 'd' behind the last walk byte seen so far
    __host__ __device__ __forceinline__ void step(unsigned long long m_eq, unsigned long long m_x, unsigned long long m_i, unsigned long long m_d,
                                                  unsigned long long e_i, unsigned long long e_d)
    {
        n_eq += uint32_t(__builtin_popcountll(m_eq));
        n_x += uint32_t(__builtin_popcountll(m_x));
        ins.step(m_i);
        del.step(m_d);
        const unsigned long long walk = m_eq | m_x | m_i | m_d;
        if (walk) {
            if (!walk_seen) {  // the end gaps below the walk's first column are the leading ones
                const unsigned long long below = (1ull << __builtin_ctzll(walk)) - 1ull;
                lead_i += uint32_t(__builtin_popcountll(e_i & below));
                lead_d += uint32_t(__builtin_popcountll(e_d & below));
                walk_seen = true;
            }
            const uint32_t top = 63u - uint32_t(__builtin_clzll(walk));  // the last walk column of this step
            const unsigned long long above = top == 63u ? 0ull : ~0ull << (top + 1u);
            trail_i = uint32_t(__builtin_popcountll(e_i & above));
            trail_d = uint32_t(__builtin_popcountll(e_d & above));
        } else if (walk_seen) {
            trail_i += uint32_t(__builtin_popcountll(e_i));
            trail_d += uint32_t(__builtin_popcountll(e_d));
        } else {
            lead_i += uint32_t(__builtin_popcountll(e_i));
            lead_d += uint32_t(__builtin_popcountll(e_d));
        }
    }
    __host__ __device__ __forceinline__ ioc_aln_stats record(uint32_t length) const
    {
        ioc_aln_stats s;
        s.length = int32_t(length);
        s.columns = int32_t(n_eq + n_x + ins.bytes + del.bytes);
        s.matches = int32_t(n_eq);
        s.mismatches = int32_t(n_x);
        s.ins = int32_t(ins.bytes);
        s.del = int32_t(del.bytes);
        s.ins_runs = int32_t(ins.runs);
        s.del_runs = int32_t(del.runs);
        s.longest_ins = int32_t(ins.longest);
        s.longest_del = int32_t(del.longest);
        s.lead_i = int32_t(lead_i);
        s.lead_d = int32_t(lead_d);
        s.trail_i = int32_t(trail_i);
        s.trail_d = int32_t(trail_d);
        s.reserved[0] = s.reserved[1] = 0;
        return s;
    }
};

__global__ void __launch_bounds__(64 * OS_WAVES)
k_ops_stats(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ end, const uint32_t* __restrict__ len,
            const uint32_t* __restrict__ room, const uint32_t* __restrict__ ord, uint32_t cnt, ioc_aln_stats* __restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t x = blockIdx.x * OS_WAVES + (threadIdx.x >> 6);
    if (x >= cnt) return;  // (whole waves: there is no barrier below)
    const uint32_t pid = ord[x];
    const uint64_t L = len[pid], e = end[pid];
    if (L == 0 || L > room[pid] || L > e) return;  // came back without an answer: left to its re-run (as ops_fetch has it)

    const uint8_t* first = buf + (e - L);
    const uint32_t head = uint32_t(reinterpret_cast<uintptr_t>(first) & 3u);
    const uint32_t* words = reinterpret_cast<const uint32_t*>(first - head);
    const uint32_t span = head + uint32_t(L);  // bytes from the aligned-down address to the string's end (L < 2^27)
    const uint32_t nwords = (span + 3u) / 4u, nchunks = (nwords + 63u) / 64u;

    OpsAcc acc;
    uint32_t w = lane < nwords ? words[lane] : 0u;
    for (uint32_t c = 0; c < nchunks; ++c) {
        const uint32_t nx = (c + 1u) * 64u + lane;
        const uint32_t w_next = nx < nwords ? words[nx] : 0u;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t pos = c * 256u + j * 64u + lane;
            const uint32_t v = uint32_t(__shfl(int(w), int(16u * j + (lane >> 2)), 64));
            const uint32_t b = (pos >= head && pos < span) ? (v >> (8u * (lane & 3u))) & 0xFFu : 0u;
            acc.step(__ballot(b == uint32_t('=')), __ballot(b == uint32_t('X')), __ballot(b == uint32_t('I')), __ballot(b == uint32_t('D')),
                     __ballot(b == uint32_t('i')), __ballot(b == uint32_t('d')));
        }
        w = w_next;
    }
    if (lane == 0) out[x] = acc.record(uint32_t(L));
}

}  // namespace

// The pairs ord[0 .. cnt) of a slice (device pair ids); record x of `out` is pair ord[x]'s.  room[pid]: query length + reference
// length.  The dword that holds a string's last byte is read whole: `buf` needs 3 readable bytes behind the slice's last region.
hipError_t iock_ops_stats(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room,
                          const uint32_t* ord, uint32_t cnt, ioc_aln_stats* out)
{
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ops_stats, dim3((cnt + OS_WAVES - 1) / OS_WAVES), dim3(64 * OS_WAVES), 0, st, buf, end, len, room, ord, cnt, out);
    return hipGetLastError();
}
