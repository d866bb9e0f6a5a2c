// ioc_site_split.hip — the split of many segments' reads in two by their linked sites, where the alleles lie (ioc_alleles_split,
// ioc_align_pairs_split; the definition is ioc_host_alleles_split, ioc_align.cpp, and the four rules are ioc_site_split.h's).
//
// A segment's reads are its pairs in ascending pair index (the host's counting sort of seg_of_pair: mem_off / members); read r of
// a segment is bit r & 63 of word r >> 6.  Tile x of the call is word x - word_off[g] of segment g = tile_seg[x].
//
//   k_site_marks      a thread per site: (minor, major) of its record as two words, so that no later kernel reads 32 bytes for 8.
//   k_allele_bits     one wave per (tile, 64 sites) — a tile is 64 reads of a segment —: the 64 x 64 bytes go through LDS — written
//                     with lane = site, so that the global reads run along a read's bytes, read with lane = read — and one
//                     __ballot per site and plane gives the word.  Planes "is minor" / "is major", word-major:
//                     bits[bit_off[g] + w * n_sites + t], so that lanes over t coalesce below.
//   k_site_link       one wave per site s: lanes over t, the words of s wave-uniform, d(s, t) from four popcounts a word
//                     (split_d_word), one wave reduction: link(s).  The sites x sites table is never stored.
//   k_split_seed      one wave per segment: the first maximum of link (a wave reduction, the lower index wins a tie).
//   k_split_phase0    a thread per site: the first phase from d(seed, t).
//   k_split_vote      one wave per pair over its own allele bytes, a wave reduction: the vote and the group.
//   k_group_bits      one wave per tile: the masks "in group 1" / "in group 0" of its 64 reads, by ballot.
//   k_split_rephase   a thread per site: dg(t) from the masks and the planes, four popcounts a word; the new phase.
//   k_split_record    one wave per segment: its record.
// A round is k_group_bits, k_split_rephase, k_split_vote.  No atomics: every output word has one writer and its value is a
// function of the inputs alone.  A segment without reads or without sites has no tile or no site to launch for.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ioc_internal.h"
#include "ioc_site_split.h"
#include "ioc_wave.h"

namespace {

using u64 = unsigned long long;

constexpr int SP_WAVES = 4;      // waves per workgroup of the kernels that give a wave a site or a pair
constexpr uint32_t TILE_ROW = 68;  // bytes per read of the LDS tile: 64 and a pad that spreads a column over the banks

// d of the pair of words (a_minor, a_major) — wave-uniform or a lane's own — with site t's, over the W words of a segment
__device__ __forceinline__ int32_t d_with_site(const u64* __restrict__ a_minor, const u64* __restrict__ a_major, uint64_t a_stride,
                                               const u64* __restrict__ bm, const u64* __restrict__ bM, uint64_t bo, uint64_t n, uint32_t W, uint64_t t)
{
    int32_t d = 0;
    for (uint32_t w = 0; w < W; ++w) d += split_d_word(a_minor[w * a_stride], a_major[w * a_stride], bm[bo + w * n + t], bM[bo + w * n + t]);
    return d;
}

__global__ void __launch_bounds__(256)
k_site_marks(const ioc_pile_site* __restrict__ sites, uint64_t n_sites, int2* __restrict__ marks)
{
    const uint64_t S = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (S < n_sites) marks[S] = make_int2(sites[S].minor, sites[S].major);
}

__global__ void __launch_bounds__(64)
k_allele_bits(IocSplitDev v)
{
    __shared__ uint8_t tile[64 * TILE_ROW];
    const uint32_t lane = threadIdx.x, x = blockIdx.x;
    if (x >= v.n_tiles) return;  // (whole workgroups)
    const uint32_t g = uint32_t(v.tile_seg[x]);
    if (g >= v.n_segs) return;
    const uint32_t w = x - v.word_off[g], m0 = v.mem_off[g], nr = v.mem_off[g + 1u] - m0;
    const uint64_t s0 = uint64_t(v.site_off[g]), n = uint64_t(v.site_off[g + 1u]) - s0, bo = uint64_t(v.bit_off[g]);
    const uint32_t r = w * 64u + lane;
    const bool valid = r < nr;
    const u64 a0 = valid ? u64(v.allele_off[v.members[m0 + r]]) : 0ull;
    const uint32_t in_tile = nr - w * 64u < 64u ? nr - w * 64u : 64u;  // reads of this tile (w * 64 < nr: the host made the tile)
    // the workgroups of a tile share out its steps of 64 sites (every lane of one takes every step of its own: there are barriers)
    for (uint64_t t0 = uint64_t(blockIdx.y) * 64u; t0 < n; t0 += uint64_t(gridDim.y) * 64u) {
        const uint64_t t = t0 + lane;
        for (uint32_t k = 0; k < in_tile; ++k) {  // read k's 64 bytes, lane = site (the rows behind in_tile are never read)
            const u64 ak = shfl64(a0, k);
            uint8_t b = 0;
            if (t < n && ak + t < v.allele_bytes) b = v.alleles[ak + t];
            tile[k * TILE_ROW + lane] = b;
        }
        __syncthreads();
        const int2 mine = t < n ? v.marks[s0 + t] : make_int2(-1, -1);  // (no byte equals -1)
        u64 w_minor = 0, w_major = 0;
        for (uint32_t s = 0; s < 64u; ++s) {  // site s of the step, lane = read
            const int32_t mi = __shfl(mine.x, int(s), 64), ma = __shfl(mine.y, int(s), 64);
            const int32_t mk = valid ? split_mark(tile[lane * TILE_ROW + s], mi, ma) : 0;  // (valid: lane < in_tile)
            const u64 b_minor = __ballot(mk > 0), b_major = __ballot(mk < 0);
            if (lane == s) w_minor = b_minor, w_major = b_major;
        }
        if (t < n && bo + uint64_t(w) * n + t < v.plane_words) {
            v.bits_minor[bo + uint64_t(w) * n + t] = w_minor;
            v.bits_major[bo + uint64_t(w) * n + t] = w_major;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(64 * SP_WAVES)
k_site_link(IocSplitDev v, int32_t min_link)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t S = uint64_t(__builtin_amdgcn_readfirstlane(int(blockIdx.x * SP_WAVES + (threadIdx.x >> 6))));
    if (S >= v.n_sites) return;  // (whole waves: there is no barrier below)
    const uint32_t g = uint32_t(v.seg_of_site[S]);
    if (g >= v.n_segs) return;
    const uint64_t s0 = uint64_t(v.site_off[g]), n = uint64_t(v.site_off[g + 1u]) - s0, s = S - s0, bo = uint64_t(v.bit_off[g]);
    const uint32_t W = v.word_off[g + 1u] - v.word_off[g];
    u64 acc = 0;
    for (uint64_t t = lane; t < n; t += 64u) {
        const int32_t d = d_with_site(v.bits_minor + bo + s, v.bits_major + bo + s, n, v.bits_minor, v.bits_major, bo, n, W, t);
        const uint32_t ad = uint32_t(d < 0 ? -d : d);
        if (t != s && ad >= uint32_t(min_link)) acc += ad;
    }
    acc = wave_sum64(acc);
    if (lane == 0) v.link[S] = (long long)acc;
}

__global__ void __launch_bounds__(64)
k_split_seed(IocSplitDev v)
{
    const uint32_t lane = threadIdx.x, g = blockIdx.x;
    if (g >= v.n_segs) return;
    const uint64_t s0 = uint64_t(v.site_off[g]), n = uint64_t(v.site_off[g + 1u]) - s0;
    long long best = -1;
    uint32_t at = 0xFFFFFFFFu;  // (n < 2^31)
    for (uint64_t t = lane; t < n; t += 64u) {  // (ascending t: a lane keeps its first maximum)
        const long long l = v.link[s0 + t];
        if (l > best) best = l, at = uint32_t(t);
    }
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) {  // the largest link, the lower index among equals
        const long long o_best = (long long)shfl64(u64(best), lane ^ d);
        const uint32_t o_at = uint32_t(__shfl(int(at), int(lane ^ d), 64));
        if (o_best > best || (o_best == best && o_at < at)) best = o_best, at = o_at;
    }
    if (lane == 0) v.seed[g] = n > 0 && best > 0 ? int32_t(at) : -1;
}

__global__ void __launch_bounds__(256)
k_split_phase0(IocSplitDev v, int32_t min_link)
{
    const uint64_t S = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (S >= v.n_sites) return;
    const uint32_t g = uint32_t(v.seg_of_site[S]);
    if (g >= v.n_segs) return;
    const uint64_t s0 = uint64_t(v.site_off[g]), n = uint64_t(v.site_off[g + 1u]) - s0, bo = uint64_t(v.bit_off[g]), t = S - s0;
    const uint32_t W = v.word_off[g + 1u] - v.word_off[g];
    const int32_t seed = v.seed[g];
    int8_t ph = 0;
    if (seed >= 0 && uint64_t(seed) < n)
        ph = t == uint64_t(seed) ? int8_t(1)
                                 : split_phase(d_with_site(v.bits_minor + bo + seed, v.bits_major + bo + seed, n, v.bits_minor, v.bits_major, bo, n, W, t), min_link);
    v.phase[S] = ph;
}

__global__ void __launch_bounds__(64 * SP_WAVES)
k_split_vote(IocSplitDev v, int32_t min_margin)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * SP_WAVES + (threadIdx.x >> 6);
    if (i >= v.n_pairs) return;  // (whole waves)
    const uint32_t g = uint32_t(v.seg_of_pair[i]);
    if (g >= v.n_segs) return;
    const uint64_t s0 = uint64_t(v.site_off[g]), n = uint64_t(v.site_off[g + 1u]) - s0, a0 = uint64_t(v.allele_off[i]);
    int32_t sum = 0;
    for (uint64_t t = lane; t < n; t += 64u) {
        if (a0 + t >= v.allele_bytes) break;
        const int2 mk = v.marks[s0 + t];
        sum += int32_t(v.phase[s0 + t]) * split_mark(v.alleles[a0 + t], mk.x, mk.y);
    }
    sum = wave_sum32(sum);
    if (lane == 0) {
        v.vote[i] = sum;
        v.group[i] = split_group(sum, min_margin);
    }
}

__global__ void __launch_bounds__(64)
k_group_bits(IocSplitDev v)
{
    const uint32_t lane = threadIdx.x, x = blockIdx.x;
    if (x >= v.n_tiles) return;
    const uint32_t g = uint32_t(v.tile_seg[x]);
    if (g >= v.n_segs) return;
    const uint32_t m0 = v.mem_off[g], nr = v.mem_off[g + 1u] - m0, r = (x - v.word_off[g]) * 64u + lane;
    const uint32_t grp = r < nr ? v.group[v.members[m0 + r]] : uint32_t(IOC_SPLIT_NONE);
    const u64 b1 = __ballot(grp == 1u), b0 = __ballot(grp == 0u);
    if (lane == 0) v.g1[x] = b1, v.g0[x] = b0;
}

__global__ void __launch_bounds__(256)
k_split_rephase(IocSplitDev v, int32_t min_link)
{
    const uint64_t S = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (S >= v.n_sites) return;
    const uint32_t g = uint32_t(v.seg_of_site[S]);
    if (g >= v.n_segs) return;
    const uint64_t s0 = uint64_t(v.site_off[g]), n = uint64_t(v.site_off[g + 1u]) - s0;
    const uint32_t wo = v.word_off[g], W = v.word_off[g + 1u] - wo;
    v.phase[S] = split_phase(d_with_site(v.g1 + wo, v.g0 + wo, 1, v.bits_minor, v.bits_major, uint64_t(v.bit_off[g]), n, W, S - s0), min_link);
}

__global__ void __launch_bounds__(64)
k_split_record(IocSplitDev v)
{
    const uint32_t lane = threadIdx.x, g = blockIdx.x;
    if (g >= v.n_segs) return;
    const uint64_t s0 = uint64_t(v.site_off[g]), n = uint64_t(v.site_off[g + 1u]) - s0;
    const uint32_t m0 = v.mem_off[g], nr = v.mem_off[g + 1u] - m0;
    int32_t linked = 0, c0 = 0, c1 = 0;
    for (uint64_t t = lane; t < n; t += 64u) linked += v.phase[s0 + t] != 0;
    for (uint32_t r = lane; r < nr; r += 64u) {
        const uint32_t grp = v.group[v.members[m0 + r]];
        c0 += grp == 0u, c1 += grp == 1u;
    }
    linked = wave_sum32(linked), c0 = wave_sum32(c0), c1 = wave_sum32(c1);
    if (lane == 0) {
        const int32_t seed = v.seed[g];
        v.rec[g] = ioc_split_seg{seed, linked, int32_t(nr), c0, c1, int32_t(nr) - c0 - c1, seed >= 0 ? int64_t(v.link[s0 + uint32_t(seed)]) : int64_t(0)};
    }
}

}  // namespace

// One step of the launch sequence (ioc_align_sinks.cpp runs them in order on the context's stream, `rounds` times the last three
// of the middle): a step without anything to launch for is no launch.
hipError_t iock_site_split(hipStream_t st, const IocSplitDev& v, IocSplitStep step, int32_t min_link, int32_t min_margin)
{
    const uint32_t site_blocks = uint32_t((v.n_sites + 255u) / 256u), site_waves = uint32_t((v.n_sites + SP_WAVES - 1) / SP_WAVES);
    switch (step) {
    case IocSplitStep::marks:
        if (v.n_sites) hipLaunchKernelGGL(k_site_marks, dim3(site_blocks), dim3(256), 0, st, v.sites, v.n_sites, v.marks);
        break;
    case IocSplitStep::bits:
        if (v.n_tiles && v.n_sites) {  // (max_seg_sites: the most sites a segment has; a segment with fewer leaves the early workgroups)
            const uint64_t site_steps = (v.max_seg_sites + 63u) / 64u;
            hipLaunchKernelGGL(k_allele_bits, dim3(v.n_tiles, uint32_t(site_steps < 1u ? 1u : site_steps > 65535u ? 65535u : site_steps)), dim3(64), 0, st, v);
        }
        break;
    case IocSplitStep::link:
        if (v.n_sites) hipLaunchKernelGGL(k_site_link, dim3(site_waves), dim3(64 * SP_WAVES), 0, st, v, min_link);
        break;
    case IocSplitStep::seed:
        if (v.n_segs) hipLaunchKernelGGL(k_split_seed, dim3(v.n_segs), dim3(64), 0, st, v);
        break;
    case IocSplitStep::phase0:
        if (v.n_sites) hipLaunchKernelGGL(k_split_phase0, dim3(site_blocks), dim3(256), 0, st, v, min_link);
        break;
    case IocSplitStep::vote:
        if (v.n_pairs) hipLaunchKernelGGL(k_split_vote, dim3((v.n_pairs + SP_WAVES - 1) / SP_WAVES), dim3(64 * SP_WAVES), 0, st, v, min_margin);
        break;
    case IocSplitStep::group_bits:
        if (v.n_tiles) hipLaunchKernelGGL(k_group_bits, dim3(v.n_tiles), dim3(64), 0, st, v);
        break;
    case IocSplitStep::rephase:
        if (v.n_sites) hipLaunchKernelGGL(k_split_rephase, dim3(site_blocks), dim3(256), 0, st, v, min_link);
        break;
    case IocSplitStep::record:
        if (v.n_segs) hipLaunchKernelGGL(k_split_record, dim3(v.n_segs), dim3(64), 0, st, v);
        break;
    }
    return hipGetLastError();
}
