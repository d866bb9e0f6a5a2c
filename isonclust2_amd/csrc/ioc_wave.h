// ioc_wave.h — what passes from lane to lane of a 64-lane wave in the stages behind the aligner (pile_sites, pile_call, site_split,
// read_correct, read_blocks, read_inserts, read_ends, insert_windows, window_variants, iso_splice): shuffles of 32 and 64 bits, the inclusive scan
// and the reductions, each written once.  Device code only; every lane of the wave has to take part in every call.
//
// wave_scan_incl is the shuffle form: six __shfl_up steps.  ioc_kdev.h has wave_incl_scan, the data-parallel-move form that the
// assignment path measured its way to.  The two are different code of different speed and each stays with its callers: do not
// replace the one by the other for the sake of the name.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

__device__ __forceinline__ uint32_t shfl32(uint32_t v, uint32_t src) { return uint32_t(__shfl(int(v), int(src), 64)); }
__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, uint32_t src)
{
    const uint32_t lo = shfl32(uint32_t(v), src), hi = shfl32(uint32_t(v >> 32), src);
    return (unsigned long long)hi << 32 | lo;
}
__device__ __forceinline__ unsigned long long shfl_up64(unsigned long long v, uint32_t d)
{
    const uint32_t lo = uint32_t(__shfl_up(int(uint32_t(v)), d, 64)), hi = uint32_t(__shfl_up(int(uint32_t(v >> 32)), d, 64));
    return (unsigned long long)hi << 32 | lo;
}
__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, uint32_t d)
{
    const uint32_t lo = uint32_t(__shfl_xor(int(uint32_t(v)), int(d), 64)), hi = uint32_t(__shfl_xor(int(uint32_t(v >> 32)), int(d), 64));
    return (unsigned long long)hi << 32 | lo;
}

// the sum of v over lanes 0 .. lane
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t up = uint32_t(__shfl_up(int(v), d, 64));
        if (lane >= d) v += up;
    }
    return v;
}

// The reductions: every lane gets the result over all 64.
__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) v += uint32_t(__shfl_xor(int(v), int(d), 64));
    return v;
}
__device__ __forceinline__ int32_t wave_sum32(int32_t v)  // (signed)
{
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) v += __shfl_xor(v, int(d), 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) v = min(v, uint32_t(__shfl_xor(int(v), int(d), 64)));
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) v = max(v, uint32_t(__shfl_xor(int(v), int(d), 64)));
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v)
{
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) v += shfl_xor64(v, d);
    return v;
}
__device__ __forceinline__ unsigned long long wave_or64(unsigned long long v)
{
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) v |= shfl_xor64(v, d);
    return v;
}
__device__ __forceinline__ unsigned long long wave_max64(unsigned long long v)
{
#pragma unroll
    for (uint32_t d = 32; d >= 1u; d >>= 1) v = max(v, shfl_xor64(v, d));
    return v;
}
