// ioc_win_stage.h — the body that the window kernels share (ioc_insert_windows.hip, ioc_window_variants.hip), written once: the
// lower median of a set of a site's members by (window length, pair).  Device code only.  The function takes the set as a
// parameter — what a lane holds of member m: whether it is in the set, its pair and its length — and no flag that says which
// kernel is calling.  The __global__ kernels stay in their files.
//
// A wave per site, nothing shared between waves: no LDS and no barrier, and every lane of the wave takes every step.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ioc_insert_windows.h"
#include "ioc_wave.h"

struct WinMedian {
    int32_t pair = -1, len = 0;  // the member of rank (n - 1) / 2, -1 and 0 for an empty set
};

// The members mb .. me - 1, 64 at a time: every member of the set gets its rank as the number of members of the set with a smaller
// (length, pair) — those of a chunk are handed round the wave one by one, unsigned compares —, and the one of rank win_median_rank(
// n_set) is returned.  Quadratic in the set.  in_set(m, pair, len): lane's member m (false from me on), the same answer every time.
template <class InSet>
__device__ __forceinline__ WinMedian win_lower_median(uint32_t mb, uint32_t me, uint32_t n_set, InSet in_set)
{
    WinMedian t;
    if (n_set == 0u) return t;  // (the same in every lane, like everything the loops below branch on)
    const uint32_t lane = threadIdx.x & 63u, want = win_median_rank(n_set);
    for (uint32_t a0 = mb; a0 < me && t.pair < 0; a0 += 64u) {
        uint32_t a_pair = 0xFFFFFFFFu, a_len = 0;
        const bool a_in = in_set(a0 + lane, a_pair, a_len);
        if (!__ballot(a_in)) continue;
        uint32_t rank = 0;
        for (uint32_t b0 = mb; b0 < me; b0 += 64u) {
            uint32_t b_pair = 0xFFFFFFFFu, b_len = 0;
            const bool b_in = in_set(b0 + lane, b_pair, b_len);
            for (unsigned long long left = __ballot(b_in); left; left &= left - 1ull) {
                const uint32_t r = uint32_t(__builtin_ctzll(left));
                rank += win_voter_less(shfl32(b_len, r), shfl32(b_pair, r), a_len, a_pair) ? 1u : 0u;
            }
        }
        const unsigned long long hit = __ballot(a_in && rank == want);
        if (hit) t.pair = int32_t(shfl32(a_pair, uint32_t(__builtin_ctzll(hit)))), t.len = int32_t(shfl32(a_len, uint32_t(__builtin_ctzll(hit))));
    }
    return t;
}
