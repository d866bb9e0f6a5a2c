// ioc_group_pile.hip — the pileup tables of ANY NUMBER of groups of a segment's pairs, added up from the pairs' own byte planes:
// what the consensus of every isoform of a cluster is called from (ioc_planes_polish_groups, ioc_align_pairs_blocks_polish; the
// definition is ioc_host_planes_pile over every group's reads, ioc_align.cpp).
//
//   k_group_pile   one workgroup of GP_WAVES waves per 64 rows of a group-segment that has reads; a lane owns a row.  The
//                  workgroup walks its group's OWN member list, gmembers[gmem_off[x] .. gmem_off[x + 1]) in ascending pair order
//                  (group_member_lists, ioc_sink_plan.h): no member of another group is touched and there is no group test in the
//                  loop, so n groups cost the member list once, not n times.  The waves take the list interleaved, wave w the
//                  positions w, w + GP_WAVES, .., and each keeps two members in flight: the seven plane bytes of the next member
//                  (its row of the base plane and of the six slot planes; the 64 lanes read 64 consecutive bytes of each) are
//                  loaded before the current member's are added — eight members a round per workgroup, where k_plane_pile
//                  (ioc_plane_pile.hip), latency-bound on a deep segment, has four.  Where a member's planes lie is two more
//                  dependent reads (the list, then the pair's plane offset): a wave takes those out of the walk by reading
//                  them GP_AHEAD steps at a time, lane l the offset of step l of the chunk, and handing each step its offset
//                  with a readlane.  A lane that has nothing to read holds bytes that add to no counter, so the walk has no
//                  branch that differs between lanes.  The 6 + 30 counters live in registers under constant indices.  Waves 1 .. GP_WAVES - 1 leave their counters in LDS, counter-major so
//                  that a wave's 64 lanes touch 64 consecutive words; wave 0 adds them in wave order, derives ins_runs (the sum
//                  of slot 0) and ins_bases (the sum of all slots) and writes its row of both tables, 160 bytes.  Integer sums
//                  in a fixed order, one writer per word, no atomics: the tables do not depend on scheduling.
// The call itself is k_pile_call / k_pile_scan (ioc_pile_call.hip) over the group-segments; those kernels are not touched.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ioc_group_pile.h"
#include "ioc_internal.h"

namespace {

constexpr uint32_t SLOTS = IOC_PILE_INS_SLOTS;
constexpr uint32_t GP_WAVES = IOC_GROUP_PILE_WAVES;
constexpr uint32_t GP_ACC = 6u + SLOTS * 5u;  // counters a lane keeps: the six of the base plane, five per slot

struct GpBytes {  // a member's seven plane bytes at a lane's row
    uint32_t b, sl[SLOTS];
};

constexpr uint32_t GP_AHEAD = IOC_GROUP_PILE_AHEAD;
static_assert(GP_AHEAD == 64 && IOC_GROUP_PILE_FLIGHT == 2, "a lane per step of a chunk; the walk below takes the steps two by two");

// the bytes at a lane's row p of the member whose planes start at `at0` (the same in every lane), or bytes that add nothing
__device__ __forceinline__ GpBytes gp_load(uint64_t at0, const uint8_t* __restrict__ base_planes, const uint8_t* __restrict__ slot_planes, uint64_t plane_bytes,
                                            uint32_t p, bool live)
{
    GpBytes v;
    v.b = group_pile_no_base();
#pragma unroll
    for (uint32_t j = 0; j < SLOTS; ++j) v.sl[j] = 0u;
    if (at0 == group_pile_no_plane()) return v;  // (the same in every lane)
    const uint64_t at = at0 + p;
    if (live && at < plane_bytes) {
        v.b = base_planes[at];
#pragma unroll
        for (uint32_t j = 0; j < SLOTS; ++j) v.sl[j] = slot_planes[uint64_t(j) * plane_bytes + at];
    }
    return v;
}

// lane `from`'s 64-bit value in every lane (`from`: the same in every lane)
__device__ __forceinline__ uint64_t gp_readlane(uint64_t v, uint32_t from)
{
    const uint32_t lo = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v)), int(from)));
    const uint32_t hi = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v >> 32)), int(from)));
    return uint64_t(hi) << 32 | lo;
}

__global__ void __launch_bounds__(64 * GP_WAVES)
k_group_pile(const IocGroupWork* __restrict__ work, uint32_t n_work, const IocPileSeg* __restrict__ gsegs, uint32_t n_gsegs, const uint32_t* __restrict__ gmem_off,
             const uint32_t* __restrict__ gmembers, uint32_t n_members, uint32_t n_pairs, const uint64_t* __restrict__ plane,
             const uint8_t* __restrict__ base_planes, const uint8_t* __restrict__ slot_planes, uint64_t plane_bytes,
             ioc_pileup_col* __restrict__ gcols, ioc_pileup_ins* __restrict__ gins, uint64_t n_rows)
{
    __shared__ uint32_t part[(GP_WAVES - 1u) * GP_ACC * 64u];
    if (blockIdx.x >= n_work) return;  // (whole workgroups)
    const IocGroupWork wk = work[blockIdx.x];
    if (wk.gseg >= n_gsegs) return;  // (whole workgroups)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));  // (a scalar: the member walk below is one)
    const IocPileSeg s = gsegs[wk.gseg];
    const uint32_t p = wk.row + lane;
    const bool live = p <= uint32_t(s.rlen);
    const uint32_t m0 = gmem_off[wk.gseg];
    const uint32_t m1 = min(gmem_off[wk.gseg + 1u], n_members);

    uint32_t cb[6] = {0, 0, 0, 0, 0, 0};
    uint32_t cs[SLOTS][5] = {};
    const uint32_t steps = group_pile_steps(m0, m1, wave);
    for (uint32_t t0 = 0; t0 < steps; t0 += GP_AHEAD) {  // (no barrier inside the walk)
        // lane l: where the member of step t0 + l has its planes
        uint64_t mine = group_pile_no_plane();
        if (t0 + lane < steps) {
            const uint32_t i = gmembers[group_pile_at(m0, wave, t0 + lane)];
            if (i < n_pairs) mine = plane[i];
        }
        const uint32_t n = min(GP_AHEAD, steps - t0);
        for (uint32_t s2 = 0; s2 < n; s2 += 2u) {
            const GpBytes cur = gp_load(gp_readlane(mine, s2), base_planes, slot_planes, plane_bytes, p, live);
            const GpBytes nxt = gp_load(s2 + 1u < n ? gp_readlane(mine, s2 + 1u) : group_pile_no_plane(), base_planes, slot_planes, plane_bytes, p, live);
#pragma unroll
            for (uint32_t v = 0; v < 6u; ++v) cb[v] += uint32_t(plane_base_adds(cur.b, v)) + uint32_t(plane_base_adds(nxt.b, v));
#pragma unroll
            for (uint32_t j = 0; j < SLOTS; ++j)
#pragma unroll
                for (uint32_t ch = 0; ch < 5u; ++ch) cs[j][ch] += uint32_t(plane_slot_adds(cur.sl[j], ch)) + uint32_t(plane_slot_adds(nxt.sl[j], ch));
        }
    }

    if (wave > 0u) {
        uint32_t* mine = part + size_t(wave - 1u) * GP_ACC * 64u + lane;
#pragma unroll
        for (uint32_t v = 0; v < 6u; ++v) mine[plane_part_at(v)] = cb[v];
#pragma unroll
        for (uint32_t j = 0; j < SLOTS; ++j)
#pragma unroll
            for (uint32_t ch = 0; ch < 5u; ++ch) mine[plane_part_at(6u + j * 5u + ch)] = cs[j][ch];
    }
    __syncthreads();
    if (wave > 0u) return;
#pragma unroll
    for (uint32_t w = 1; w < GP_WAVES; ++w) {  // (wave order: a fixed order of integer adds)
        const uint32_t* theirs = part + size_t(w - 1u) * GP_ACC * 64u + lane;
#pragma unroll
        for (uint32_t v = 0; v < 6u; ++v) cb[v] += theirs[plane_part_at(v)];
#pragma unroll
        for (uint32_t j = 0; j < SLOTS; ++j)
#pragma unroll
            for (uint32_t ch = 0; ch < 5u; ++ch) cs[j][ch] += theirs[plane_part_at(6u + j * 5u + ch)];
    }
    const uint64_t row = uint64_t(s.row0) + p;
    if (!live || row >= n_rows) return;
    ioc_pileup_col col{};
    ioc_pileup_ins in{};
    col.a = cb[0], col.c = cb[1], col.g = cb[2], col.t = cb[3], col.other = cb[4], col.del = cb[5];
#pragma unroll
    for (uint32_t j = 0; j < SLOTS; ++j)
#pragma unroll
        for (uint32_t ch = 0; ch < 5u; ++ch) {
            in.slot[j][ch] = cs[j][ch];
            col.ins_bases += cs[j][ch];
            if (j == 0u) col.ins_runs += cs[j][ch];
        }
    gcols[row] = col;
    gins[row] = in;
}

}  // namespace

static_assert(sizeof(ioc_pileup_col) == 32 && sizeof(ioc_pileup_ins) == 128 && IOC_PILE_INS_SLOTS == 6, "the tables are laid out as the public records");

// The tables of the group-segments gsegs (device; n_gsegs of them, row0 and rlen are read; group-segment x: the pairs
// gmembers[gmem_off[x] .. gmem_off[x + 1]), n_members in all) from the planes: work item w is 64 rows of a group-segment, from
// `row` on.  Rows no work item covers are not written: the caller has set the tables (n_rows records each) to 0.
hipError_t iock_group_pile(hipStream_t st, const IocGroupWork* work, uint32_t n_work, const IocPileSeg* gsegs, uint32_t n_gsegs, const uint32_t* gmem_off,
                           const uint32_t* gmembers, uint32_t n_members, uint32_t n_pairs, const uint64_t* plane, const uint8_t* base_planes,
                           const uint8_t* slot_planes, uint64_t plane_bytes, ioc_pileup_col* gcols, ioc_pileup_ins* gins, uint64_t n_rows)
{
    if (n_work == 0) return hipSuccess;
    hipLaunchKernelGGL(k_group_pile, dim3(n_work), dim3(64 * GP_WAVES), 0, st, work, n_work, gsegs, n_gsegs, gmem_off, gmembers, n_members, n_pairs, plane,
                       base_planes, slot_planes, plane_bytes, gcols, gins, n_rows);
    return hipGetLastError();
}
