// ioc_group_pile_weighted.hip — the quality-weighted pileup tables of ANY NUMBER of groups of a segment's pairs, added up from
// the pairs' byte planes and the WEIGHT PLANES beside them: what the weighted consensus of every isoform of a cluster is called
// from (ioc_planes_polish_groups_weighted, ioc_align_pairs_blocks_polish_weighted; the definitions are
// ioc_host_ops_project_weights and ioc_host_planes_pile_weighted, ioc_align.cpp).
//
//   k_ops_project_weights   beside k_ops_project_ins (ioc_plane_pile.hip), over the same bytes of a slice: one wave per pair
//                           repeats that kernel's walk (chunks of 64 aligned dwords, four steps of 64 bytes, PileAcc with the run
//                           bookkeeping of the ins variant).  The lane of a '=' / 'X' stores the weight of its quality byte
//                           (pile_qual_weight) into the wbase plane at the pair's row, the lane of a 'D' the deletion weight
//                           (PileAcc::del_weight: the smaller of its neighbours' weights within the pair's own quality bytes),
//                           the lane of an 'I' whose index j in its run is below IOC_PILE_INS_SLOTS the weight of its quality
//                           byte into wslot plane j: [wbase plane][wslot-0 planes] .. [wslot-5 planes], plane_bytes each, a
//                           pair's bytes at its `plane` offset in every one of them.  A (plane, row) of a pair is consumed by one
//                           byte of its string, so every byte has one writer: plain byte stores, no atomics, and a re-run
//                           rewrites what it wrote.  No LDS, no scratch.  The planes are set to 0 before the call's first slice.
//   k_group_pile_weighted   the shape of k_group_pile (ioc_group_pile.hip): one workgroup of GP_WAVES waves per 64 rows of a
//                           group-segment that has reads, a lane per row, over the group's OWN member list, the waves
//                           interleaved, two members in flight per wave, the plane offsets read GP_AHEAD steps ahead and handed
//                           over by readlane, and no branch in the walk that differs between lanes.  Per member a lane reads 14
//                           bytes — its row of the base plane, of the six slot planes and of their seven weight planes — and
//                           keeps GPW_ACC = 44 counters in registers under constant indices: the six counts of gcols, ins_runs
//                           and ins_bases, the six sums of gwcols, the thirty of gwins.  Waves 1 .. GP_WAVES - 1 leave theirs in
//                           LDS, counter-major (3 x 44 x 64 words); wave 0 adds them in wave order and writes its row of the
//                           three tables, 32 + 32 + 128 bytes.  Integer sums in a fixed order, one writer per word, no atomics.
//                           gcols is what k_group_pile writes for the same groups, byte for byte.
// The call itself is the weighted mode of k_pile_call / k_pile_scan (ioc_pile_call.hip) over the group-segments.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ioc_group_pile_weighted.h"
#include "ioc_internal.h"

namespace {

constexpr int OP_WAVES = 4;  // pairs per workgroup of k_ops_project_weights (nothing is shared between them)
constexpr uint32_t SLOTS = IOC_PILE_INS_SLOTS;

__global__ void __launch_bounds__(64 * OP_WAVES)
k_ops_project_weights(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ end, const uint32_t* __restrict__ len,
                      const uint32_t* __restrict__ room, const uint32_t* __restrict__ ord, uint32_t cnt, const int64_t* __restrict__ row_base,
                      const uint32_t* __restrict__ q_off, const uint32_t* __restrict__ q_len, const uint64_t* __restrict__ plane,
                      const uint8_t* __restrict__ quals, uint64_t pool_bytes, uint8_t* __restrict__ weight_planes, uint64_t plane_bytes)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t x = blockIdx.x * OP_WAVES + (threadIdx.x >> 6);
    if (x >= cnt) return;  // (whole waves: there is no barrier below)
    const uint32_t pid = ord[x];
    const uint64_t L = len[pid], e = end[pid];
    if (L == 0 || L > room[pid] || L > e) return;  // came back without an answer: left to its re-run (as k_ops_project_ins has it)
    if (row_base[pid] < 0) return;                 // (piled and projected by an earlier run of this call already)
    const uint64_t qo = q_off[pid], po = plane[pid];
    // the pair's quality bytes, and how many of them lie inside the pool (all of them, unless the pair is not of this pool)
    const uint32_t qn = qo >= pool_bytes ? 0u : uint32_t(pool_bytes - qo < uint64_t(q_len[pid]) ? pool_bytes - qo : uint64_t(q_len[pid]));
    const uint8_t* qq = quals + qo;

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
            // (a byte outside the planes, a quality outside the pool: only a string that does not belong to its pair could ask for one)
            const uint64_t at_row = po + acc.row(lane);
            const uint32_t qp = acc.qpos(lane);
            if (at_row < plane_bytes) {
                if (acc.is_base(lane)) {
                    if (qp < qn) weight_planes[uint64_t(weight_plane_base()) * plane_bytes + at_row] = uint8_t(pile_qual_weight(qq[qp]));
                } else if (acc.is_del(lane)) {
                    weight_planes[uint64_t(weight_plane_base()) * plane_bytes + at_row] = uint8_t(acc.del_weight(lane, qn, qq));
                } else if (acc.is_ins(lane)) {
                    const uint32_t k = acc.ins_index(lane);
                    if (k < SLOTS && qp < qn) weight_planes[uint64_t(weight_plane_slot(k)) * plane_bytes + at_row] = uint8_t(pile_qual_weight(qq[qp]));
                }
            }
            acc.end_len();
            acc.end();
        }
        w = w_next;
    }
}

constexpr uint32_t GP_WAVES = IOC_GROUP_PILE_WAVES;
constexpr uint32_t GP_AHEAD = IOC_GROUP_PILE_AHEAD;
static_assert(GP_AHEAD == 64 && IOC_GROUP_PILE_FLIGHT == 2, "a lane per step of a chunk; the walk below takes the steps two by two");

struct GpwBytes {  // a member's fourteen plane bytes at a lane's row: base and slots, and the weight of each
    uint32_t b, sl[SLOTS], wb, wsl[SLOTS];
};

// the bytes at a lane's row p of the member whose planes start at `at0` (the same in every lane), or bytes that add nothing
__device__ __forceinline__ GpwBytes gpw_load(uint64_t at0, const uint8_t* __restrict__ base_planes, const uint8_t* __restrict__ slot_planes,
                                              const uint8_t* __restrict__ weight_planes, uint64_t plane_bytes, uint32_t p, bool live)
{
    GpwBytes v;
    v.b = group_pile_no_base(), v.wb = 0u;
#pragma unroll
    for (uint32_t j = 0; j < SLOTS; ++j) v.sl[j] = 0u, v.wsl[j] = 0u;
    if (at0 == group_pile_no_plane()) return v;  // (the same in every lane)
    const uint64_t at = at0 + p;
    if (live && at < plane_bytes) {
        v.b = base_planes[at];
        v.wb = weight_planes[uint64_t(weight_plane_base()) * plane_bytes + at];
#pragma unroll
        for (uint32_t j = 0; j < SLOTS; ++j) {
            v.sl[j] = slot_planes[uint64_t(j) * plane_bytes + at];
            v.wsl[j] = weight_planes[uint64_t(weight_plane_slot(j)) * plane_bytes + at];
        }
    }
    return v;
}

// lane `from`'s 64-bit value in every lane (`from`: the same in every lane)
__device__ __forceinline__ uint64_t gpw_readlane(uint64_t v, uint32_t from)
{
    const uint32_t lo = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v)), int(from)));
    const uint32_t hi = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v >> 32)), int(from)));
    return uint64_t(hi) << 32 | lo;
}

// one member's bytes into a lane's counters (constant indices throughout)
__device__ __forceinline__ void gpw_add(uint32_t (&acc)[GPW_ACC], const GpwBytes& m)
{
#pragma unroll
    for (uint32_t v = 0; v < 6u; ++v) {
        acc[GPW_COUNT + v] += uint32_t(plane_base_adds(m.b, v));
        acc[GPW_WBASE + v] += plane_base_weighs(m.b, m.wb, v);
    }
#pragma unroll
    for (uint32_t j = 0; j < SLOTS; ++j) {
        const uint32_t in = uint32_t(plane_slot_inserts(m.sl[j]));
        acc[GPW_BASES] += in;
        if (j == 0u) acc[GPW_RUNS] += in;
#pragma unroll
        for (uint32_t ch = 0; ch < 5u; ++ch) acc[GPW_WSLOT + j * 5u + ch] += plane_slot_weighs(m.sl[j], m.wsl[j], ch);
    }
}

__global__ void __launch_bounds__(64 * GP_WAVES)
k_group_pile_weighted(const IocGroupWork* __restrict__ work, uint32_t n_work, const IocPileSeg* __restrict__ gsegs, uint32_t n_gsegs,
                      const uint32_t* __restrict__ gmem_off, const uint32_t* __restrict__ gmembers, uint32_t n_members, uint32_t n_pairs,
                      const uint64_t* __restrict__ plane, const uint8_t* __restrict__ base_planes, const uint8_t* __restrict__ slot_planes,
                      const uint8_t* __restrict__ weight_planes, uint64_t plane_bytes, ioc_pileup_col* __restrict__ gcols,
                      ioc_pileup_col* __restrict__ gwcols, ioc_pileup_ins* __restrict__ gwins, uint64_t n_rows)
{
    __shared__ uint32_t part[(GP_WAVES - 1u) * GPW_ACC * 64u];
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

    uint32_t acc[GPW_ACC] = {};
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
            const GpwBytes cur = gpw_load(gpw_readlane(mine, s2), base_planes, slot_planes, weight_planes, plane_bytes, p, live);
            const GpwBytes nxt = gpw_load(s2 + 1u < n ? gpw_readlane(mine, s2 + 1u) : group_pile_no_plane(), base_planes, slot_planes, weight_planes,
                                          plane_bytes, p, live);
            gpw_add(acc, cur);
            gpw_add(acc, nxt);
        }
    }

    if (wave > 0u) {
        uint32_t* mine = part + size_t(wave - 1u) * GPW_ACC * 64u + lane;
#pragma unroll
        for (uint32_t k = 0; k < GPW_ACC; ++k) mine[plane_part_at(k)] = acc[k];
    }
    __syncthreads();
    if (wave > 0u) return;
#pragma unroll
    for (uint32_t w = 1; w < GP_WAVES; ++w) {  // (wave order: a fixed order of integer adds)
        const uint32_t* theirs = part + size_t(w - 1u) * GPW_ACC * 64u + lane;
#pragma unroll
        for (uint32_t k = 0; k < GPW_ACC; ++k) acc[k] += theirs[plane_part_at(k)];
    }
    const uint64_t row = uint64_t(s.row0) + p;
    if (!live || row >= n_rows) return;
    ioc_pileup_col col{}, wcol{};
    ioc_pileup_ins win{};
    col.a = acc[GPW_COUNT + 0u], col.c = acc[GPW_COUNT + 1u], col.g = acc[GPW_COUNT + 2u], col.t = acc[GPW_COUNT + 3u], col.other = acc[GPW_COUNT + 4u];
    col.del = acc[GPW_COUNT + 5u], col.ins_runs = acc[GPW_RUNS], col.ins_bases = acc[GPW_BASES];
    wcol.a = acc[GPW_WBASE + 0u], wcol.c = acc[GPW_WBASE + 1u], wcol.g = acc[GPW_WBASE + 2u], wcol.t = acc[GPW_WBASE + 3u], wcol.other = acc[GPW_WBASE + 4u];
    wcol.del = acc[GPW_WBASE + 5u];
#pragma unroll
    for (uint32_t j = 0; j < SLOTS; ++j)
#pragma unroll
        for (uint32_t ch = 0; ch < 5u; ++ch) win.slot[j][ch] = acc[GPW_WSLOT + j * 5u + ch];
    gcols[row] = col;
    gwcols[row] = wcol;
    gwins[row] = win;
}

}  // namespace

static_assert(sizeof(ioc_pileup_col) == 32 && sizeof(ioc_pileup_ins) == 128 && IOC_PILE_INS_SLOTS == 6, "the tables are laid out as the public records");

// The weights of the pairs ord[0 .. cnt) of a slice into the seven weight planes (plane_bytes each): pair pid's bytes from
// plane[pid] on of every plane, its quality bytes at quals + q_off[pid], q_len[pid] of them.  The arguments of iock_ops_project_ins
// otherwise; `buf` needs 3 readable bytes behind the slice's last region.
hipError_t iock_ops_project_weights(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room, const uint32_t* ord,
                                    uint32_t cnt, const int64_t* row_base, const uint32_t* q_off, const uint32_t* q_len, const uint64_t* plane,
                                    const uint8_t* quals, uint64_t pool_bytes, uint8_t* weight_planes, uint64_t plane_bytes)
{
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ops_project_weights, dim3((cnt + OP_WAVES - 1) / OP_WAVES), dim3(64 * OP_WAVES), 0, st, buf, end, len, room, ord, cnt, row_base,
                       q_off, q_len, plane, quals, pool_bytes, weight_planes, plane_bytes);
    return hipGetLastError();
}

// The three tables of the group-segments gsegs from the planes and the weight planes: the arguments of iock_group_pile, with the
// weight planes and gwcols / gwins (n_rows records each).  Rows no work item covers are not written: the caller has set the
// tables to 0.
hipError_t iock_group_pile_weighted(hipStream_t st, const IocGroupWork* work, uint32_t n_work, const IocPileSeg* gsegs, uint32_t n_gsegs, const uint32_t* gmem_off,
                                    const uint32_t* gmembers, uint32_t n_members, uint32_t n_pairs, const uint64_t* plane, const uint8_t* base_planes,
                                    const uint8_t* slot_planes, const uint8_t* weight_planes, uint64_t plane_bytes, ioc_pileup_col* gcols,
                                    ioc_pileup_col* gwcols, ioc_pileup_ins* gwins, uint64_t n_rows)
{
    if (n_work == 0) return hipSuccess;
    hipLaunchKernelGGL(k_group_pile_weighted, dim3(n_work), dim3(64 * GP_WAVES), 0, st, work, n_work, gsegs, n_gsegs, gmem_off, gmembers, n_members, n_pairs,
                       plane, base_planes, slot_planes, weight_planes, plane_bytes, gcols, gwcols, gwins, n_rows);
    return hipGetLastError();
}
