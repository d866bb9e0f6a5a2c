// ioc_plane_pile.hip — the pileup tables of ANY subset of a call's pairs, added up from the pairs' own byte planes after the
// alignments are gone: what the consensus of each side of a split is called from (ioc_planes_polish,
// ioc_align_pairs_split_polish; the definitions are ioc_host_ops_project_ins and ioc_host_planes_pile, ioc_align.cpp).
//
//   k_ops_project_ins   beside k_ops_project (ioc_pile_sites.hip), over the same bytes of a slice: one wave per pair repeats that
//                       kernel's walk (chunks of 64 aligned dwords, four steps of 64 bytes, PileAcc) with the run bookkeeping of
//                       the ins variant of k_ops_pileup (is_ins, ins_index, end_len).  The lane of an 'I' byte whose index j in its
//                       run is below IOC_PILE_INS_SLOTS stores 1 + the channel of its query base into slot plane j at the pair's
//                       row: [all slot-0 planes] .. [all slot-5 planes], plane_bytes each, a pair's bytes at its `plane` offset in
//                       every one of them.  A (slot, row) of a pair is consumed by one byte of its string, so every byte has one
//                       writer: plain byte stores, no atomics, and a re-run rewrites what it wrote.  No LDS, no scratch.
//   k_plane_pile        one workgroup of PP_WAVES waves per 64 rows of a group-segment that has reads; a lane owns a row.  The
//                       waves take the segment's members (ascending pairs, the split's list) interleaved, wave w the positions
//                       w, w + PP_WAVES, ..; a member counts where its group byte is the workgroup's — a test on scalars, the
//                       same in every lane.  Per member the lane reads its row of the base plane and of the six slot planes (the
//                       64 lanes read 64 consecutive bytes of each) and adds, by compare, into 6 + 30 counters that live in
//                       registers under constant indices.  Waves 1 .. PP_WAVES - 1 leave their counters in LDS, counter-major so
//                       that a wave's 64 lanes touch 64 consecutive words; wave 0 adds them in wave order, derives ins_runs (the
//                       sum of slot 0) and ins_bases (the sum of all slots) and writes its row of both tables.  Integer sums in a
//                       fixed order, one writer per word, no atomics: the tables do not depend on scheduling.
// The call itself is k_pile_call / k_pile_scan (ioc_pile_call.hip) over the group-segments; those kernels are not touched.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ioc_internal.h"
#include "ioc_ops_pileup.h"
#include "ioc_plane_pile.h"

namespace {

constexpr int OP_WAVES = 4;  // pairs per workgroup of k_ops_project_ins (nothing is shared between them)
constexpr uint32_t SLOTS = IOC_PILE_INS_SLOTS;

__global__ void __launch_bounds__(64 * OP_WAVES)
k_ops_project_ins(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ end, const uint32_t* __restrict__ len,
                  const uint32_t* __restrict__ room, const uint32_t* __restrict__ ord, uint32_t cnt, const int64_t* __restrict__ row_base,
                  const uint32_t* __restrict__ q_off, const uint64_t* __restrict__ plane, const uint8_t* __restrict__ pool, uint64_t pool_bytes,
                  uint8_t* __restrict__ slot_planes, uint64_t plane_bytes)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t x = blockIdx.x * OP_WAVES + (threadIdx.x >> 6);
    if (x >= cnt) return;  // (whole waves: there is no barrier below)
    const uint32_t pid = ord[x];
    const uint64_t L = len[pid], e = end[pid];
    if (L == 0 || L > room[pid] || L > e) return;  // came back without an answer: left to its re-run (as k_ops_project has it)
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
            if (acc.is_ins(lane)) {
                const uint64_t at_row = po + acc.row(lane), at = qo + acc.qpos(lane);
                const uint32_t k = acc.ins_index(lane);
                if (k < SLOTS && at_row < plane_bytes && at < pool_bytes)
                    slot_planes[uint64_t(k) * plane_bytes + at_row] = uint8_t(plane_slot_byte(PileAcc::channel(pool[at])));
            }
            acc.end_len();
            acc.end();
        }
        w = w_next;
    }
}

constexpr uint32_t PP_WAVES = IOC_PLANE_PILE_WAVES;
constexpr uint32_t PP_ACC = 6u + SLOTS * 5u;  // counters a lane keeps: the six of the base plane, five per slot

__global__ void __launch_bounds__(64 * PP_WAVES)
k_plane_pile(const IocPlaneWork* __restrict__ work, uint32_t n_work, const IocPileSeg* __restrict__ gsegs, const uint32_t* __restrict__ mem_off,
             const uint32_t* __restrict__ members, uint32_t n_pairs, const uint8_t* __restrict__ group, const uint64_t* __restrict__ plane,
             const uint8_t* __restrict__ base_planes, const uint8_t* __restrict__ slot_planes, uint64_t plane_bytes,
             ioc_pileup_col* __restrict__ gcols, ioc_pileup_ins* __restrict__ gins, uint64_t n_rows)
{
    __shared__ uint32_t part[(PP_WAVES - 1u) * PP_ACC * 64u];
    if (blockIdx.x >= n_work) return;  // (whole workgroups)
    const IocPlaneWork wk = work[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));  // (a scalar: the member walk below is one)
    const uint32_t g = wk.gseg >> 1, h = wk.gseg & 1u;
    const IocPileSeg s = gsegs[wk.gseg];
    const uint32_t p = wk.row + lane;
    const bool live = p <= uint32_t(s.rlen);
    const uint32_t m0 = mem_off[g], m1 = mem_off[g + 1u];

    uint32_t cb[6] = {0, 0, 0, 0, 0, 0};
    uint32_t cs[SLOTS][5] = {};
    for (uint32_t x = m0 + wave; x < m1; x += PP_WAVES) {
        const uint32_t i = members[x];
        if (i >= n_pairs || uint32_t(group[i]) != h) continue;  // (the same in every lane)
        const uint64_t at = plane[i] + p;
        if (!live || at >= plane_bytes) continue;  // (no barrier inside the walk)
        const uint32_t b = base_planes[at];
        uint32_t sl[SLOTS];
#pragma unroll
        for (uint32_t j = 0; j < SLOTS; ++j) sl[j] = slot_planes[uint64_t(j) * plane_bytes + at];
#pragma unroll
        for (uint32_t v = 0; v < 6u; ++v) cb[v] += uint32_t(plane_base_adds(b, v));
#pragma unroll
        for (uint32_t j = 0; j < SLOTS; ++j)
#pragma unroll
            for (uint32_t ch = 0; ch < 5u; ++ch) cs[j][ch] += uint32_t(plane_slot_adds(sl[j], ch));
    }

    if (wave > 0u) {
        uint32_t* mine = part + size_t(wave - 1u) * PP_ACC * 64u + lane;
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
    for (uint32_t w = 1; w < PP_WAVES; ++w) {  // (wave order: a fixed order of integer adds)
        const uint32_t* theirs = part + size_t(w - 1u) * PP_ACC * 64u + lane;
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

// Beside iock_ops_project, over the same slice and the same columns: what pair pid inserts goes into the six planes of
// slot_planes (plane_bytes bytes each, one behind the other) from byte plane[pid] of each on — reference length + 1 bytes of
// each, which the caller has set to 0 once.
hipError_t iock_ops_project_ins(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room,
                                const uint32_t* ord, uint32_t cnt, const int64_t* row_base, const uint32_t* q_off, const uint64_t* plane,
                                const uint8_t* pool, uint64_t pool_bytes, uint8_t* slot_planes, uint64_t plane_bytes)
{
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ops_project_ins, dim3((cnt + OP_WAVES - 1) / OP_WAVES), dim3(64 * OP_WAVES), 0, st, buf, end, len, room, ord, cnt, row_base,
                       q_off, plane, pool, pool_bytes, slot_planes, plane_bytes);
    return hipGetLastError();
}

// The tables of the group-segments gsegs (device; group-segment 2 g + h: the pairs members[mem_off[g] .. mem_off[g + 1]) whose
// group byte is h; row0 and rlen are read) from the planes: work item x is 64 rows of a group-segment, from `row` on.  Rows no
// work item covers are not written: the caller has set the tables (n_rows records each) to 0.
hipError_t iock_plane_pile(hipStream_t st, const IocPlaneWork* work, uint32_t n_work, const IocPileSeg* gsegs, const uint32_t* mem_off,
                           const uint32_t* members, uint32_t n_pairs, const uint8_t* group, const uint64_t* plane, const uint8_t* base_planes,
                           const uint8_t* slot_planes, uint64_t plane_bytes, ioc_pileup_col* gcols, ioc_pileup_ins* gins, uint64_t n_rows)
{
    if (n_work == 0) return hipSuccess;
    hipLaunchKernelGGL(k_plane_pile, dim3(n_work), dim3(64 * PP_WAVES), 0, st, work, n_work, gsegs, mem_off, members, n_pairs, group, plane,
                       base_planes, slot_planes, plane_bytes, gcols, gins, n_rows);
    return hipGetLastError();
}
