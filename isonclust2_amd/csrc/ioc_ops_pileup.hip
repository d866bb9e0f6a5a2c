// ioc_ops_pileup.hip — the pileup of the alignments of an emitting slice on their references, reduced where the walks left their
// bytes (ioc_align_pairs_pileup; the definition is ioc_host_ops_pileup, ioc_align.cpp), by count and, in the variant at the end of
// the file, by base quality as well.
//
// One wave per pair, over the pair's string as k_ops_stats reads it (ioc_ops_stats.hip): chunks of 64 aligned dwords with the next
// chunk's load in flight, four steps of 64 bytes per chunk, bit l of a ballot = position l, bytes outside the string masked to 0.
// A lane's reference position is the running one plus the popcount, below the lane, of the mask of the bytes that consume a
// reference base ("=XDd"); its query position the same with "=XIi" (PileAcc, ioc_ops_pileup.h).  A '=' / 'X' lane reads its query
// byte from the sequence pool and adds 1 to that base's word of its row, a 'D' lane to `del`; the 'I' bytes are added per piece
// of a run, by the piece's first lane.  Everything leaves through no-return integer atomics on the call's table: the sums do
// not depend on the order of arrival, so the table is reproducible bit for bit.  No LDS, no scratch.
//
// The device table is laid out as the public record (8 words per row), so that it is copied out as it stands.  In a run of '='
// the 64 lanes of an add touch 64 consecutive rows, 2 KB: 32 segments of 64 bytes with one word in each half — between the
// shapes measured for float atomics (256 contiguous bytes at full rate, 64 scattered rows 17 times slower).  Planes per channel
// would bring that down to 4 x 256 bytes or so and cost a transpose of the whole table at the end of the call; at one word per
// alignment column the adds of a full batch (27 M columns: 108 MB) are about a millisecond even at the scattered rate, beside
// alignments that take a hundred.  profiles/align_pileup.txt has the measured rate.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ioc_internal.h"
#include "ioc_ops_pileup.h"

namespace {

constexpr int OP_WAVES = 4;  // pairs per workgroup (nothing is shared between them)
constexpr uint32_t INS_WORDS = sizeof(ioc_pileup_ins) / 4, INS_LONGER = IOC_PILE_INS_SLOTS * 5;  // ioc_pileup_ins in words

__device__ __forceinline__ void pile_add(uint32_t* word, uint32_t v)
{
    (void)__hip_atomic_fetch_add(word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (result unused: the no-return form)
}

// INS: the variant of ioc_align_pairs_polish, which adds what the 'I' bytes insert into a second table as well (ioc_pileup_ins:
// 32 words per row), one add per 'I' byte, by its index in its run and its query base.
template <bool INS>
__global__ void __launch_bounds__(64 * OP_WAVES)
k_ops_pileup(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ end, const uint32_t* __restrict__ len,
             const uint32_t* __restrict__ room, const uint32_t* __restrict__ ord, uint32_t cnt, const int64_t* __restrict__ row_base,
             const uint32_t* __restrict__ q_off, const uint8_t* __restrict__ pool, uint64_t pool_bytes, uint32_t* __restrict__ cols,
             uint64_t n_rows, uint32_t* __restrict__ ins)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t x = blockIdx.x * OP_WAVES + (threadIdx.x >> 6);
    if (x >= cnt) return;  // (whole waves: there is no barrier below)
    const uint32_t pid = ord[x];
    const uint64_t L = len[pid], e = end[pid];
    if (L == 0 || L > room[pid] || L > e) return;  // came back without an answer: left to its re-run (as k_ops_stats has it)
    const int64_t rb = row_base[pid];
    if (rb < 0) return;  // (added by an earlier run of this call already)
    const uint64_t qo = q_off[pid];

    const uint8_t* first = buf + (e - L);
    const uint32_t head = uint32_t(reinterpret_cast<uintptr_t>(first) & 3u);
    const uint32_t* words = reinterpret_cast<const uint32_t*>(first - head);
    const uint32_t span = head + uint32_t(L);  // bytes from the aligned-down address to the string's end (L < 2^27)
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
            // (a row outside the table, a base outside the pool: only a string that does not belong to its pair could ask for one)
            const uint64_t row = uint64_t(rb) + acc.row(lane);
            if (row < n_rows) {
                uint32_t* rec = cols + row * PILE_WORDS;
                if (acc.is_base(lane)) {
                    const uint64_t at = qo + acc.qpos(lane);
                    if (at < pool_bytes) pile_add(rec + PileAcc::channel(pool[at]), 1u);
                } else if (acc.is_del(lane)) {
                    pile_add(rec + PILE_DEL, 1u);
                } else if (const uint32_t piece = acc.ins_piece(lane)) {
                    pile_add(rec + PILE_INS_BASES, piece);
                    if (acc.run_start(lane)) pile_add(rec + PILE_INS_RUNS, 1u);
                }
                if (INS && acc.is_ins(lane)) {
                    const uint64_t at = qo + acc.qpos(lane);
                    const uint32_t j = acc.ins_index(lane);
                    if (at < pool_bytes)
                        pile_add(ins + row * INS_WORDS + (j < uint32_t(IOC_PILE_INS_SLOTS) ? j * 5u + PileAcc::channel(pool[at]) : INS_LONGER), 1u);
                }
            }
            if (INS) acc.end_len();
            acc.end();
        }
        w = w_next;
    }
}

// The weighted variant (ioc_align_pairs_polish_weighted; "k_ops_pileup<weighted>" in the trace line).  It is a kernel of its own
// and repeats the walk above, so that the two instantiations of k_ops_pileup stay the code they were, instruction for instruction
// (as one template with the weights compiled out they were scheduled differently: profiles/align_polish_weighted.txt).  The adds
// of the first table as above, so that `cols` is bit-identical, and the weights of ioc_host_ops_pileup_weighted into two tables
// of their own: beside the add of a base or a 'D' its weight into the same word of wcols — one more atomic word per event — and
// per 'I' byte its weight into wins, where the ins variant adds 1 into ins, which this variant does not keep.  A base or 'I'
// lane reads its quality byte at the pool offset of its query base, a 'D' lane those of its one or two neighbours
// (PileAcc::del_weight) within the pair's q_len bytes and within the pool.  A lane touches two or three records of its row (32 B
// cols, 32 B wcols, 128 B wins), laid out as the public ones and copied out as they stand.
__global__ void __launch_bounds__(64 * OP_WAVES)
k_ops_pileup_weighted(const uint8_t* __restrict__ buf, const uint64_t* __restrict__ end, const uint32_t* __restrict__ len,
                      const uint32_t* __restrict__ room, const uint32_t* __restrict__ ord, uint32_t cnt, const int64_t* __restrict__ row_base,
                      const uint32_t* __restrict__ q_off, const uint32_t* __restrict__ q_len, const uint8_t* __restrict__ pool,
                      const uint8_t* __restrict__ quals, uint64_t pool_bytes, uint32_t* __restrict__ cols, uint32_t* __restrict__ wcols,
                      uint32_t* __restrict__ wins, uint64_t n_rows)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t x = blockIdx.x * OP_WAVES + (threadIdx.x >> 6);
    if (x >= cnt) return;  // (whole waves: there is no barrier below)
    const uint32_t pid = ord[x];
    const uint64_t L = len[pid], e = end[pid];
    if (L == 0 || L > room[pid] || L > e) return;
    const int64_t rb = row_base[pid];
    if (rb < 0) return;
    const uint64_t qo = q_off[pid];
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
            const uint64_t row = uint64_t(rb) + acc.row(lane);
            if (row < n_rows) {  // (the same guards as above: the row inside the tables, the base inside the pool)
                uint32_t* rec = cols + row * PILE_WORDS;
                uint32_t* wrec = wcols + row * PILE_WORDS;
                if (acc.is_base(lane)) {
                    const uint64_t at = qo + acc.qpos(lane);
                    if (at < pool_bytes) {
                        const uint32_t ch = PileAcc::channel(pool[at]);
                        pile_add(rec + ch, 1u);
                        pile_add(wrec + ch, pile_qual_weight(quals[at]));
                    }
                } else if (acc.is_del(lane)) {
                    pile_add(rec + PILE_DEL, 1u);
                    pile_add(wrec + PILE_DEL, acc.del_weight(lane, qn, qq));
                } else if (const uint32_t piece = acc.ins_piece(lane)) {
                    pile_add(rec + PILE_INS_BASES, piece);
                    if (acc.run_start(lane)) pile_add(rec + PILE_INS_RUNS, 1u);
                }
                if (acc.is_ins(lane)) {  // (every 'I' has its own slot and its own weight: no piece to merge)
                    const uint64_t at = qo + acc.qpos(lane);
                    const uint32_t j = acc.ins_index(lane);
                    if (at < pool_bytes)
                        pile_add(wins + row * INS_WORDS + (j < uint32_t(IOC_PILE_INS_SLOTS) ? j * 5u + PileAcc::channel(pool[at]) : INS_LONGER),
                                 pile_qual_weight(quals[at]));
                }
            }
            acc.end_len();
            acc.end();
        }
        w = w_next;
    }
}

}  // namespace

static_assert(sizeof(ioc_pileup_col) == PILE_WORDS * 4, "the device table is laid out as the public record");

// The pairs ord[0 .. cnt) of a slice (device pair ids) add into `cols` (n_rows records): pair pid into the rows from
// row_base[pid] on (negative: the pair is skipped), its query at pool + q_off[pid].  room[pid]: query length + reference length.
// The dword that holds a string's last byte is read whole: `buf` needs 3 readable bytes behind the slice's last region.
hipError_t iock_ops_pileup(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room,
                           const uint32_t* ord, uint32_t cnt, const int64_t* row_base, const uint32_t* q_off, const uint8_t* pool,
                           uint64_t pool_bytes, ioc_pileup_col* cols, uint64_t n_rows)
{
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ops_pileup<false>, dim3((cnt + OP_WAVES - 1) / OP_WAVES), dim3(64 * OP_WAVES), 0, st, buf, end, len, room, ord, cnt,
                       row_base, q_off, pool, pool_bytes, reinterpret_cast<uint32_t*>(cols), n_rows, static_cast<uint32_t*>(nullptr));
    return hipGetLastError();
}

static_assert(sizeof(ioc_pileup_ins) == 128 && offsetof(ioc_pileup_ins, longer) == INS_LONGER * 4, "the second table is laid out as the public record");

// ... and into `ins` (n_rows records) what they insert (ioc_host_ops_pileup_ins): the variant ioc_align_pairs_polish runs
hipError_t iock_ops_pileup_ins(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room,
                               const uint32_t* ord, uint32_t cnt, const int64_t* row_base, const uint32_t* q_off, const uint8_t* pool,
                               uint64_t pool_bytes, ioc_pileup_col* cols, ioc_pileup_ins* ins, uint64_t n_rows)
{
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ops_pileup<true>, dim3((cnt + OP_WAVES - 1) / OP_WAVES), dim3(64 * OP_WAVES), 0, st, buf, end, len, room, ord, cnt,
                       row_base, q_off, pool, pool_bytes, reinterpret_cast<uint32_t*>(cols), n_rows, reinterpret_cast<uint32_t*>(ins));
    return hipGetLastError();
}

// ... and the weights of the same events into wcols / wins (ioc_host_ops_pileup_weighted) under the pool's quality bytes `quals`
// (pool_bytes of them); q_len[pid]: the pair's query length.  The variant ioc_align_pairs_polish_weighted runs.
hipError_t iock_ops_pileup_weighted(hipStream_t st, const uint8_t* buf, const uint64_t* end, const uint32_t* len, const uint32_t* room,
                                    const uint32_t* ord, uint32_t cnt, const int64_t* row_base, const uint32_t* q_off, const uint32_t* q_len,
                                    const uint8_t* pool, const uint8_t* quals, uint64_t pool_bytes, ioc_pileup_col* cols,
                                    ioc_pileup_col* wcols, ioc_pileup_ins* wins, uint64_t n_rows)
{
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ops_pileup_weighted, dim3((cnt + OP_WAVES - 1) / OP_WAVES), dim3(64 * OP_WAVES), 0, st, buf, end, len, room, ord, cnt,
                       row_base, q_off, q_len, pool, quals, pool_bytes, reinterpret_cast<uint32_t*>(cols), reinterpret_cast<uint32_t*>(wcols),
                       reinterpret_cast<uint32_t*>(wins), n_rows);
    return hipGetLastError();
}
