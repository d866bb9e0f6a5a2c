// ioc_align_gpu.hip — batched semi-global affine alignment on the GPU for the sahlin / furious fallback
// (getBestClusterAln, src/cluster.cpp:461-515: ParasailAlign :408-423 + getAlnRatio :442-459).
//
// The reference needs the alignment only for ONE number: how many k-windows of the comparison string
// hold at least floor((1-e)k) matches (getAlnRatio).  Two device formulations, both bit-identical to the
// host aligner (ioc_align.cpp: same recurrence, strict-`>` tie-breaks, end-cell choice):
//
//  * "trace" (default) — what parasail_sg_trace does, without its O(n*m) traceback matrix:
//      pass 1  k_align_fwd    score-only Gotoh DP (~10 VALU per cell), which also drops CHECKPOINTS: (H, F)
//                             of every 256th row and (H, E) of every 256th column, and finds the end cell;
//      pass 2  k_align_trace  walks back from the end cell one 256 x 256 tile at a time: the tile's
//                             direction nibbles are recomputed in LDS from its top-row / left-column
//                             checkpoints, the walk feeds the comparison bits (in reverse order) into the
//                             sliding window counter.  Only ~(n + m) / 256 * 2 tiles are ever recomputed.
//  * "carry" (IOC_ALIGN_VARIANT=carry) — single pass, every DP state carries the window statistics of its
//      best path (~39 VALU per cell); kept as an independent cross-check of the trace variant.
//      It has no walk: ioc_align_pairs_ops (the alignment itself as an operation string, written by the emitting variants of the
//      walk kernels: OpsOut below) takes the trace formulation whatever IOC_ALIGN_VARIANT says.
//
// Mapping of the forward passes: one workgroup per pair, NT = 64 * waves threads.  Thread g owns C
// consecutive columns of a strip of NT * C columns and walks down the rows skewed by g (systolic wavefront):
// at step s it computes row s - g.  Its right-edge (H, E) and the query base move to thread g + 1 by one DPP
// wave shift (through LDS between waves, one barrier per step).
//
// This file: the kernels, the launches and whatever needs the context.  What a call decides on the host before it launches — bands,
// corridors, couples, slices, tile counts, version 1's waves and arena — and the records host and kernels share: ioc_align_plan.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "ioc_align_plan.h"
#include "ioc_align_sink.h"
#include "ioc_internal.h"

namespace {

constexpr int ALN_NEG = INT32_MIN / 4;
constexpr uint32_t ALN_LEN_SHIFT = 26;  // window statistics word: [31:26] min(len, k), [25:0] qualifying windows

struct St {  // one DP state: score + statistics of its best path
    int s;
    uint32_t b, c;
};

__device__ __forceinline__ uint32_t spaces_c(uint32_t g, uint32_t k, int il)
{
    // g end-gap columns (all ' '): len = min(g, k); a window of blanks qualifies iff 0 >= ilimit
    const uint32_t len = g < k ? g : k;
    const uint32_t cnt = (il <= 0 && g > k) ? g - k : 0u;
    return (len << ALN_LEN_SHIFT) | cnt;
}

// append one comparison character (bit = mbit for '|', 0 for ' ') to a path's statistics.
// hb = 64 - ilimit (ilimit clamped to 0..33): popc(window) + hb has bit 6 set iff popc >= ilimit, so the
// "window qualifies" test is two plain ALU ops and never touches VCC.
// GEN: paths shorter than k may exist (top-left k x k corner of the matrix only).
template <bool GEN>
__device__ __forceinline__ void append(uint32_t& b, uint32_t& c, uint32_t bit, uint32_t hb, uint32_t k)
{
    const uint32_t hit = (uint32_t(__popc(b)) + hb) >> 6;  // 0 or 1
    if (GEN) {
        const bool full = (c >> ALN_LEN_SHIFT) >= k;
        c += full ? hit : (1u << ALN_LEN_SHIFT);
    } else {
        c += hit;
    }
    b = (b << 1) | bit;
}

// value of the left neighbour lane (lane 0 keeps its own): one DPP move instead of an LDS permute
__device__ __forceinline__ uint32_t from_left(uint32_t v)
{
    return uint32_t(__builtin_amdgcn_update_dpp(int(v), int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}

// same, lane 0 takes `first` (its own copy of it) instead: the strip's left edge enters the wave here
__device__ __forceinline__ uint32_t from_left_or(uint32_t v, uint32_t first)
{
    return uint32_t(__builtin_amdgcn_update_dpp(int(first), int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}

__device__ __forceinline__ uint8_t comp_base(uint8_t ch)
{
    return ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : ch;
}

template <bool GEN>
__device__ __forceinline__ void row_cells(St (&Hp)[ALN_C], St (&F)[ALN_C], const uint32_t (&rpk)[ALN_C / 4], St& hl,
                                          St& el, St dg, uint32_t qc, int go, uint32_t hb, const AlnParams& P)
{
#pragma unroll
    for (int c = 0; c < ALN_C; ++c) {
        // E: gap in the query (horizontal move) from the cell on the left
        St E;
        {
            const int eo = hl.s - go, ee = el.s - P.gap_extend;
            const bool ex = ee > eo;
            E.s = ex ? ee : eo;
            E.b = ex ? el.b : hl.b;
            E.c = ex ? el.c : hl.c;
            append<GEN>(E.b, E.c, 0u, hb, P.k);
        }
        // F: gap in the reference (vertical move) from the cell above
        St Fn;
        {
            const int fo = Hp[c].s - go, fe = F[c].s - P.gap_extend;
            const bool fx = fe > fo;
            Fn.s = fx ? fe : fo;
            Fn.b = fx ? F[c].b : Hp[c].b;
            Fn.c = fx ? F[c].c : Hp[c].c;
            append<GEN>(Fn.b, Fn.c, 0u, hb, P.k);
        }
        St h;
        {
            const bool mt = qc == ((rpk[c >> 2] >> (8 * (c & 3))) & 0xFFu);
            h.s = dg.s + (mt ? P.match : P.mismatch);
            h.b = dg.b;
            h.c = dg.c;
            append<GEN>(h.b, h.c, mt ? P.mbit : 0u, hb, P.k);
        }
        if (E.s > h.s) h = E;
        if (Fn.s > h.s) h = Fn;
        dg = Hp[c];
        Hp[c] = h;
        F[c] = Fn;
        hl = h;
        el = E;
    }
}

__global__ void __launch_bounds__(64 * ALN_MAXW, 3)
k_align_carry(const AlnPairDev* __restrict__ pairs, const uint32_t* __restrict__ order, const uint8_t* __restrict__ pool,
        AlnParams P, uint32_t* __restrict__ bnd, uint64_t bnd_stride, uint32_t* __restrict__ lrow,
        uint64_t lrow_stride, int32_t* __restrict__ out_score, uint32_t* __restrict__ out_count)
{
    __shared__ uint32_t xb[2][ALN_MAXW][8];
    __shared__ uint32_t s_look[7][64];
    __shared__ uint32_t s_lc[4];
    const uint32_t pid = order[blockIdx.x];
    const AlnPairDev pr = pairs[pid];
    const uint32_t n = pr.n, m = pr.m;
    const int go = pr.gap_open, il = pr.ilimit;
    const uint32_t hb = uint32_t(64 - (il < 0 ? 0 : il > 33 ? 33 : il));
    const uint8_t* __restrict__ q = pool + pr.q_off;
    const uint8_t* __restrict__ r = pool + pr.r_off;
    const uint32_t NT = blockDim.x;
    const uint32_t g = threadIdx.x, lane = g & 63u, wave = g >> 6, nwaves = NT >> 6;
    uint32_t* mybnd = bnd + uint64_t(blockIdx.x) * bnd_stride;    // [2][6][n]
    uint32_t* mylrow = lrow + uint64_t(blockIdx.x) * lrow_stride;  // [entries][4]
    const uint32_t strip_cols = NT * ALN_C;
    const uint32_t nstrips = (m + strip_cols - 1) / strip_cols;
    const uint32_t nsteps = n + NT - 1;
    if (g == 0) {
        s_lc[0] = uint32_t(ALN_NEG);
        s_lc[1] = s_lc[2] = s_lc[3] = 0;
    }

    for (uint32_t p = 0; p < nstrips; ++p) {
        const uint32_t jb = p * strip_cols + g * ALN_C;  // columns to the left of this thread's block
        uint32_t rpk[ALN_C / 4];  // this thread's reference bytes, 4 per register; 0 (never a base) beyond the end
#pragma unroll
        for (int c4 = 0; c4 < ALN_C / 4; ++c4) {
            uint32_t w = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t j = jb + c4 * 4 + e;
                uint32_t ch = 0;
                if (j < m) ch = pr.rc ? comp_base(r[m - 1 - j]) : r[j];
                w |= ch << (8 * e);
            }
            rpk[c4] = w;
        }
        St Hp[ALN_C], F[ALN_C];
#pragma unroll
        for (int c = 0; c < ALN_C; ++c) {
            Hp[c].s = 0;  // row 0: free leading gap, jb + c + 1 blank columns
            Hp[c].b = 0;
            Hp[c].c = spaces_c(jb + c + 1, P.k, il);
            F[c].s = ALN_NEG;
            F[c].b = 0;
            F[c].c = 0;
        }
        St dg{0, 0u, spaces_c(jb, P.k, il)};  // H(0, jb)
        const int lastc = (m - 1 >= jb && m - 1 < jb + ALN_C) ? int(m - 1 - jb) : -1;
        St bc{ALN_NEG, 0u, 0u};
        uint32_t bc_i = 0;
        const bool corner_cols = jb < P.k;
        const uint32_t* bin = mybnd + uint64_t((p + 1) & 1u) * 6u * n;  // written by strip p-1
        uint32_t* bout = mybnd + uint64_t(p & 1u) * 6u * n;
        const bool write_edge = (g == NT - 1) && (p + 1 < nstrips);

        // wave 0 looks ahead in blocks of 64 rows — the query bytes and (strips > 0) the left-edge records:
        // loaded one block early into registers, published to LDS when the block becomes current; lane 0
        // (the only consumer) picks one row per step
        uint32_t qn = 0, en[6] = {0, 0, 0, 0, 0, 0};
        St out_h{0, 0u, 0u}, out_e{ALN_NEG, 0u, 0u};
        uint32_t out_q = 0;
        for (uint32_t s = 0; s < nsteps; ++s) {
            if (wave == 0 && (s & 63u) == 0) {
                if (s == 0) {
                    const uint32_t row = lane;
                    qn = row < n ? q[row] : 0u;
                    if (p > 0) {
#pragma unroll
                        for (int w = 0; w < 6; ++w) en[w] = row < n ? bin[uint64_t(w) * n + row] : 0u;
                    }
                }
                s_look[6][lane] = qn;
#pragma unroll
                for (int w = 0; w < 6; ++w) s_look[w][lane] = en[w];
                const uint32_t row = s + 64u + lane;
                qn = row < n ? q[row] : 0u;
                if (p > 0) {
#pragma unroll
                    for (int w = 0; w < 6; ++w) en[w] = row < n ? bin[uint64_t(w) * n + row] : 0u;
                }
            }
            // inputs of this step: what the left neighbour produced in the previous step
            St hl, el;
            uint32_t qc;
            hl.s = int(from_left(uint32_t(out_h.s)));
            hl.b = from_left(out_h.b);
            hl.c = from_left(out_h.c);
            el.s = int(from_left(uint32_t(out_e.s)));
            el.b = from_left(out_e.b);
            el.c = from_left(out_e.c);
            qc = from_left(out_q);
            if (lane == 0) {
                if (wave > 0) {
                    const uint32_t* x = xb[(s + 1) & 1u][wave - 1];
                    hl.s = int(x[0]);
                    hl.b = x[1];
                    hl.c = x[2];
                    el.s = int(x[3]);
                    el.b = x[4];
                    el.c = x[5];
                    qc = x[6];
                } else {
                    const uint32_t sl = s & 63u;
                    qc = s_look[6][sl];
                    if (p == 0) {
                        hl.s = 0;  // column 0: free leading gap of s + 1 blank columns
                        hl.b = 0;
                        hl.c = spaces_c(s + 1, P.k, il);
                        el.s = ALN_NEG;
                        el.b = 0;
                        el.c = 0;
                    } else {
                        hl.s = int(s_look[0][sl]);
                        hl.b = s_look[1][sl];
                        hl.c = s_look[2][sl];
                        el.s = int(s_look[3][sl]);
                        el.b = s_look[4][sl];
                        el.c = s_look[5][sl];
                    }
                }
            }
            const int i = int(s) - int(g);
            const bool active = i >= 0 && uint32_t(i) < n;
            if (active) {
                const St hl_in = hl;
                if (corner_cols && uint32_t(i) < P.k)
                    row_cells<true>(Hp, F, rpk, hl, el, dg, qc, go, hb, P);
                else
                    row_cells<false>(Hp, F, rpk, hl, el, dg, qc, go, hb, P);
                dg = hl_in;
                if (lastc >= 0) {  // one thread of the last strip: best of the last column, first row wins ties
                    St hm = Hp[0];
#pragma unroll
                    for (int c = 1; c < ALN_C; ++c)
                        if (c == lastc) hm = Hp[c];
                    if (hm.s > bc.s) {
                        bc = hm;
                        bc_i = uint32_t(i) + 1u;
                    }
                }
                if (write_edge) {
                    bout[0ull * n + uint32_t(i)] = uint32_t(hl.s);
                    bout[1ull * n + uint32_t(i)] = hl.b;
                    bout[2ull * n + uint32_t(i)] = hl.c;
                    bout[3ull * n + uint32_t(i)] = uint32_t(el.s);
                    bout[4ull * n + uint32_t(i)] = el.b;
                    bout[5ull * n + uint32_t(i)] = el.c;
                }
                if (uint32_t(i) == n - 1) {
                    // last row: this thread's best cell, first column wins ties
                    St br{ALN_NEG, 0u, 0u};
                    uint32_t bj = 0;
#pragma unroll
                    for (int c = 0; c < ALN_C; ++c) {
                        if (jb + c < m && Hp[c].s > br.s) {
                            br = Hp[c];
                            bj = jb + c + 1;
                        }
                    }
                    uint32_t* e = mylrow + uint64_t(p * NT + g) * 4u;
                    e[0] = uint32_t(br.s);
                    e[1] = bj;
                    e[2] = br.b;
                    e[3] = br.c;
                }
            }
            out_h = hl;
            out_e = el;
            out_q = qc;
            if (lane == 63 && wave + 1 < nwaves) {
                uint32_t* x = xb[s & 1u][wave];
                x[0] = uint32_t(hl.s);
                x[1] = hl.b;
                x[2] = hl.c;
                x[3] = uint32_t(el.s);
                x[4] = el.b;
                x[5] = el.c;
                x[6] = qc;
            }
            if (nwaves > 1) __syncthreads();
        }
        if (lastc >= 0) {
            s_lc[0] = uint32_t(bc.s);
            s_lc[1] = bc_i;
            s_lc[2] = bc.b;
            s_lc[3] = bc.c;
        }
        __syncthreads();
    }

    // end cell: best of the last column (rows ascending), replaced only by a strictly larger cell of the
    // last row (columns ascending from 0) — the host aligner's scan order (ioc_align.cpp)
    if (wave == 0) {
        St br{0, 0u, spaces_c(n, P.k, il)};  // H(n, 0)
        uint32_t bj = 0;
        const uint32_t entries = nstrips * NT;
        for (uint32_t e = lane; e < entries; e += 64) {
            const uint32_t* x = mylrow + uint64_t(e) * 4u;
            const int s = int(x[0]);
            const uint32_t j = x[1];
            if (s > br.s || (s == br.s && j < bj)) {
                br.s = s;
                bj = j;
                br.b = x[2];
                br.c = x[3];
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const int s = __shfl_xor(br.s, o);
            const uint32_t j = __shfl_xor(bj, o), b = __shfl_xor(br.b, o), c = __shfl_xor(br.c, o);
            if (s > br.s || (s == br.s && j < bj)) {
                br.s = s;
                bj = j;
                br.b = b;
                br.c = c;
            }
        }
        if (lane == 0) {
            St fin{int(s_lc[0]), s_lc[2], s_lc[3]};
            uint32_t bi = s_lc[1], bjj = m;
            if (br.s > fin.s) {
                fin = br;
                bi = n;
                bjj = bj;
            }
            // trailing end gaps: (m - bj) + (n - bi) blanks
            const uint32_t gtrail = (m - bjj) + (n - bi);
            const uint32_t t = gtrail < P.k ? gtrail : P.k;
            for (uint32_t x = 0; x < t; ++x) append<true>(fin.b, fin.c, 0u, hb, P.k);
            uint32_t cnt = fin.c & ((1u << ALN_LEN_SHIFT) - 1u);
            if (il <= 0) cnt += gtrail - t;
            out_score[pid] = fin.s;
            out_count[pid] = cnt;
        }
    }
}

// ---- "trace" variant ------------------------------------------------------------------------------
constexpr int TR_C = TILE / 64;  // columns per lane in the traceback tile (one wave per pair)

__device__ __forceinline__ uint32_t ref_byte(const uint8_t* __restrict__ r, uint32_t m, uint32_t rc, uint32_t j)
{
    if (j >= m) return 0u;  // never equals a base
    return rc ? comp_base(r[m - 1 - j]) : r[j];
}

// The forward pass works on SLANTED scores: X*(i, j) = X(i, j) + ge * (i + j) for X in {H, E, F}, and keeps
// Hq = H* - (go - ge) instead of H*.  Extending a gap then costs nothing (the slant pays the ge), opening
// one is the "- (go - ge)" already folded into Hq, and a diagonal step adds match + 2 ge or mismatch + 2 ge:
//     E*(i, j) = max(E*(i, j-1), Hq(i, j-1))          F*(i, j) = max(F*(i-1, j), Hq(i-1, j))
//     H*(i, j) = max3(Hq(i-1, j-1) + (s + 2 ge + go - ge), E*, F*)
// 7 VALU per cell instead of 10; true values (checkpoints, end cell) are X* - ge * (i + j).
// tail launch of the forward pass: a pair split over `groups` workgroups (see k_align_fwd)
struct AlnCross {
    uint32_t groups = 1;       // workgroups per pair (1: the usual launch)
    uint32_t first_wg = 0;     // first workgroup of the launch that belongs to a split pair
    uint32_t first_pair = 0;   // ... and the pair (position in `order`) it starts with
    uint32_t flag_stride = 0;  // flags per pair
    uint32_t* flags = nullptr; // [pair][band][strip]: the band's checkpoints of the strip are out
    int2* best = nullptr;      // [pair][band]: best cell of the band's part of the last column
    uint32_t* err = nullptr;   // a wait ran out
};

struct FwdConst {
    int gd;      // go - ge
    int cm, cx;  // match / mismatch + 2 ge + gd
    int ge;
};

// An opaque copy of a per-lane value: address / predicate / slant arithmetic derived from it inside a
// rarely taken block stays inside that block instead of being hoisted out of the step loop into dozens of
// long-lived registers.
__device__ __forceinline__ uint32_t opaque(uint32_t v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// PROF: the diagonal increment (cm for identical bases, cx otherwise) comes as one byte per column out of
// the lane's QUERY PROFILE in LDS — per strip, for each of A C G T (and "anything else"), the 16 increments
// of the lane's 16 columns packed four to a word; `xw` holds the row of this query base.  One add with a
// byte-select operand instead of compare + select + add: 5 VALU per cell.
template <int C, bool PROF>
__device__ __forceinline__ void fwd_cells(int (&Hq)[C], int (&F)[C], const uint32_t (&rpk)[C / 4], int& hql, int& el,
                                          int dgq, uint32_t qc, const FwdConst& K)
{
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int E = max(el, hql);
        const int Fn = max(F[c], Hq[c]);
        int inc;
        if (PROF) {
            inc = int((rpk[c >> 2] >> (8 * (c & 3))) & 0xFFu);  // rpk = the profile row here
        } else {
            const bool mt = qc == ((rpk[c >> 2] >> (8 * (c & 3))) & 0xFFu);
            inc = mt ? K.cm : K.cx;
        }
        const int hq = max(max(dgq + inc, E), Fn) - K.gd;
        dgq = Hq[c];
        Hq[c] = hq;
        F[c] = Fn;
        hql = hq;
        el = E;
    }
}

// Pass 1: scores only.  A strip is 64 * FW_C = 1024 columns (a multiple of TILE, so its right edge IS a
// column checkpoint and the next strip reads its left edge from there); one WAVE walks a strip top to
// bottom, FW_R rows per step, its lanes skewed by one step: the right edge (Hq, E*) and the query bases
// of a lane reach the next lane by one DPP wave shift — no LDS, no barrier inside a strip.
// The waves of a workgroup split the ROWS into bands of whole tiles and run the (band, strip) grid as a
// pipeline: wave b does strip p in round p + b, taking its top edge from the row checkpoint band b - 1
// wrote one round earlier.  One barrier per round (~4000 steps) instead of one per step: waves of one pair
// share SIMDs with other pairs' waves, and per-step lockstep cost 30 % of the throughput.
constexpr int FW_R = 4;
static_assert(FW_C == 16, "the last-column select tree assumes 16 (or, narrow last strip, 8) columns per lane");
static_assert(FW_R == 4, "the look-ahead hands 4 rows per step to lane 0 (one 16-byte LDS read per field)");

#ifndef IOC_FWD_WAVES_PER_EU
#define IOC_FWD_WAVES_PER_EU 3
#endif
#ifndef IOC_FWD_NARROW_LAST
#define IOC_FWD_NARROW_LAST 1
#endif
#ifndef IOC_TR_STEP_UNROLL
#define IOC_TR_STEP_UNROLL 2
#endif
#ifndef IOC_FWD_STEP_UNROLL
#define IOC_FWD_STEP_UNROLL 4
#endif
template <bool PROF>
__global__ void __launch_bounds__(64 * ALN_MAXW) __attribute__((amdgpu_waves_per_eu(IOC_FWD_WAVES_PER_EU, 8)))
k_align_fwd(const AlnPairDev* __restrict__ pairs, const uint32_t* __restrict__ order, uint32_t count, uint32_t wpp_main,
            uint32_t n_main, uint32_t wpp_tail, const uint8_t* __restrict__ pool, AlnParams P, int2* ck, const AlnCk* __restrict__ cko, int2* lrow,
            uint64_t lrow_stride, int4* __restrict__ ends, AlnCross X)
{
    // A workgroup is 4 (or 8) waves = one per SIMD of its CU, however the dispatcher places workgroups; it
    // carries (waves / wpp) pairs, each split over wpp waves ("bands").  (Workgroups of 2 waves were seen
    // sharing SIMDs while others idled.)
    __shared__ __attribute__((aligned(16))) uint32_t s_look_all[ALN_MAXW][3][128];
    __shared__ int s_best[ALN_MAXW][2];
    __shared__ uint32_t s_rounds;
    // PROF: query profile of the current strip, [wave][base code 0..4][lane][4 words]
    __shared__ __attribute__((aligned(16))) uint32_t s_prof_all[PROF ? ALN_MAXW : 1][5][64][4];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));  // uniform: keep the band in SGPRs
    // The first n_main workgroups (one resident generation of the chip) split their pairs over wpp_main waves;
    // the ones after them — dispatched as those retire — over wpp_tail >= wpp_main waves, so that the tail
    // generation, which runs on a half-empty chip, is over sooner.
    const bool tail = blockIdx.x >= n_main;
    const uint32_t wpp = tail ? wpp_tail : wpp_main, wg_waves = blockDim.x >> 6;
    // X.groups > 1 (the tail launch): a pair is split over X.groups WORKGROUPS of 4 waves, band = 4 * group + wave;
    // the band below another workgroup's last band takes its top edges when that band's flag says they are there
    // (X.first_wg: the workgroups before it are ordinary ones of the same launch — the split pairs then start on
    // whatever CU frees up first; a workgroup only ever waits for one with a smaller index, dispatched before it)
    const bool cross = X.groups > 1 && blockIdx.x >= X.first_wg;
    const uint32_t xb = cross ? blockIdx.x - X.first_wg : 0u;
    const uint32_t grp = cross ? xb % X.groups : 0u;
    const uint32_t slot = cross ? 0u : wv / wpp, wave = cross ? grp * wg_waves + wv : wv % wpp, nwaves = cross ? X.groups * wg_waves : wpp;
    const uint32_t pslot = cross ? X.first_pair + xb / X.groups
                         : tail  ? n_main * (wg_waves / wpp_main) + (blockIdx.x - n_main) * (wg_waves / wpp_tail) + slot
                                 : blockIdx.x * (wg_waves / wpp_main) + slot;  // pair of this wave, in `order`
    const bool live = pslot < count;
    if (threadIdx.x == 0) s_rounds = 0;
    __syncthreads();
    const uint32_t pid = order[live ? pslot : 0];
    const AlnPairDev pr = pairs[pid];
    const uint32_t n = pr.n, m = pr.m;
    FwdConst K;
    K.ge = P.gap_extend;
    K.gd = pr.gap_open - P.gap_extend;
    K.cm = P.match + 2 * P.gap_extend + K.gd;
    K.cx = P.mismatch + 2 * P.gap_extend + K.gd;
    const uint8_t* __restrict__ q = pool + pr.q_off;
    const uint8_t* __restrict__ r = pool + pr.r_off;
    int2* rowck = ck + cko[pid].row_off;
    int2* colck = ck + cko[pid].col_off;
    int2* mylrow = lrow + uint64_t(live ? pslot : 0) * lrow_stride;
    uint32_t(*s_look)[128] = s_look_all[wv];
    uint32_t(*s_prof)[64][4] = s_prof_all[PROF ? wv : 0];
    // what travels with a row: the query byte, or (PROF) the word offset of its profile row
    auto qcode = [](uint32_t ch) -> uint32_t {
        if (!PROF) return ch;
        const uint32_t code = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
        return code * 256u;
    };
    constexpr uint32_t strip_cols = 64u * FW_C;
    const uint32_t nstrips = (m + strip_cols - 1) / strip_cols;
    const bool narrow_last = IOC_FWD_NARROW_LAST && m - (nstrips - 1u) * strip_cols <= strip_cols / 2u;  // (uniform) see `strip`
    // this wave's band of rows [r_lo, r_hi), whole tiles
    const uint32_t ntiles = (n + TILE - 1) / TILE, tpb = (ntiles + nwaves - 1) / nwaves;
    const uint32_t r_lo = min(n, wave * tpb * TILE), r_hi = min(n, (wave + 1u) * tpb * TILE);
    const uint32_t nblocks = (r_hi - r_lo + FW_R - 1) / FW_R;  // row blocks of the band
    const uint32_t nsteps = nblocks + 63u;
    const bool last_band = r_hi == n && r_lo < n;
    int bc = ALN_NEG;  // best of the last column inside this band (true score), first row wins ties
    uint32_t bc_i = 0;

    // the pairs of a workgroup may need different numbers of rounds: everybody stays for the barriers
    uint32_t* xflag = cross ? X.flags + uint64_t(live ? pslot - X.first_pair : 0) * X.flag_stride : nullptr;  // [band][strip]
    bool xbad = false;
    if (live && lane == 0) atomicMax(&s_rounds, nstrips + nwaves - 1u);
    __syncthreads();
    const uint32_t rounds = s_rounds;
    for (uint32_t round = 0; round < rounds; ++round) {
        const int ps = int(round) - int(wave);
        if (live && ps >= 0 && uint32_t(ps) < nstrips && nblocks > 0) {
            const uint32_t p = uint32_t(ps);
            if (cross && wv == 0 && wave > 0) {
                // the band above lives in another workgroup: wait for its row checkpoint of this strip (bounded:
                // the launch keeps all its workgroups resident, but a wait without an end could take the GPU down)
                uint32_t seen = 0;
                if (lane == 0 && !xbad) {
                    for (uint32_t it = 0; it < (1u << 22); ++it) {
                        seen = __hip_atomic_load(&xflag[uint64_t(wave - 1u) * nstrips + p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (seen) break;
                        if ((it & 1023u) == 1023u && __hip_atomic_load(X.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;  // somebody gave up
                        __builtin_amdgcn_s_sleep(8);
                    }
                    if (!seen) atomicOr(X.err, 1u);
                }
                seen = uint32_t(__builtin_amdgcn_readfirstlane(int(seen)));
                if (!seen) xbad = true;
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            }
            // The strip with C columns per lane: 16, or — the last strip of a pair when no more than half a strip of
            // columns is left — 8: a step then costs 45 + 4 x 8 x 5 instructions instead of 45 + 4 x 16 x 5 for the same
            // number of steps (m = 16.6 kb: 17 strips, the last one 283 columns wide on average — 18 of 64 lanes busy).
            auto strip = [&](auto cc) __attribute__((always_inline)) {
            constexpr int C = decltype(cc)::value;
            const uint32_t jb = p * strip_cols + lane * uint32_t(C);  // columns to the left of this lane's block
            uint32_t rpk[C / 4];
#pragma unroll
            for (int c4 = 0; c4 < C / 4; ++c4) {
                uint32_t w = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) w |= ref_byte(r, m, pr.rc, jb + c4 * 4 + e) << (8 * e);
                rpk[c4] = w;
            }
            if (PROF) {
                const uint32_t bases = 'A' | ('C' << 8) | ('G' << 16) | ('T' << 24);
#pragma unroll
                for (int code = 0; code < 5; ++code) {
                    const uint32_t b = code < 4 ? (bases >> (8 * code)) & 0xFFu : 0x100u;  // 0x100: equals no byte
#pragma unroll
                    for (int c4 = 0; c4 < C / 4; ++c4) {
                        uint32_t w = 0;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            w |= uint32_t(((rpk[c4] >> (8 * e)) & 0xFFu) == b ? K.cm : K.cx) << (8 * e);
                        s_prof[code][lane][c4] = w;
                    }
                }
            }
            // Hq and F* of the row above the band (slanted, see fwd_cells): row 0 of the matrix (free leading
            // gap, H = 0) or the row checkpoint the band above wrote in the previous round
            int Hp[C], F[C];
            int dg;
            if (r_lo == 0) {
                const int base = K.ge * int(jb) - K.gd;  // per-column parts (ge * c) are scalar
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    Hp[c] = base + K.ge * (c + 1);
                    F[c] = ALN_NEG;
                }
                dg = base;
            } else {
                const int* roh = reinterpret_cast<const int*>(rowck + uint64_t(r_lo / TILE - 1) * row_pitch(m));
                const int* rof = roh + row_pitch(m);
#pragma unroll
                for (int c = 0; c < C; ++c) {  // row checkpoints hold the slanted (Hq, F*)
                    const int2 v = (jb + c < m) ? int2{roh[jb + c], rof[jb + c]} : int2{0, 0};
                    Hp[c] = v.x;
                    F[c] = v.y;
                }
                dg = (jb > 0 && jb <= m) ? roh[jb - 1] : K.ge * int(r_lo) - K.gd;  // column 0 holds H = 0
            }
            const bool has_cols = jb < m;
            const int lastc = (m - 1 >= jb && m - 1 < jb + uint32_t(C)) ? int(m - 1 - jb) : -1;
            const bool strip_has_lastc = uint64_t(p + 1u) * strip_cols >= m;  // (uniform) the last strip
            // this lane's right edge is a column checkpoint (lane 63: the next strip's input)
            const uint32_t jr = jb + uint32_t(C);
            const bool wr_col = (jr % TILE) == 0 && jr < m;
            int2* colout = wr_col ? colck + uint64_t(jr / TILE - 1) * col_pitch(n) : colck;
            const int2* colin = p ? colck + uint64_t(p * strip_cols / TILE - 1) * col_pitch(n) : colck;
            // look-ahead in blocks of 64 rows — the query bytes and the strip's left edge (Hq, E*): column 0
            // of the matrix (H = 0, no gap to extend) or the column checkpoint, slanted
            auto left_edge = [&](uint32_t row) {
                int2 v{K.ge * int(row + 1) - K.gd, ALN_NEG};
                if (p > 0 && row < r_hi) v = colin[row];  // checkpoints hold the slanted (Hq, E*) as passed between lanes
                return v;
            };
            uint32_t qn = 0;
            int2 en{0, 0};
            int hl[FW_R], el[FW_R];  // inputs of the step from the left; after the step: this lane's right edge
            uint32_t qc[FW_R];
#pragma unroll
            for (int rr = 0; rr < FW_R; ++rr) {
                hl[rr] = 0;
                el[rr] = ALN_NEG;
                qc[rr] = 0;
            }
            // Look-ahead of the left edge + query, 64 rows at a time, one block AHEAD of its use in a 128-row
            // ring in LDS; every lane reads the 4 rows of the NEXT step from there (one address for the whole
            // wave, a step before they are needed) and lane 0 picks them up as the `old` operand of the DPP shift.
            auto publish = [&](uint32_t blk) {
                s_look[0][(blk & 1u) * 64u + lane] = uint32_t(en.x);
                s_look[1][(blk & 1u) * 64u + lane] = uint32_t(en.y);
                s_look[2][(blk & 1u) * 64u + lane] = qn;
            };
            auto fetch = [&](uint32_t blk) {
                const uint32_t row = r_lo + blk * 64u + lane;
                qn = qcode(row < r_hi ? q[row] : 0u);
                en = left_edge(row);
            };
            fetch(0);
            publish(0);
            fetch(1);
            uint4 nxh, nxe, nxq;  // inputs of lane 0 for the coming step
            {
                nxh = *reinterpret_cast<const uint4*>(&s_look[0][0]);
                nxe = *reinterpret_cast<const uint4*>(&s_look[1][0]);
                nxq = *reinterpret_cast<const uint4*>(&s_look[2][0]);
            }
            // one step of the wave; the loop below runs two per iteration (the compiler cannot unroll a loop with wave-level
            // operations by itself): half of the register copies that carry the inputs from step to step go away
            auto step = [&](const uint32_t s) __attribute__((always_inline)) {
                if ((s & (64 / FW_R - 1)) == 0) {  // steps 16 b .. : publish block b + 1, fetch block b + 2
                    const uint32_t blk = s / (64 / FW_R) + 1u;
                    publish(blk);
                    fetch(blk + 1u);
                }
                {
                    const uint32_t h4[FW_R] = {nxh.x, nxh.y, nxh.z, nxh.w}, e4[FW_R] = {nxe.x, nxe.y, nxe.z, nxe.w},
                                   q4[FW_R] = {nxq.x, nxq.y, nxq.z, nxq.w};
#pragma unroll
                    for (int rr = 0; rr < FW_R; ++rr) {
                        hl[rr] = int(from_left_or(uint32_t(hl[rr]), h4[rr]));
                        el[rr] = int(from_left_or(uint32_t(el[rr]), e4[rr]));
                        qc[rr] = from_left_or(qc[rr], q4[rr]);
                    }
                    const uint32_t nx = ((s + 1u) * FW_R) & 127u;  // rows of the next step
                    nxh = *reinterpret_cast<const uint4*>(&s_look[0][nx]);
                    nxe = *reinterpret_cast<const uint4*>(&s_look[1][nx]);
                    nxq = *reinterpret_cast<const uint4*>(&s_look[2][nx]);
                }
                const int bi = int(s) - int(lane);  // row block of this lane in this step
                if (bi >= 0 && uint32_t(bi) < nblocks && has_cols) {
                    const uint32_t i0 = r_lo + uint32_t(bi) * FW_R;
                    // rows past the end (last block of the last band) run on a query byte of 0 and are never looked at
                    // wave-uniform: the special path is right for every lane (its extras are guarded per lane), and a wave whose
                    // lanes disagree would run BOTH copies of the cells — in the last strip, where one lane owns the last
                    // column, for every step of the strip
                    // (in scalar terms: a lane of the strip owns the last column, or some lane — s - lane for a lane 0..63 — is on
                    // the last row block of the last band)
                    const bool special = strip_has_lastc || (last_band && s + 1u >= nblocks && s + 1u - nblocks < 64u);
                    if (!special) {
#pragma unroll
                        for (int rr = 0; rr < FW_R; ++rr) {
                            const int hl_in = hl[rr];
                            if (PROF) {
                                const uint4 x = *reinterpret_cast<const uint4*>(&s_prof[0][0][0] + qc[rr] + lane * 4u);
                                const uint32_t x4[4] = {x.x, x.y, x.z, x.w};
                                uint32_t xw[C / 4];
#pragma unroll
                                for (int c4 = 0; c4 < C / 4; ++c4) xw[c4] = x4[c4];
                                fwd_cells<C, true>(Hp, F, xw, hl[rr], el[rr], dg, qc[rr], K);
                            } else {
                                fwd_cells<C, false>(Hp, F, rpk, hl[rr], el[rr], dg, qc[rr], K);
                            }
                            dg = hl_in;
                        }
                    } else {
#pragma unroll
                        for (int rr = 0; rr < FW_R; ++rr) {
                            const int hl_in = hl[rr];
                            if (PROF) {
                                const uint4 x = *reinterpret_cast<const uint4*>(&s_prof[0][0][0] + qc[rr] + lane * 4u);
                                const uint32_t x4[4] = {x.x, x.y, x.z, x.w};
                                uint32_t xw[C / 4];
#pragma unroll
                                for (int c4 = 0; c4 < C / 4; ++c4) xw[c4] = x4[c4];
                                fwd_cells<C, true>(Hp, F, xw, hl[rr], el[rr], dg, qc[rr], K);
                            } else {
                                fwd_cells<C, false>(Hp, F, rpk, hl[rr], el[rr], dg, qc[rr], K);
                            }
                            dg = hl_in;
                            const uint32_t i = i0 + rr;  // 0-based row
                            if (i < r_hi) {
                                if (lastc >= 0) {
                                    // Hp[lastc] by a select tree over the bits of lastc (4 conditions, not 15)
                                    const uint32_t lc = opaque(uint32_t(lastc));
                                    // (written out: an index computed in a loop makes the compiler move Hp to LDS)
                                    const bool b0 = lc & 1u, b1 = lc & 2u, b2 = lc & 4u, b3 = lc & 8u;
                                    const int s0 = b0 ? Hp[1] : Hp[0], s1 = b0 ? Hp[3] : Hp[2], s2 = b0 ? Hp[5] : Hp[4],
                                              s3 = b0 ? Hp[7] : Hp[6];
                                    const int u0 = b1 ? s1 : s0, u1 = b1 ? s3 : s2;
                                    int hm = b2 ? u1 : u0;
                                    if constexpr (C == 16) {
                                        const int s4 = b0 ? Hp[9] : Hp[8], s5 = b0 ? Hp[11] : Hp[10], s6 = b0 ? Hp[13] : Hp[12],
                                                  s7 = b0 ? Hp[15] : Hp[14];
                                        const int u2 = b1 ? s5 : s4, u3 = b1 ? s7 : s6;
                                        const int v1 = b2 ? u3 : u2;
                                        hm = b3 ? v1 : hm;
                                    }
                                    hm += K.gd - K.ge * int(opaque(i) + 1 + m);  // true H(i + 1, m)
                                    if (hm > bc) {
                                        bc = hm;
                                        bc_i = i + 1u;
                                    }
                                }
                                if (i + 1u == n) {  // last row: this lane's best cell, first column wins ties
                                    int br = ALN_NEG;
                                    uint32_t bj = 0;
                                    const uint32_t jbo = opaque(jb);
                                    const int base = K.gd - K.ge * int(n + jbo);
#pragma unroll
                                    for (int c = 0; c < C; ++c) {
                                        const int ht = Hp[c] + base - K.ge * (c + 1);  // true H(n, jb + c + 1)
                                        if (jbo + c < m && ht > br) {
                                            br = ht;
                                            bj = jbo + c + 1;
                                        }
                                    }
                                    mylrow[p * 64u + lane] = int2{br, int(bj)};
                                }
                            }
                        }
                    }
                    if (wr_col) {
                        if (!special) {  // i0 is a multiple of 4: two 16-byte stores
                            int4* co = reinterpret_cast<int4*>(colout + i0);
                            co[0] = int4{hl[0], el[0], hl[1], el[1]};
                            co[1] = int4{hl[2], el[2], hl[3], el[3]};
                        } else {
#pragma unroll
                            for (int rr = 0; rr < FW_R; ++rr)
                                if (i0 + rr < r_hi) colout[i0 + rr] = int2{hl[rr], el[rr]};
                        }
                    }
                    const uint32_t i1 = i0 + FW_R;  // DP index of the block's last row (TILE is a multiple of FW_R)
                    if ((i1 % TILE) == 0 && i1 < n) {
                        const uint32_t jbo = opaque(jb);
                        // two planes (Hq, F*): each lane's 16 values go out as they sit in its registers.  The offset from the
                        // pair's (uniform) row region is a 32-bit number of ints (the launcher refuses pairs whose region is
                        // larger): scalar base + one vector offset instead of 64-bit vector address arithmetic in a block
                        // that two lanes of every wave take in every step
                        const uint32_t pitch32 = uint32_t(row_pitch(m));
                        int* rb = reinterpret_cast<int*>(rowck) + ((i1 / TILE - 1u) * (2u * pitch32) + jbo);
                        int4* roh = reinterpret_cast<int4*>(rb);
                        int4* rof = reinterpret_cast<int4*>(rb + pitch32);
#pragma unroll
                        for (int c = 0; c < C; c += 4) {
                            roh[c / 4] = int4{Hp[c], Hp[c + 1], Hp[c + 2], Hp[c + 3]};
                            rof[c / 4] = int4{F[c], F[c + 1], F[c + 2], F[c + 3]};
                        }
                    }
                }
            };
            {
                uint32_t s = 0;
#if IOC_FWD_STEP_UNROLL == 8
                for (; s + 7u < nsteps; s += 8) {
                    step(s);
                    step(s + 1u);
                    step(s + 2u);
                    step(s + 3u);
                    step(s + 4u);
                    step(s + 5u);
                    step(s + 6u);
                    step(s + 7u);
                }
#endif
#if IOC_FWD_STEP_UNROLL >= 4
                for (; s + 3u < nsteps; s += 4) {
                    step(s);
                    step(s + 1u);
                    step(s + 2u);
                    step(s + 3u);
                }
#endif
#if IOC_FWD_STEP_UNROLL >= 2
                for (; s + 1u < nsteps; s += 2) {
                    step(s);
                    step(s + 1u);
                }
#endif
                for (; s < nsteps; ++s) step(s);
            }
            // the lane that owns the last column hands the band's best to lane 0 (a strip of the last round)
            if (lastc >= 0) {
                s_best[wv][0] = bc;
                s_best[wv][1] = int(bc_i);
                if (cross) X.best[uint64_t(pslot - X.first_pair) * nwaves + wave] = int2{bc, int(bc_i)};
            }
            };
            if (narrow_last && p + 1u == nstrips)
                strip(std::integral_constant<int, 8>{});
            else
                strip(std::integral_constant<int, FW_C>{});
            if (cross) {  // this band's checkpoints of the strip are out: tell the band below (and the final reduction)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                if (lane == 0) __hip_atomic_store(&xflag[uint64_t(wave) * nstrips + p], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (rounds > 1 || nwaves > 1) __syncthreads();  // orders this round's checkpoints before the next round reads them
    }
    __syncthreads();

    // end cell: best of the last column (rows ascending), replaced only by a strictly larger cell of the
    // last row (columns ascending from 0) — the host aligner's scan order (ioc_align.cpp)
    if (xbad && lane == 0) atomicOr(X.err, 1u);
    const bool reducer = cross ? (grp + 1u == X.groups && wv == 0) : wave == 0;
    if (live && reducer) {
        if (cross) {  // every band that has rows has finished its last strip?
            uint32_t okf = 1;
            if (lane == 0) {
                for (uint32_t b2 = 0; b2 < nwaves && okf; ++b2) {
                    if (min(n, b2 * tpb * TILE) >= n) break;
                    uint32_t seen = 0;
                    for (uint32_t it = 0; it < (1u << 22); ++it) {
                        seen = __hip_atomic_load(&xflag[uint64_t(b2) * nstrips + (nstrips - 1u)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (seen) break;
                        __builtin_amdgcn_s_sleep(8);
                    }
                    if (!seen) okf = 0;
                }
                if (!okf) atomicOr(X.err, 1u);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        int br = 0;  // H(n, 0)
        uint32_t bj = 0;
        for (uint32_t e = lane; e < nstrips * 64u; e += 64) {
            {   // entry e = (strip, lane): lanes right of the matrix wrote nothing
                const uint32_t ep = e >> 6, el = e & 63u;
                const uint32_t cpl = (narrow_last && ep + 1u == nstrips) ? 8u : uint32_t(FW_C);
                if (uint64_t(ep) * strip_cols + el * cpl >= m) continue;
            }
            const int2 x = mylrow[e];
            if (x.x > br || (x.x == br && uint32_t(x.y) < bj)) {
                br = x.x;
                bj = uint32_t(x.y);
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const int s = __shfl_xor(br, o);
            const uint32_t j = __shfl_xor(bj, o);
            if (s > br || (s == br && j < bj)) {
                br = s;
                bj = j;
            }
        }
        if (lane == 0) {
            int fin = ALN_NEG;
            uint32_t bi = 0, bjj = m;
            for (uint32_t b2 = 0; b2 < nwaves; ++b2) {  // bands top to bottom: the first row wins ties
                if (min(n, b2 * tpb * TILE) >= n) break;
                const int2 bb = cross ? X.best[uint64_t(pslot - X.first_pair) * nwaves + b2] : int2{s_best[slot * wpp + b2][0], s_best[slot * wpp + b2][1]};
                if (bb.x > fin) {
                    fin = bb.x;
                    bi = uint32_t(bb.y);
                }
            }
            if (br > fin) {
                fin = br;
                bi = n;
                bjj = bj;
            }
            ends[pid] = int4{fin, int(bi), int(bjj), 0};
        }
    }
}

// sliding k-window counter over the comparison string, fed in REVERSE order: getAlnRatio counts the
// windows [i, i + k) for i = 0 .. len - k - 1, i.e. every window but the last one — in reverse order,
// every window but the first one to complete.
struct WinStat {
    uint32_t wb = 0, pushed = 0, cnt = 0;
    __device__ __forceinline__ void push(uint32_t bit, uint32_t kmask, uint32_t k, int il)
    {
        wb = ((wb << 1) | bit) & kmask;
        ++pushed;
        if (pushed > k && int(__popc(wb)) >= il) ++cnt;
    }
    // m <= 64 pushes at once, bit x of `bits` = the x-th character pushed; every lane gets the same arguments
    // and lane x evaluates the window as it stands after push x
    __device__ __forceinline__ void push_run(unsigned long long bits, uint32_t m, uint32_t kmask, uint32_t k, int il, uint32_t lane)
    {
        // the characters up to push `lane`, the latest in bit 0 (as the window keeps them)
        const unsigned long long upto = __brevll(bits << (63u - lane));
        const unsigned long long old = lane + 1u < 64u ? (unsigned long long)wb << (lane + 1u) : 0ull;
        const uint32_t win = uint32_t(old | upto) & kmask;
        const bool hit = lane < m && pushed + lane + 1u > k && int(__popc(win)) >= il;
        cnt += uint32_t(__popcll(__ballot(hit)));
        wb = uint32_t(__builtin_amdgcn_readlane(int(win), int(m - 1u)));
        pushed += m;
    }
    __device__ __forceinline__ void blanks(uint32_t g, uint32_t kmask, uint32_t k, int il)
    {
        const uint32_t t = g < k ? g : k;
        for (uint32_t x = 0; x < t; ++x) push(0u, kmask, k, il);
        if (g > t) {  // the window is all blanks from here on
            const uint32_t rest = g - t;
            const uint32_t first_counted = pushed >= k ? 0u : k - pushed;  // pushes until pushed > k holds
            pushed += rest;
            if (il <= 0 && rest > first_counted) cnt += rest - first_counted;
        }
    }
};

// ioc_align_pairs_ops: where the walks write the alignment itself.  A pair's operation bytes ('=' 'X' 'I' 'D', end gaps 'i' 'd':
// ioc_host_align_ops) go DOWNWARDS from the end of its region of query length + reference length bytes — the walk runs
// backwards, so the bytes stand in forward order at the region's end — and the count comes out beside score and windows.
struct AlnOpsDev {
    uint8_t* buf;
    const uint64_t* end;  // per pair: one past the last byte of its region
    uint32_t* len;        // per pair: bytes written (0: the pair came back without an answer)
};

// The hooks of an emitting walk, beside the window counter's (push_run, push, blanks).  EMIT false: an empty object whose calls are
// nothing at all — the walk's code is what it was.  The cursor is the same in every lane; global memory directly, plain vector
// stores, no LDS.
struct NoOpsDev {};
template <bool EMIT>
struct OpsOut {
    using Dev = NoOpsDev;
    __device__ __forceinline__ void begin(Dev, uint32_t, uint32_t) {}
    __device__ __forceinline__ void run(unsigned long long, uint32_t, uint32_t) {}
    __device__ __forceinline__ void step(uint8_t, uint32_t) {}
    __device__ __forceinline__ void fill(uint8_t, uint32_t, uint32_t) {}
    __device__ __forceinline__ void end(Dev, uint32_t, uint32_t) {}
    __device__ __forceinline__ void none(Dev, uint32_t) {}
};
template <>
struct OpsOut<true> {
    using Dev = AlnOpsDev;
    uint8_t* cur = nullptr;  // the lowest byte written so far
    uint8_t* lo = nullptr;   // the region's first byte.  A walk never gets there before it ends — every column takes a base of the
                             // query's or the reference's — unless it runs on a forward pass that was given up (a wait ran out: the
                             // host throws the slice away): nothing is stored below `lo` then either.
    __device__ __forceinline__ void begin(const Dev& od, uint32_t pid, uint32_t room)
    {
        cur = od.buf + od.end[pid];
        lo = cur - room;
    }
    // a run of m <= 64 diagonal moves, bit x of `bits` = the x-th of them (in walk order) joins equal bases: one store by the wave
    __device__ __forceinline__ void run(unsigned long long bits, uint32_t m, uint32_t lane)
    {
        if (lane < m && cur - 1 - lane >= lo) cur[-1 - int(lane)] = (bits >> lane) & 1ull ? uint8_t('=') : uint8_t('X');
        cur -= m;
    }
    __device__ __forceinline__ void step(uint8_t op, uint32_t lane)  // one E ('D') or F ('I') move
    {
        if (lane == 0 && cur > lo) cur[-1] = op;
        cur -= 1;
    }
    __device__ __forceinline__ void fill(uint8_t op, uint32_t g, uint32_t lane)  // g end-gap columns: a strided fill by the wave
    {
        const uint64_t room = uint64_t(cur > lo ? cur - lo : 0);
        for (uint32_t x = lane; x < g && x < room; x += 64) cur[-1 - int64_t(x)] = op;
        cur -= g;
    }
    __device__ __forceinline__ void end(const Dev& od, uint32_t pid, uint32_t lane)
    {
        if (lane == 0) od.len[pid] = cur >= lo ? uint32_t((od.buf + od.end[pid]) - cur) : 0xFFFFFFFFu;
    }
    __device__ __forceinline__ void none(const Dev& od, uint32_t pid) { od.len[pid] = 0u; }  // (one lane: the pair has no answer)
};

// Pass 2: one wave per pair.  Direction nibble of a cell: bits 0-1 = where H came from (0 diagonal with
// identical bases, 3 diagonal with different bases, 1 E, 2 F), bit 2 = E extended, bit 3 = F extended.
constexpr int TR_WAVES = 4;
// what a barrier is to a one-wave workgroup: LDS operations of a wave complete in order, the compiler must not move them
__device__ __forceinline__ void tr_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

#define ALN_TRACE_KERNEL k_align_trace
#define ALN_TRACE_EMIT 0
#include "ioc_align_trace.inc"
#undef ALN_TRACE_KERNEL
#undef ALN_TRACE_EMIT
// the emitting variant (ioc_align_pairs_ops)
#define ALN_TRACE_KERNEL k_align_trace_ops
#define ALN_TRACE_EMIT 1
#include "ioc_align_trace.inc"
#undef ALN_TRACE_KERNEL
#undef ALN_TRACE_EMIT

// per sequence: does it hold a byte other than A C G T?  (The query-profile kernel knows four bases; a pair
// with anything else — the host aligner matches any two equal bytes — takes the comparing kernel.)
__global__ void __launch_bounds__(256)
k_seq_flags(const uint8_t* __restrict__ pool, const int64_t* __restrict__ offs, uint8_t* __restrict__ flags)
{
    __shared__ uint32_t s_any;
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    const int64_t a = offs[blockIdx.x], b = offs[blockIdx.x + 1];
    uint32_t any = 0;
    for (int64_t i = a + threadIdx.x; i < b; i += 256) {
        const uint8_t ch = pool[i];
        any |= (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') ? 1u : 0u;
    }
    if (any) s_any = 1;
    __syncthreads();
    if (threadIdx.x == 0) flags[blockIdx.x] = uint8_t(s_any);
}

#include "ioc_align_v2.inc"

// ---- host side ----------------------------------------------------------------------------------------------------------

// the device time of the first `used` events' slices, into ms_align_fwd / ms_align_trace
void add_elapsed(ioc_ctx* c, const std::vector<hipEvent_t>& evs, size_t used)
{
    for (size_t x = 0; x + 2 < used && x + 2 < evs.size(); x += 3) {
        float a = 0, b = 0;
        if (hipEventElapsedTime(&a, evs[x], evs[x + 1]) == hipSuccess) c->tm.ms_align_fwd += a;
        if (hipEventElapsedTime(&b, evs[x + 1], evs[x + 2]) == hipSuccess) c->tm.ms_align_trace += b;
    }
}

// IOC_TRACE=1: the host's wall-clock between the stages of a call on stderr (developer aid, like the driver's PhaseTrace in
// ioc_host.cpp; profiles/step_gaps.txt).  A mark takes no synchronisation: a stage that waits for the device says so in its name.
struct StageTrace {
    bool on = getenv("IOC_TRACE") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void mark(const char* what)
    {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[ioc]     align %-24s %9.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

int compute_units(const ioc_ctx* c)
{
    int n_cu = 256;
    (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device);
    return n_cu < 1 ? 256 : n_cu;
}

// half of what is free (the checkpoint arena's own reservation counted as free), or IOC_ALIGN_CK_BUDGET_MB.  `held`: bytes the
// call holds beside the arena for its whole length (a pileup call's table) — counted as free, then taken off the budget.
int ck_budget(ioc_ctx* c, uint64_t* budget, uint64_t held = 0)
{
    size_t free_b = 0, total_b = 0;
    IOC_CHK(c, hipMemGetInfo(&free_b, &total_b));
    *budget = (uint64_t(free_b + c->a_ck.cap) + held) / 2;
    if (const char* e = getenv("IOC_ALIGN_CK_BUDGET_MB")) *budget = uint64_t(atoll(e)) << 20;
    *budget -= std::min(*budget, held);
    return IOC_OK;
}

// ---- the operation bytes of an emitting call (ioc_align_pairs_ops) ------------------------------------------------------

// (the caller's side, indexed by the caller's pair: AlnSink, ioc_align_sink.h)

// One run's side (version 2's, version 1's).  The pairs of a slice get consecutive regions of ONE device buffer, as large as the
// largest slice needs — its bytes count against the checkpoint arena's budget (slice_couples, plan_v1) — and the buffer is
// copied out after every slice.
struct OpsRun {
    const AlnSink* host;
    const uint32_t* back;       // device pair -> caller's pair
    std::vector<uint64_t> end;  // per device pair: the end of its region within its slice's bytes
    AlnOpsDev dev{};
    std::vector<uint8_t> stage;
    std::vector<uint32_t> len;
    std::vector<uint32_t> room;        // (statistics) per device pair: query length + reference length ...
    const uint32_t* d_room = nullptr;  // ... and where that table is on the device
    std::vector<ioc_aln_stats> recs;   // (statistics) a slice's records, in the slice's order
    std::vector<int64_t> row_base;     // (pileup) per device pair: its first row, -1 for a pair that has been added already ...
    std::vector<uint32_t> q_off;       // ... and where its query starts in the pool
    const int64_t* d_row_base = nullptr;
    const uint32_t* d_q_off = nullptr;
    std::vector<uint32_t> q_len;  // (weighted pileup, a pile that projects the weights) per device pair: its query's length
    const uint32_t* d_q_len = nullptr;
    std::vector<uint64_t> plane;  // (a pile that projects) per device pair: where its planes start
    const uint64_t* d_plane = nullptr;
};

// the buffer [end per pair][len per pair][the bytes of a slice] and the table of ends (after o.end is filled); the columns a
// reduced sink adds, and the spare bytes behind the slice's: OpsLayout
int ops_reserve(ioc_ctx* c, OpsRun& o, uint64_t max_slice_bytes, const std::vector<AlnPairDev>& dp)
{
    const AlnSink& h = *o.host;
    const size_t np = o.end.size();
    const OpsLayout lay = h.layout(np);
    const int r = ioc_reserve(c, c->a_ops, lay.bytes + size_t(max_slice_bytes) + lay.spare);
    if (r != IOC_OK) return r;
    uint8_t* p = static_cast<uint8_t*>(c->a_ops.p);
    o.dev = AlnOpsDev{p + lay.bytes, reinterpret_cast<const uint64_t*>(p + lay.end), reinterpret_cast<uint32_t*>(p + lay.len)};
    IOC_CHK(c, hipMemcpyAsync(p + lay.end, o.end.data(), np * 8, hipMemcpyHostToDevice, c->stream));
    if (h.reduced()) {
        o.room.resize(np);
        for (size_t x = 0; x < np; ++x) o.room[x] = dp[x].n + dp[x].m;
        o.d_room = reinterpret_cast<const uint32_t*>(p + lay.room);
        IOC_CHK(c, hipMemcpyAsync(p + lay.room, o.room.data(), np * 4, hipMemcpyHostToDevice, c->stream));
    }
    if (h.has_pile()) {
        o.row_base.resize(np);
        o.q_off.resize(np);
        for (size_t x = 0; x < np; ++x) {
            o.row_base[x] = h.pile.piled[o.back[x]] ? -1 : h.pile.row_base[o.back[x]];
            o.q_off[x] = dp[x].q_off;
        }
        o.d_row_base = reinterpret_cast<const int64_t*>(p + lay.row_base);
        o.d_q_off = reinterpret_cast<const uint32_t*>(p + lay.q_off);
        IOC_CHK(c, hipMemcpyAsync(p + lay.row_base, o.row_base.data(), np * 8, hipMemcpyHostToDevice, c->stream));
        IOC_CHK(c, hipMemcpyAsync(p + lay.q_off, o.q_off.data(), np * 4, hipMemcpyHostToDevice, c->stream));
    }
    if (h.has_pile() && (h.pile.kind == PileKind::weighted || h.projects_weights())) {
        o.q_len.resize(np);
        for (size_t x = 0; x < np; ++x) o.q_len[x] = dp[x].n;
        o.d_q_len = reinterpret_cast<const uint32_t*>(p + lay.q_len);
        IOC_CHK(c, hipMemcpyAsync(p + lay.q_len, o.q_len.data(), np * 4, hipMemcpyHostToDevice, c->stream));
    }
    if (h.projects()) {
        o.plane.resize(np);
        for (size_t x = 0; x < np; ++x) o.plane[x] = uint64_t(h.pile.plane[o.back[x]]);
        o.d_plane = reinterpret_cast<const uint64_t*>(p + lay.plane);
        IOC_CHK(c, hipMemcpyAsync(p + lay.plane, o.plane.data(), np * 8, hipMemcpyHostToDevice, c->stream));
    }
    return IOC_OK;
}

// a slice's sink in a call that reduces on the device (ioc_align_pairs_stats, ioc_align_pairs_pileup): k_ops_stats and / or
// k_ops_pileup over the slice's pairs where their bytes lie; the lengths and the 64-byte records come back, the bytes do not (the
// pileup's table stays where it is until the call is over).  The same pairs are skipped as in ops_fetch.
int ops_fetch_reduced(ioc_ctx* c, OpsRun& o, const std::vector<AlnPairDev>& dp, const uint32_t* ord, const uint32_t* d_ord, uint32_t cnt)
{
    const AlnSink& h = *o.host;
    const AlnSink::Pile& pl = h.pile;
    const bool stats = h.has_stats(), pile = h.has_pile();
    AlnTally& t = *h.tally;
    int r;
    if (stats && (r = ioc_reserve(c, c->a_ostats, size_t(cnt) * sizeof(ioc_aln_stats))) != IOC_OK) return r;
    EventSet ev;
    ev.v.assign(6, nullptr);
    for (auto& e : ev.v) IOC_CHK(c, hipEventCreate(&e));
    IOC_CHK(c, hipEventRecord(ev.v[0], c->stream));
    if (stats) IOC_CHK(c, iock_ops_stats(c->stream, o.dev.buf, o.dev.end, o.dev.len, o.d_room, d_ord, cnt, c->a_ostats.as<ioc_aln_stats>()));
    IOC_CHK(c, hipEventRecord(ev.v[1], c->stream));
    const uint8_t* pool = static_cast<const uint8_t*>(c->a_pool.p);
    const uint64_t pool_bytes = uint64_t(c->aln_offs.back());
    switch (pile ? pl.kind : PileKind::none) {
    case PileKind::none: break;
    case PileKind::counts:
        IOC_CHK(c, iock_ops_pileup(c->stream, o.dev.buf, o.dev.end, o.dev.len, o.d_room, d_ord, cnt, o.d_row_base, o.d_q_off, pool, pool_bytes,
                                   pl.cols, uint64_t(pl.rows)));
        break;
    case PileKind::ins:
        IOC_CHK(c, iock_ops_pileup_ins(c->stream, o.dev.buf, o.dev.end, o.dev.len, o.d_room, d_ord, cnt, o.d_row_base, o.d_q_off, pool, pool_bytes,
                                       pl.cols, pl.ins, uint64_t(pl.rows)));
        break;
    case PileKind::weighted:
        IOC_CHK(c, iock_ops_pileup_weighted(c->stream, o.dev.buf, o.dev.end, o.dev.len, o.d_room, d_ord, cnt, o.d_row_base, o.d_q_off, o.d_q_len, pool,
                                            static_cast<const uint8_t*>(c->a_qual.p), pool_bytes, pl.cols, pl.wcols, pl.wins, uint64_t(pl.rows)));
        break;
    }
    IOC_CHK(c, hipEventRecord(ev.v[2], c->stream));
    if (h.projects())
        IOC_CHK(c, iock_ops_project(c->stream, o.dev.buf, o.dev.end, o.dev.len, o.d_room, d_ord, cnt, o.d_row_base, o.d_q_off, o.d_plane, pool, pool_bytes,
                                    pl.base_planes, pl.ins_planes, uint64_t(pl.plane_bytes)));
    IOC_CHK(c, hipEventRecord(ev.v[3], c->stream));
    if (h.projects_ins())
        IOC_CHK(c, iock_ops_project_ins(c->stream, o.dev.buf, o.dev.end, o.dev.len, o.d_room, d_ord, cnt, o.d_row_base, o.d_q_off, o.d_plane, pool,
                                        pool_bytes, pl.slot_planes, uint64_t(pl.plane_bytes)));
    IOC_CHK(c, hipEventRecord(ev.v[4], c->stream));
    if (h.projects_weights())
        IOC_CHK(c, iock_ops_project_weights(c->stream, o.dev.buf, o.dev.end, o.dev.len, o.d_room, d_ord, cnt, o.d_row_base, o.d_q_off, o.d_q_len, o.d_plane,
                                            static_cast<const uint8_t*>(c->a_qual.p), pool_bytes, pl.weight_planes, uint64_t(pl.plane_bytes)));
    IOC_CHK(c, hipEventRecord(ev.v[5], c->stream));
    if (h.projects_ilen()) {  // (its own event, and only where it runs: every other call records what it always did)
        ev.v.push_back(nullptr);
        IOC_CHK(c, hipEventCreate(&ev.v.back()));
        IOC_CHK(c, iock_ops_project_ilen(c->stream, o.dev.buf, o.dev.end, o.dev.len, o.d_room, d_ord, cnt, o.d_row_base, o.d_plane, pl.ilen_planes,
                                         uint64_t(pl.plane_bytes)));
        IOC_CHK(c, hipEventRecord(ev.v.back(), c->stream));
    }
    size_t ev_qpos = 0;
    if (h.projects_qpos()) {  // (likewise: its own event, behind whatever the calls that exist record)
        ev.v.push_back(nullptr);
        IOC_CHK(c, hipEventCreate(&ev.v.back()));
        ev_qpos = ev.v.size() - 1;
        IOC_CHK(c, iock_ops_project_qpos(c->stream, o.dev.buf, o.dev.end, o.dev.len, o.d_room, d_ord, cnt, o.d_row_base, o.d_plane, pl.qpos_planes,
                                         uint64_t(pl.plane_bytes)));
        IOC_CHK(c, hipEventRecord(ev.v.back(), c->stream));
    }
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    const auto t0 = std::chrono::steady_clock::now();
    o.len.resize(dp.size());
    IOC_CHK(c, hipMemcpy(o.len.data(), o.dev.len, dp.size() * 4, hipMemcpyDeviceToHost));
    if (stats) {
        o.recs.resize(cnt);
        IOC_CHK(c, hipMemcpy(o.recs.data(), c->a_ostats.p, size_t(cnt) * sizeof(ioc_aln_stats), hipMemcpyDeviceToHost));
    }
    for (uint32_t x = 0; x < cnt; ++x) {
        const uint32_t pid = ord[x], i = o.back[pid];
        const uint64_t L = o.len[pid];
        if (L == 0 || L > uint64_t(dp[pid].n) + dp[pid].m || L > o.end[pid]) continue;
        if (stats) h.stats[i] = o.recs[x];
        if (pile) pl.piled[i] = 1;
        h.len[i] = int64_t(L);
    }
    float ms = 0;
    if (stats && hipEventElapsedTime(&ms, ev.v[0], ev.v[1]) == hipSuccess) t.ms_stats += double(ms);
    if (pile && hipEventElapsedTime(&ms, ev.v[1], ev.v[2]) == hipSuccess) t.ms_pileup += double(ms);
    if (h.projects() && hipEventElapsedTime(&ms, ev.v[2], ev.v[3]) == hipSuccess) t.ms_project += double(ms);
    if (h.projects_ins() && hipEventElapsedTime(&ms, ev.v[3], ev.v[4]) == hipSuccess) t.ms_project_ins += double(ms);
    if (h.projects_weights() && hipEventElapsedTime(&ms, ev.v[4], ev.v[5]) == hipSuccess) t.ms_project_weights += double(ms);
    if (h.projects_ilen() && hipEventElapsedTime(&ms, ev.v[5], ev.v[6]) == hipSuccess) t.ms_project_ilen += double(ms);
    if (h.projects_qpos() && hipEventElapsedTime(&ms, ev.v[ev_qpos - 1], ev.v[ev_qpos]) == hipSuccess) t.ms_project_qpos += double(ms);
    t.ms_copy += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    t.copied += int64_t(dp.size() * 4 + (stats ? size_t(cnt) * sizeof(ioc_aln_stats) : 0));
    if (stats) t.records += int64_t(cnt);
    return IOC_OK;
}

// after a slice: its pairs' bytes to the caller's regions.  A pair that came back without an answer (len 0: refused by the 16-bit
// window or by the corridor's certificate; out of range: the walk of a forward pass that was given up) is left to its re-run.
int ops_fetch(ioc_ctx* c, OpsRun& o, const std::vector<AlnPairDev>& dp, const uint32_t* ord, const uint32_t* d_ord, uint32_t cnt, uint64_t bytes)
{
    if (o.host->reduced()) return ops_fetch_reduced(c, o, dp, ord, d_ord, cnt);
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    const auto t0 = std::chrono::steady_clock::now();
    o.len.resize(dp.size());
    if (o.stage.size() < bytes) o.stage.resize(size_t(bytes));
    IOC_CHK(c, hipMemcpy(o.len.data(), o.dev.len, dp.size() * 4, hipMemcpyDeviceToHost));
    IOC_CHK(c, hipMemcpy(o.stage.data(), o.dev.buf, size_t(bytes), hipMemcpyDeviceToHost));
    for (uint32_t x = 0; x < cnt; ++x) {
        const uint32_t pid = ord[x], i = o.back[pid];
        const uint64_t L = o.len[pid];
        if (L == 0 || L > uint64_t(dp[pid].n) + dp[pid].m || L > o.end[pid]) continue;
        memcpy(o.host->bytes.buf + o.host->bytes.base[i], o.stage.data() + (o.end[pid] - L), size_t(L));
        o.host->len[i] = int64_t(L);
    }
    o.host->tally->ms_copy += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    o.host->tally->copied += int64_t(bytes);
    return IOC_OK;
}

// ---- version 2 (ioc_align_v2.inc) ---------------------------------------------------------------------------------------

// the bound on |relative H| at a rebase of version 2's 16-bit window: what is live in a wave at one time differs by a few
// thousand at most, two cells of it being joined through a common ancestor by paths no longer than the window
constexpr int P16_GUARD = ALN_V2_GUARD;  // (ioc_align_sink.h: the routing predicate reasons from it)

// the switches that shape a plan (ioc_align_plan.h), read once per call of align_pairs: the tests change them between calls
AlnPlanOpts plan_opts()
{
    AlnPlanOpts o;
    if (const char* e = getenv("IOC_ALIGN_CORRIDOR")) {
        o.corridor_frac = std::max(0.0, std::min(1.0, atof(e)));
        o.corridor_fixed = true;
    }
    if (const char* e = getenv("IOC_ALIGN_CORRIDOR_TAPER")) o.taper = atoi(e) != 0;
    if (const char* e = getenv("IOC_ALIGN_CORRIDOR_MARGIN")) o.taper_margin = uint32_t(std::max(0, std::min(1 << 20, atoi(e))));
    o.no_fit = getenv("IOC_ALIGN_CORRIDOR_NO_FIT") != nullptr;
    if (const char* e = getenv("IOC_ALIGN_V2_FEW")) o.few_limit = uint32_t(std::max(0, atoi(e)));
    if (const char* e = getenv("IOC_ALIGN_WAVES")) {
        o.waves = atoi(e);
        o.waves_set = true;
    }
    o.no_cross_tail = getenv("IOC_ALIGN_NO_CROSS_TAIL") != nullptr;
    return o;
}

// ... and a slice's list as the device made it against the host's, item by item (behind a wait for the stream)
int device_items_check(ioc_ctx* c, const V2Plan& pl, const V2Item* d_items, size_t si)
{
    const std::vector<V2Item>& want = pl.items[si];
    std::vector<V2Item> got(want.size());
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    if (!got.empty()) IOC_CHK(c, hipMemcpy(got.data(), d_items, got.size() * sizeof(V2Item), hipMemcpyDeviceToHost));
    for (size_t x = 0; x < want.size(); ++x)
        if (got[x].couple != want[x].couple || got[x].band != want[x].band || got[x].strip != want[x].strip)
            return ioc_fail(c, IOC_ERR_STATE, "IOC_V2_ITEMS_CHECK: slice " + std::to_string(si) + ": the device's list differs from the host's at index " +
                                                  std::to_string(x) + " of " + std::to_string(want.size()) + " (" + std::to_string(pl.n_probe[si]) +
                                                  " of the probe): couple " + std::to_string(got[x].couple) + " band " + std::to_string(got[x].band) + " strip " +
                                                  std::to_string(got[x].strip) + ", the host has couple " + std::to_string(want[x].couple) + " band " +
                                                  std::to_string(want[x].band) + " strip " + std::to_string(want[x].strip));
    if (getenv("IOC_TRACE")) {
        fprintf(stderr, "[ioc]   aligner v2: IOC_V2_ITEMS_CHECK: slice %zu: %zu tiles (%u of the probe) equal the host's list\n", si, want.size(), pl.n_probe[si]);
        // (the grids the list was made from, bands x strips per couple; c: a corridor with its probe's grid, 1: a couple of one pair)
        fprintf(stderr, "[ioc]   aligner v2: IOC_V2_ITEMS_CHECK: slice %zu grids:", si);
        for (uint32_t k2 = pl.slices[si].first; k2 < pl.slices[si].first + pl.slices[si].second; ++k2) {
            const V2Couple& cp = pl.cps[k2];
            fprintf(stderr, " %ux%u", cp.nbands, cp.nstrips);
            if (cp.corridor) fprintf(stderr, "c%ux%u", uint32_t(cp.probe_band) + 1u, uint32_t(cp.probe_strip) + 1u);
            if (cp.pid[1] == 0xFFFFFFFFu) fprintf(stderr, "/1");
        }
        fprintf(stderr, "\n");
    }
    return IOC_OK;
}

// ... and, after the slice has run, how many of the couples the host planned a corridor for the probe's verdicts opened (every
// tile) — they come after the list and are no part of it
int device_probe_report(ioc_ctx* c, const V2Plan& pl, const V2Couple* d_cps, size_t si)
{
    if (!getenv("IOC_TRACE")) return IOC_OK;
    const uint32_t k_first = pl.slices[si].first, n_couples = pl.slices[si].second;
    std::vector<V2Couple> got(n_couples);
    IOC_CHK(c, hipMemcpy(got.data(), d_cps + k_first, size_t(n_couples) * sizeof(V2Couple), hipMemcpyDeviceToHost));
    uint32_t planned = 0, opened = 0;
    std::string which;
    for (uint32_t x = 0; x < n_couples; ++x) {
        planned += pl.cps[k_first + x].corridor ? 1u : 0u;
        if (pl.cps[k_first + x].corridor && !got[x].corridor) {
            ++opened;
            which += " " + std::to_string(k_first + x);
        }
    }
    fprintf(stderr, "[ioc]   aligner v2: IOC_V2_ITEMS_CHECK: slice %zu: %u couples with a corridor planned, %u opened by the probe (couples:%s)\n", si, planned,
            opened, which.c_str());
    return IOC_OK;
}

// the launch settings of align_v2_run (environment switches and the chip)
struct V2Opts {
    int n_cu, occ, guard;
    uint32_t few_limit;                  // couples in a launch up to which its tiles wait for rows instead of tiles (IOC_ALIGN_V2_FEW; 0: never)
    uint32_t deadline;                   // traceback blocks before a walk is parked for the second launch (IOC_TRACE2_DEADLINE; 0: one launch)
    unsigned long long deadline_cycles;  // ... or cycles of the first launch (IOC_TRACE2_CYCLES; 0: the block count alone)
    uint32_t help_wgs;                   // workgroups of the helper launches
    bool side_help;                      // the wrong candidates' walks on the side stream, beside the first launch (IOC_TRACE2_EARLY)
};

// where the plan lives on the device, in the context's buffers
struct V2Dev {
    V2Couple* cps;
    V2PairCk* pck;
    V2PairEnd* pend;
    V2Item* items;
    int2 *lrow, *best;
    // [queue][err][pad][pad][tiles computed][links without a left side][links with the left tile done][pad ...][flags][rows of a tile's
    // right edge that are out (v2_wait_rows)][ovf per pair][claims, indexed like the flags (v2_fwd_body: links)][computed cells, 8-byte aligned]
    uint32_t* ctl;
    size_t ctl_words;
    V2Scratch *scratch, *hscratch;
    uint32_t* resume;  // per pair: V2_RESUME_WORDS of parked state and records
    uint32_t* park;    // [count][pair slots of the slice]: parked by the first traceback launch
    uint32_t* early;   // ... and sent to the helper launch by k_fwd2_ends (wrong candidates, by their score)
    uint32_t* gate;    // workgroups of that launch that have started
    uint32_t* split;   // per pair: V2_SPLIT_WORDS, where the walk's time went in either launch
    size_t resume_words;
};

// the plan's tables on the device and every buffer of the launches (after the checkpoint arena)
int v2_tables(ioc_ctx* c, const V2Plan& pl, uint32_t help_wgs, V2Dev& t)
{
    hipStream_t s = c->stream;
    const uint32_t ncouples = pl.ncouples, np = pl.np;
    const size_t tab_bytes = size_t(ncouples) * sizeof(V2Couple) + size_t(np) * (sizeof(V2PairCk) + sizeof(V2PairEnd)) + size_t(pl.max_items) * sizeof(V2Item) + 256;
    IOC_TRY(ioc_reserve(c, c->a_cko, tab_bytes));
    uint8_t* tb = static_cast<uint8_t*>(c->a_cko.p);
    t.cps = reinterpret_cast<V2Couple*>(tb);
    t.pck = reinterpret_cast<V2PairCk*>(tb + size_t(ncouples) * sizeof(V2Couple));
    t.pend = reinterpret_cast<V2PairEnd*>(reinterpret_cast<uint8_t*>(t.pck) + size_t(np) * sizeof(V2PairCk));
    t.items = reinterpret_cast<V2Item*>(reinterpret_cast<uint8_t*>(t.pend) + size_t(np) * sizeof(V2PairEnd));
    IOC_CHK(c, hipMemcpyAsync(t.cps, pl.cps.data(), size_t(ncouples) * sizeof(V2Couple), hipMemcpyHostToDevice, s));
    IOC_CHK(c, hipMemcpyAsync(t.pck, pl.pck.data(), size_t(np) * sizeof(V2PairCk), hipMemcpyHostToDevice, s));
    IOC_CHK(c, hipMemcpyAsync(t.pend, pl.pend.data(), size_t(np) * sizeof(V2PairEnd), hipMemcpyHostToDevice, s));
    // the query profiles of every (couple, strip) of a slice (made slice by slice, in front of the slice's forward pass)
    IOC_TRY(ioc_reserve(c, c->a_prof, size_t(pl.prof_total) * sizeof(uint4) + 256));
    IOC_TRY(ioc_reserve(c, c->a_ends2, size_t(np) * sizeof(int4)));
    IOC_TRY(ioc_reserve(c, c->a_lrow, (size_t(pl.lrow_total) + pl.best_total + 16) * sizeof(int2)));
    t.lrow = static_cast<int2*>(c->a_lrow.p);
    t.best = t.lrow + pl.lrow_total;
    t.ctl_words = ((16 + 3 * size_t(pl.max_flags) + np + 1) & ~size_t(1)) + 2;
    IOC_TRY(ioc_reserve(c, c->a_xflags, t.ctl_words * 4));
    t.ctl = static_cast<uint32_t*>(c->a_xflags.p);
    // per pair: its own scratch and 16 words of parked state and records; (the helper buffers belong to the second launch's
    // WORKGROUPS — one per compute unit — not to the pairs: 0.66 MB each)
    const size_t n_scratch = size_t(pl.max_pairs) + size_t(help_wgs) * V2_NHELP * V2_HBUF;
    // (parked state, the two lists of walks for the helper launches, the walks' time records)
    t.resume_words = size_t(np) * V2_RESUME_WORDS + 2u * (size_t(pl.max_pairs) + 1u) + 4u + size_t(np) * V2_SPLIT_WORDS;
    IOC_TRY(ioc_reserve(c, c->a_bnd, n_scratch * sizeof(V2Scratch) + t.resume_words * 4));
    t.scratch = static_cast<V2Scratch*>(c->a_bnd.p);
    t.hscratch = t.scratch + pl.max_pairs;
    t.resume = reinterpret_cast<uint32_t*>(t.scratch + n_scratch);
    t.park = t.resume + size_t(np) * V2_RESUME_WORDS;
    t.early = t.park + size_t(pl.max_pairs) + 1u;
    t.gate = t.early + size_t(pl.max_pairs) + 1u;
    t.split = t.gate + 4u;
    return IOC_OK;
}

// Workgroups per compute unit of a slice's main launch.  A tile waits for the tile above and the tile to its left, so a couple's
// grid offers only its current anti-diagonal — with the corridor 2 - 3 tiles of a 16.7 kb pair — and a tile takes 0.5 - 0.9 ms:
// the pass is bound by tiles in flight as much as by throughput (config 3: 37 ms for a critical path of ~18).  Waves beyond the
// tiles that can run sit on a tile whose neighbours are still being computed, and they sit unevenly: a SIMD with three busy
// waves next to one with a single busy wave and two waiting.  So: as many workgroups per CU as the list's tiles per
// anti-diagonal keep busy, the same number on every CU (config 3 with the corridor: 2 per CU 37.2 ms, 3 per CU 39.8,
// 2.25 per CU 40.6; every tile: 3 per CU 67.6, 2 per CU 72.7; a quarter of the batch: 1 per CU 22.7, 3 per CU 25.1).
uint32_t v2_per_cu(const V2Plan& pl, size_t si, const V2Opts& o, bool few_couples)
{
    if (few_couples) return uint32_t(o.occ);
    uint64_t tiles = 0;
    uint32_t diags = 1;
    for (uint32_t k2 = pl.slices[si].first; k2 < pl.slices[si].first + pl.slices[si].second; ++k2) {
        const V2Couple& cp = pl.cps[k2];
        for (uint32_t b = 0; b < cp.nbands; ++b) tiles += uint32_t(cp.phi[b]) - uint32_t(cp.plo[b]) + 1u;
        diags = std::max(diags, cp.nbands + cp.nstrips - 1u);
    }
    const double x = double(tiles) / double(diags) / double(uint32_t(o.n_cu) * uint32_t(V2_WAVES));
    return x < 1.0 ? 1u : x < 2.75 ? std::min(2u, uint32_t(o.occ)) : uint32_t(o.occ);
}

// One slice's launches: profiles, probe, forward pass, ends, traceback (events ev[0 .. 3) around them), then its error word
// (*xe: a bounded wait ran out), computed cells and links (link_sum[0 .. 3) += tiles computed, links of either kind).
// `od`: an emitting call — the traceback launches are the emitting kernels, the same launches otherwise.
int v2_slice(ioc_ctx* c, const V2Plan& pl, const V2Dev& t, size_t si, const V2Opts& o, const AlnParams& P, const uint32_t* d_order,
             int32_t* d_score, uint32_t* d_count, const hipEvent_t* ev, uint32_t* xe, uint32_t* link_sum, const AlnOpsDev* od, StageTrace& tr)
{
    hipStream_t s = c->stream;
    const uint32_t k_first = pl.slices[si].first, n_couples = pl.slices[si].second;
    const uint32_t first_pair = 2u * k_first, n_pairs = std::min(pl.cnt, 2u * (k_first + n_couples)) - first_pair;
    const uint32_t n_items = pl.n_items[si], n_probe = pl.n_probe[si];
    const AlnPairDev* d_pairs = static_cast<const AlnPairDev*>(c->a_pairs.p);
    const uint8_t* d_pool = static_cast<const uint8_t*>(c->a_pool.p);
    uint32_t* d_ctl = t.ctl;
    // (few couples: bound by ONE grid's critical path — tiles follow their left neighbours row by row, v2_wait_rows; a tile
    // publishes its progress every block of 64 rows)
    const bool few_couples = n_couples <= o.few_limit;
    const uint32_t prog_every = few_couples ? 1u : 0u;
    // (IOC_ALIGN_V2_LINK=0: no claims, no run goes on into the band below — v2_fwd_body)
    const bool links = !(getenv("IOC_ALIGN_V2_LINK") && atoi(getenv("IOC_ALIGN_V2_LINK")) == 0);
    uint32_t* const d_claims = links ? d_ctl + 16 + 2 * pl.max_flags + pl.np : static_cast<uint32_t*>(nullptr);
    // the slice's list of tiles, from the couples as the host planned them (v2_tables sent them up; the probe's verdicts, which
    // rewrite a couple's corridor, come after the list and never enter it)
    const bool items_check = !pl.items.empty();  // (IOC_V2_ITEMS_CHECK)
    if (items_check)  // (no item an earlier call or slice left there can stand in for one the kernel did not write)
        IOC_CHK(c, hipMemsetAsync(t.items, 0xFF, size_t(n_items) * sizeof(V2Item), s));
    hipLaunchKernelGGL(k_fwd2_items, dim3(pl.n_diag[si], 2), dim3(V2_ITEMS_T), 0, s, t.cps, k_first, n_couples, n_probe, t.items, n_items);
    IOC_CHK(c, hipGetLastError());
    if (items_check) IOC_TRY(device_items_check(c, pl, t.items, si));
    hipLaunchKernelGGL(k_fwd2_prof, dim3(n_couples, pl.max_strips), dim3(128), 0, s, d_pairs, t.cps + k_first, d_pool, P, static_cast<uint4*>(c->a_prof.p));
    IOC_CHK(c, hipGetLastError());
    IOC_CHK(c, hipMemsetAsync(d_ctl, 0, t.ctl_words * 4, s));
    IOC_CHK(c, hipMemsetAsync(t.resume, 0, t.resume_words * 4, s));  // (parked state and the two lists of walks; k_fwd2_ends writes into them)
    if (pl.tiles_skipped)  // (the bests of the last row and the last column that a skipped tile does not write: far below any score)
        IOC_CHK(c, hipMemsetAsync(t.lrow, 0x80, (size_t(pl.lrow_total) + pl.best_total) * sizeof(int2), s));
    if (getenv("IOC_ALIGN_V2_FAKE_TIMEOUT")) {  // (tests: as if a bounded wait had run out — every later wait gives up at once,
        const uint32_t one = 1;                 // tiles run on whatever is there, the host must fall back to version 1)
        IOC_CHK(c, hipMemcpyAsync(d_ctl + 1, &one, 4, hipMemcpyHostToDevice, s));
    }
    IOC_CHK(c, hipEventRecord(ev[0], s));
    // persistent waves: as many workgroups as the chip holds, but no more waves than tiles
    auto fwd = [&](decltype(&k_fwd2) kernel, uint32_t n_wg, const V2Item* items, uint32_t n, uint32_t link_mode) {
        hipLaunchKernelGGL(kernel, dim3(n_wg), dim3(64 * V2_WAVES), 0, s, d_pairs, t.cps, items, n, d_ctl, d_ctl + 16, d_ctl + 1, d_pool, P,
                           static_cast<uint32_t*>(c->a_ck.p), t.lrow, t.best, d_ctl + 16 + 2 * pl.max_flags, o.guard, static_cast<const uint4*>(c->a_prof.p),
                           reinterpret_cast<unsigned long long*>(d_ctl + t.ctl_words - 2), few_couples ? d_ctl + 16 + pl.max_flags : static_cast<uint32_t*>(nullptr),
                           prog_every, d_claims, link_mode);
    };
    if (n_probe) {  // the probe launch and its verdicts (V2Couple): all on the device, nothing comes back to the host
        fwd(k_fwd2, std::max(1u, std::min(uint32_t(o.occ) * uint32_t(o.n_cu), (n_probe + V2_WAVES - 1) / V2_WAVES)), t.items, n_probe, 2u);
        IOC_CHK(c, hipGetLastError());
        hipLaunchKernelGGL(k_fwd2_probe, dim3(n_couples), dim3(64), 0, s, d_pairs, t.cps + k_first, t.pend, static_cast<const uint32_t*>(c->a_ck.p), P);
        IOC_CHK(c, hipGetLastError());
        IOC_CHK(c, hipMemsetAsync(d_ctl, 0, 4, s));  // (the queue's counter; the flags of the probe's tiles stay)
    }
    tr.mark("v2_slice up to the probe");
    const uint32_t n_main = n_items - n_probe, per_cu = v2_per_cu(pl, si, o, few_couples);
    const uint32_t n_wg = std::max(1u, std::min(per_cu * uint32_t(o.n_cu), (n_main + V2_WAVES - 1) / V2_WAVES));
    // (two workgroups per CU: the build of the kernel that may use the registers of the third)
    const bool w2 = per_cu <= 2 && !getenv("IOC_ALIGN_V2_NO_W2");
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner v2: shape: slice %zu: %u couples, waits for %s, per_cu %u, n_wg %u, kernel %s, n_probe %u\n", si, n_couples,
                few_couples ? "rows" : "tiles", per_cu, n_wg, w2 ? "k_fwd2_w2" : "k_fwd2", n_probe);
    fwd(w2 ? k_fwd2_w2 : k_fwd2, n_wg, t.items + n_probe, n_main, 1u);
    IOC_CHK(c, hipGetLastError());
    bool tapered = false;  // (some pair of the slice is vouched for by its exit cells: V2PairEnd)
    for (uint32_t k2 = k_first; k2 < k_first + n_couples && !tapered; ++k2)
        for (int h = 0; h < 2; ++h)
            if (pl.cps[k2].pid[h] != 0xFFFFFFFFu && pl.pend[pl.cps[k2].pid[h]].start != INT32_MAX) tapered = true;
    if (tapered) {
        hipLaunchKernelGGL(k_fwd2_cert, dim3(n_pairs, V2_CERT_Y), dim3(V2_CERT_T), 0, s, d_pairs, t.cps, d_order + first_pair, n_pairs, t.pend,
                           static_cast<const uint32_t*>(c->a_ck.p), P);
        IOC_CHK(c, hipGetLastError());
    }
    const uint32_t n_help = std::min<uint32_t>(n_pairs, o.help_wgs);
    hipLaunchKernelGGL(k_fwd2_ends, dim3(n_pairs), dim3(64), 0, s, d_pairs, t.cps, d_order + first_pair, n_pairs, t.pend, t.lrow, t.best,
                       d_ctl + 16 + 2 * pl.max_flags, static_cast<int4*>(c->a_ends2.p), t.resume, t.early, o.side_help ? int(P.match) : 0, n_help);
    IOC_CHK(c, hipGetLastError());
    IOC_CHK(c, hipEventRecord(ev[1], s));
    // the traceback in two launches: walks that need more than `deadline` blocks go on in the second one, with helper waves
    auto help = [&](hipStream_t hs, uint32_t* list, uint32_t which, uint32_t* gate) {
        if (od)
            hipLaunchKernelGGL(k_trace2_help_ops, dim3(n_help), dim3(64 * V2_HWAVES), 0, hs, d_pairs, d_order + first_pair, d_pool, P,
                               static_cast<const uint32_t*>(c->a_ck.p), t.cps, t.pck, static_cast<const int4*>(c->a_ends2.p), t.scratch, t.hscratch,
                               t.resume, list, t.split, d_score, d_count, n_pairs, which, gate, *od);
        else
            hipLaunchKernelGGL(k_trace2_help, dim3(n_help), dim3(64 * V2_HWAVES), 0, hs, d_pairs, d_order + first_pair, d_pool, P,
                               static_cast<const uint32_t*>(c->a_ck.p), t.cps, t.pck, static_cast<const int4*>(c->a_ends2.p), t.scratch, t.hscratch,
                               t.resume, list, t.split, d_score, d_count, n_pairs, which, gate);
    };
    if (o.side_help) {  // (issued before the first launch: its workgroups — a walker and ten helpers each — take their places first)
        IOC_CHK(c, hipEventRecord(c->ev_side[0], s));
        IOC_CHK(c, hipStreamWaitEvent(c->side_stream, c->ev_side[0], 0));
        help(c->side_stream, t.early, 2u, t.gate);
        IOC_CHK(c, hipGetLastError());
        IOC_CHK(c, hipEventRecord(c->ev_side[1], c->side_stream));
        hipLaunchKernelGGL(k_trace2_gate, dim3(1), dim3(1), 0, s, t.early, t.gate, n_help);
        IOC_CHK(c, hipGetLastError());
    }
    if (od)
        hipLaunchKernelGGL(k_trace2_ops, dim3((n_pairs + TR_WAVES - 1) / TR_WAVES), dim3(64 * TR_WAVES), 0, s, d_pairs, d_order + first_pair, d_pool, P,
                           static_cast<const uint32_t*>(c->a_ck.p), t.cps, t.pck, static_cast<const int4*>(c->a_ends2.p), t.scratch, t.resume, t.park,
                           t.split, d_score, d_count, n_pairs, o.deadline, o.deadline_cycles, *od);
    else
        hipLaunchKernelGGL(k_trace2, dim3((n_pairs + TR_WAVES - 1) / TR_WAVES), dim3(64 * TR_WAVES), 0, s, d_pairs, d_order + first_pair, d_pool, P,
                           static_cast<const uint32_t*>(c->a_ck.p), t.cps, t.pck, static_cast<const int4*>(c->a_ends2.p), t.scratch, t.resume, t.park,
                           t.split, d_score, d_count, n_pairs, o.deadline, o.deadline_cycles);
    IOC_CHK(c, hipGetLastError());
    if (o.side_help) IOC_CHK(c, hipStreamWaitEvent(s, c->ev_side[1], 0));  // (the two helper launches share the helpers' buffers)
    if (o.deadline) {  // (one workgroup per compute unit: a walker and its helpers fill one; more parked walks than that take turns)
        help(s, t.park, 1u, nullptr);
        IOC_CHK(c, hipGetLastError());
    }
    IOC_CHK(c, hipEventRecord(ev[2], s));
    unsigned long long cells_done = 0;
    IOC_CHK(c, hipMemcpyAsync(xe, d_ctl + 1, 4, hipMemcpyDeviceToHost, s));
    IOC_CHK(c, hipMemcpyAsync(&cells_done, d_ctl + t.ctl_words - 2, 8, hipMemcpyDeviceToHost, s));
    uint32_t link_counts[3] = {0, 0, 0};
    if (getenv("IOC_TRACE")) IOC_CHK(c, hipMemcpyAsync(link_counts, d_ctl + 4, sizeof link_counts, hipMemcpyDeviceToHost, s));
    tr.mark("v2_slice other launches");
    IOC_CHK(c, hipStreamSynchronize(s));
    tr.mark("v2_slice wait (device)");
    c->tm.n_align_cells_computed += int64_t(cells_done);
    for (int x = 0; x < 3; ++x) link_sum[x] += link_counts[x];
    if (items_check) IOC_TRY(device_probe_report(c, pl, t.cps, si));
    return IOC_OK;
}

// developer aids after a slice (tools/corridor_rates.py): IOC_V2_TRACE_RATES prints the score per base against the
// summed error rate, pair by pair (the corridor's calibration); IOC_V2_TRACE_TIMES the slowest walks of the slice (k_trace2
// ends when its slowest wave does)
int v2_report(ioc_ctx* c, const std::vector<AlnPairDev>& dp, const uint32_t* order, const V2Plan& pl, const V2Dev& t, size_t si, uint32_t deadline)
{
    const bool rates = getenv("IOC_V2_TRACE_RATES") != nullptr, times = getenv("IOC_V2_TRACE_TIMES") != nullptr;
    if (!rates && !times) return IOC_OK;
    const uint32_t np = pl.np, first_pair = 2u * pl.slices[si].first;
    const uint32_t n_pairs = std::min(pl.cnt, 2u * (pl.slices[si].first + pl.slices[si].second)) - first_pair;
    std::vector<int4> he(np);
    IOC_CHK(c, hipMemcpy(he.data(), c->a_ends2.p, size_t(np) * sizeof(int4), hipMemcpyDeviceToHost));
    if (rates)
        for (uint32_t x = 0; x < n_pairs; ++x) {
            const uint32_t pid = order[first_pair + x];
            const AlnPairDev& d = dp[pid];
            fprintf(stderr, "[rate] e %.5f n %u m %u score %d per_base %.5f go %d flags %d corridor %u\n", double(d.e_sum), d.n, d.m, he[pid].x,
                    double(he[pid].x) / double(std::max(d.n, d.m)), d.gap_open, he[pid].w, pl.cps[pl.pend[pid].couple].corridor);
        }
    if (!times) return IOC_OK;
    std::vector<uint32_t> rw(size_t(np) * V2_RESUME_WORDS);
    IOC_CHK(c, hipMemcpy(rw.data(), t.resume, rw.size() * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> ids(n_pairs);
    for (uint32_t x = 0; x < n_pairs; ++x) ids[x] = order[first_pair + x];
    // (first launch + second launch: the second starts when the first has ended, so the sum orders the pairs by what they cost)
    auto rec = [&](uint32_t pid, uint32_t w) { return rw[size_t(pid) * V2_RESUME_WORDS + w]; };
    auto cost = [&](uint32_t pid) { return (double(rec(pid, 8)) + double(rec(pid, 12))) * 256.0; };
    std::sort(ids.begin(), ids.end(), [&](uint32_t a, uint32_t b) { return cost(a) > cost(b); });
    double sum = 0;
    uint32_t parked = 0;
    for (uint32_t pid : ids) {
        sum += cost(pid);
        parked += rec(pid, 6) ? 1u : 0u;
    }
    fprintf(stderr, "[ioc] k_trace2: %u pairs, %u walks went on in the second launch (deadline %u blocks); mean %.3e cycles (s_memtime), slowest first:\n", n_pairs, parked,
            deadline, sum / n_pairs);
    auto line = [&](const char* tag, uint32_t pid) {
        const AlnPairDev& d = dp[pid];
        fprintf(stderr, "[ioc]   %s pair %u: %.3e + %.3e cycles, n %u m %u, blocks %u (%u on the diagonal) + %u (%u by helpers), tiles %u + %u, gap steps %u, windows %u\n", tag, pid,
                double(rec(pid, 8)) * 256.0, double(rec(pid, 12)) * 256.0, d.n, d.m, rec(pid, 9) & 0xFFFFu, rec(pid, 9) >> 16, rec(pid, 13) & 0xFFFFu, rec(pid, 13) >> 16,
                rec(pid, 10), rec(pid, 14), rec(pid, 11), rec(pid, 15));
    };
    {   // how well does the forward score tell the walks that get parked (wrong candidates) from the others?  score / shorter length
        double pk_max = -1e9, un_min = 1e9, pk_sum = 0, un_sum = 0;
        uint32_t npk = 0, nun = 0;
        std::vector<double> pks, uns;
        for (uint32_t pid : ids) {
            const AlnPairDev& d = dp[pid];
            const double q = double(he[pid].x) / double(std::max(1u, std::min(d.n, d.m)));
            if (rec(pid, 6)) {
                pk_max = std::max(pk_max, q), pk_sum += q, ++npk;
                pks.push_back(q);
            } else {
                un_min = std::min(un_min, q), un_sum += q, ++nun;
                uns.push_back(q);
            }
        }
        std::sort(pks.begin(), pks.end());
        std::sort(uns.begin(), uns.end());
        auto qt = [](const std::vector<double>& v, double f) { return v.empty() ? 0.0 : v[std::min(v.size() - 1, size_t(f * double(v.size())))]; };
        fprintf(stderr, "[ioc]   forward score / shorter length: parked walks (%u) mean %.3f, 50 %% %.3f, 90 %% %.3f, 99 %% %.3f, max %.3f | others (%u) min %.3f, 1 %% %.3f, 10 %% %.3f, mean %.3f\n", npk,
                npk ? pk_sum / npk : 0.0, qt(pks, 0.5), qt(pks, 0.9), qt(pks, 0.99), pk_max, nun, un_min, qt(uns, 0.01), qt(uns, 0.1), nun ? un_sum / nun : 0.0);
    }
    for (uint32_t x = 0; x < std::min(n_pairs, 10u); ++x) line("", ids[x]);
    for (uint32_t qx : {n_pairs / 4u, n_pairs / 2u, 3u * n_pairs / 4u}) line("rank", ids[qx]);
    // where a walk's time goes, per launch: its blocks (waiting for a helper's, or recomputing), the recomputation of its tiles, its walk loop
    std::vector<uint32_t> sw(size_t(np) * V2_SPLIT_WORDS);
    IOC_CHK(c, hipMemcpy(sw.data(), t.split, sw.size() * 4, hipMemcpyDeviceToHost));
    for (uint32_t l = 0; l < 2u; ++l) {
        auto cyc = [&](uint32_t pid) { return double(rec(pid, l ? 12 : 8)) * 256.0; };
        auto spl = [&](uint32_t pid, uint32_t w) { return sw[size_t(pid) * V2_SPLIT_WORDS + l * (V2_SPLIT_WORDS / 2u) + w]; };
        std::vector<uint32_t> in;
        for (uint32_t pid : ids)
            if (rec(pid, l ? 12 : 8)) in.push_back(pid);
        std::sort(in.begin(), in.end(), [&](uint32_t a, uint32_t b) { return cyc(a) > cyc(b); });
        double tot[11] = {};
        for (uint32_t pid : in) {
            tot[0] += cyc(pid);
            for (uint32_t w = 0; w < 3u; ++w) tot[1 + w] += double(spl(pid, w)) * 256.0;
            tot[4] += double(spl(pid, 3) & 0xFFFFu);
            tot[5] += double(spl(pid, 4));
            tot[6] += double(spl(pid, 5));
            tot[7] += double(spl(pid, 6));
            for (uint32_t w = 0; w < 3u; ++w) tot[8 + w] += double(spl(pid, 7 + w)) * 256.0;  // (own blocks: all, <= 64 columns, <= 64 rows)
        }
        const double nn = double(std::max<size_t>(1, in.size()));
        fprintf(stderr, "[ioc] split of %s: %zu walks; mean %.3e cycles: blocks %.1f %%, tile recomputation %.1f %%, walk loop %.1f %%; %.1f cycles per tile step; "
                        "blocks of <= 64 columns: %.2f per walk, %.1f %% of the block steps recomputed by walkers\n",
                l ? "k_trace2_help" : "k_trace2", in.size(), tot[0] / nn, 100.0 * tot[1] / std::max(1.0, tot[0]), 100.0 * tot[2] / std::max(1.0, tot[0]),
                100.0 * tot[3] / std::max(1.0, tot[0]), tot[2] / std::max(1.0, tot[7]), tot[4] / nn, 100.0 * tot[6] / std::max(1.0, tot[5]));
        fprintf(stderr, "[ioc]   own blocks: %.1f %% of the blocks' cycles (the rest: waiting for a helper's); %.1f cycles per own block step in blocks of > 64 columns, %.1f in those of <= 64; "
                        "blocks of <= 64 rows: %.1f %% of the own blocks' cycles\n",
                100.0 * tot[8] / std::max(1.0, tot[1]), (tot[8] - tot[9]) / std::max(1.0, tot[5] - tot[6]), tot[9] / std::max(1.0, tot[6]), 100.0 * tot[10] / std::max(1.0, tot[8]));
        for (size_t x = 0; x < std::min<size_t>(in.size(), 10); ++x) {
            const uint32_t pid = in[x];
            const uint32_t nb = l ? rec(pid, 13) & 0xFFFFu : rec(pid, 9) & 0xFFFFu;
            fprintf(stderr, "[ioc]   split pair %u: %.3e cycles: blocks %.3e, tiles %.3e, walk %.3e; blocks %u (<= 64 columns %u, <= 64 rows %u), own block steps %u (%u in thin), own block cycles %.3e (%.3e in <= 64 columns, %.3e in <= 64 rows), tiles %u, tile steps %u\n",
                    pid, cyc(pid), double(spl(pid, 0)) * 256.0, double(spl(pid, 1)) * 256.0, double(spl(pid, 2)) * 256.0, nb, spl(pid, 3) & 0xFFFFu, spl(pid, 3) >> 16,
                    spl(pid, 4), spl(pid, 5), double(spl(pid, 7)) * 256.0, double(spl(pid, 8)) * 256.0, double(spl(pid, 9)) * 256.0, rec(pid, l ? 14 : 10), spl(pid, 6));
        }
    }
    return IOC_OK;
}

// IOC_V2_CERT_CHECK (developer switch): after a slice, every pair of up to 12 kb that kept its corridor once more on the host
// (ioc_host_align_corridor, with the corridor as the probe left it): the restricted score and end cell and the bounds of the
// certificate must be the device's; the call fails at the first pair that differs.  The parent bound is planned per couple — with the
// larger pair's rows and columns — so a shorter pair's may exceed the host's.
int v2_cert_check(ioc_ctx* c, const std::vector<AlnPairDev>& dp, const uint32_t* order, const V2Plan& pl, const V2Dev& t, size_t si, const AlnParams& P)
{
    const uint32_t k_first = pl.slices[si].first, n_couples = pl.slices[si].second, first_pair = 2u * k_first;
    const uint32_t n_pairs = std::min(pl.cnt, 2u * (k_first + n_couples)) - first_pair;
    std::vector<V2Couple> cps(n_couples);
    std::vector<V2PairEnd> pe(pl.np);
    std::vector<int4> he(pl.np);
    IOC_CHK(c, hipMemcpy(cps.data(), t.cps + k_first, size_t(n_couples) * sizeof(V2Couple), hipMemcpyDeviceToHost));
    IOC_CHK(c, hipMemcpy(pe.data(), t.pend, size_t(pl.np) * sizeof(V2PairEnd), hipMemcpyDeviceToHost));
    IOC_CHK(c, hipMemcpy(he.data(), c->a_ends2.p, size_t(pl.np) * sizeof(int4), hipMemcpyDeviceToHost));
    uint32_t checked = 0, tapered = 0, refuted = 0;
    std::vector<char> q, r;
    for (uint32_t x = 0; x < n_pairs; ++x) {
        const uint32_t pid = order[first_pair + x];
        const AlnPairDev& d = dp[pid];
        const V2PairEnd& e = pe[pid];
        const V2Couple& cp = cps[e.couple - k_first];
        if (!cp.corridor || e.cert == INT32_MIN || std::max(d.n, d.m) > 12288u || d.n == 0 || d.m == 0 || (he[pid].w & 1)) continue;
        q.resize(d.n);
        r.resize(d.m);
        IOC_CHK(c, hipMemcpy(q.data(), static_cast<const uint8_t*>(c->a_pool.p) + d.q_off, d.n, hipMemcpyDeviceToHost));
        IOC_CHK(c, hipMemcpy(r.data(), static_cast<const uint8_t*>(c->a_pool.p) + d.r_off, d.m, hipMemcpyDeviceToHost));
        auto acgt = [](char ch) { return ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T'; };
        if (d.rc) {
            std::reverse(r.begin(), r.end());
            for (char& ch : r) ch = ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : ch;
        }
        for (char& ch : q)  // (the kernels' rule: a letter other than A, C, G, T equals nothing)
            if (!acgt(ch)) ch = 1;
        for (char& ch : r)
            if (!acgt(ch)) ch = 2;
        int32_t rows[V2_MAX_BANDS], lo[V2_MAX_BANDS], hi[V2_MAX_BANDS], out[8];
        uint32_t nmax = 0, mmax = 0;
        for (int h = 0; h < 2; ++h)
            if (cp.pid[h] != 0xFFFFFFFFu) {
                nmax = std::max(nmax, dp[cp.pid[h]].n);
                mmax = std::max(mmax, dp[cp.pid[h]].m);
            }
        for (uint32_t b = 0; b < cp.nbands; ++b) {
            rows[b] = int32_t(uint32_t(cp.bstart[b + 1u]) - uint32_t(cp.bstart[b])) * CK2;
            lo[b] = cp.plo[b];
            hi[b] = cp.phi[b];
        }
        const int hr = ioc_host_align_corridor(q.data(), int32_t(d.n), r.data(), int32_t(d.m), P.match, P.mismatch, d.gap_open, P.gap_extend, rows,
                                               int32_t(cp.nbands), 64 * FW_C, lo, hi, nullptr, 0, out);
        const bool own = e.start != INT32_MAX, largest = d.n == nmax && d.m == mmax;
        const int32_t cert = own ? std::min(e.cert, std::max(e.start, e.exit)) : e.cert;
        const bool same = hr >= 0 && out[0] == he[pid].x && out[1] == he[pid].y && out[2] == he[pid].z && (largest ? e.cert == out[3] : e.cert >= out[3]) &&
                          (!own || (e.start == out[4] && e.exit == out[5])) && ((he[pid].w & 2) != 0) == (he[pid].x <= cert);
        if (!same)
            return ioc_fail(c, IOC_ERR_STATE, "IOC_V2_CERT_CHECK: slice " + std::to_string(si) + ": pair " + std::to_string(pid) + " (n " + std::to_string(d.n) +
                                                  ", m " + std::to_string(d.m) + ", half " + std::to_string(cp.pid[0] == pid ? 0 : 1) + "): the device has score " +
                                                  std::to_string(he[pid].x) + " at (" + std::to_string(he[pid].y) + ", " + std::to_string(he[pid].z) + "), flags " +
                                                  std::to_string(he[pid].w) + ", bounds " + std::to_string(e.cert) + " / " + std::to_string(e.start) + " / " +
                                                  std::to_string(e.exit) + "; the host (" + std::to_string(hr) + ") score " + std::to_string(out[0]) + " at (" +
                                                  std::to_string(out[1]) + ", " + std::to_string(out[2]) + "), bounds " + std::to_string(out[3]) + " / " +
                                                  std::to_string(out[4]) + " / " + std::to_string(out[5]));
        ++checked;
        tapered += own ? 1u : 0u;
        refuted += (he[pid].w & 2) ? 1u : 0u;
    }
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner v2: IOC_V2_CERT_CHECK: slice %zu: %u pairs equal the host's (%u with a tapered corridor, %u refuted)\n", si, checked,
                tapered, refuted);
    return IOC_OK;
}

// Version 2: the pairs order[0 .. cnt) (all of the query-profile kind, heaviest first) through k_fwd2 / k_fwd2_ends / k_trace2, with
// the corridor (`corridor` false: every tile).  Returns IOC_OK with *fell_back = true when a bounded wait of the forward pass ran
// out (the caller then runs the same pairs through version 1).
// `ops`: an emitting call (null otherwise).
int align_v2_run(ioc_ctx* c, const std::vector<AlnPairDev>& dp, const uint32_t* order, uint32_t cnt, const uint32_t* d_order,
                 const AlnParams& P, const AlnPlanOpts& po, int32_t* d_score, uint32_t* d_count, bool corridor, bool* fell_back, OpsRun* ops,
                 StageTrace& tr)
{
    *fell_back = false;
    if (cnt == 0) return IOC_OK;
    int r;
    const auto t_plan0 = std::chrono::steady_clock::now();  // (IOC_TRACE: host time of the planning up to the first launch)
    V2Opts o{};
    o.n_cu = compute_units(c);
    uint64_t budget = 0;
    if ((r = ck_budget(c, &budget, ops ? ops->host->pile_bytes() : 0)) != IOC_OK) return r;
    // the 16-bit window's guard (|relative score| at a rebase): a pair beyond it is flagged and re-run by version 1
    o.guard = P16_GUARD;
    if (const char* e = getenv("IOC_ALIGN_V2_GUARD")) o.guard = std::max(1, std::min(P16_GUARD, atoi(e)));
    o.few_limit = po.few_limit;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o.occ, reinterpret_cast<const void*>(k_fwd2), 64 * V2_WAVES, 0) != hipSuccess) o.occ = 0;
    (void)hipGetLastError();
    if (o.occ < 1) o.occ = 3;
    tr.mark("budget, occupancy");

    V2Plan pl;
    pl.cnt = cnt;
    pl.np = uint32_t(dp.size());
    pl.ncouples = (cnt + 1u) / 2u;
    const uint32_t want_bands = band_target(pl.ncouples, o.few_limit, o.occ, o.n_cu);
    if (getenv("IOC_TRACE"))  // (which shape the call runs in: tests/test_gpu_align_shapes.py reads this line and v2_slice's)
        fprintf(stderr, "[ioc]   aligner v2: shape: %u couples, band target %u, few_limit %u, occ %d, n_cu %d\n", pl.ncouples, want_bands, o.few_limit, o.occ,
                o.n_cu);
    const bool fit_sig_ok = c->aln_fit_sig[0] == P.match && c->aln_fit_sig[1] == P.mismatch && c->aln_fit_sig[2] == P.gap_extend;
    plan_couples(pl, dp, order, corridor_model(P, corridor, po, c->aln_fit, fit_sig_ok), want_bands);
    tr.mark("plan_couples");
    std::vector<uint64_t> cops;  // (emitting call) the operation bytes of a couple's pairs: query length + reference length each
    if (ops) {
        cops.assign(pl.ncouples, 0);
        for (uint32_t x = 0; x < cnt; ++x) cops[x / 2u] += uint64_t(dp[order[x]].n) + dp[order[x]].m;
    }
    slice_couples(pl, budget, cops);
    tr.mark("slice_couples");
    std::vector<uint64_t> slice_ops(pl.slices.size(), 0);
    if (ops) {  // a slice's pairs, in the slice's order, one region behind the other
        ops->end.assign(dp.size(), 0);
        uint64_t most = 0;
        for (size_t si = 0; si < pl.slices.size(); ++si) {
            const uint32_t x0 = 2u * pl.slices[si].first, x1 = std::min(cnt, 2u * (pl.slices[si].first + pl.slices[si].second));
            for (uint32_t x = x0; x < x1; ++x) ops->end[order[x]] = slice_ops[si] += uint64_t(dp[order[x]].n) + dp[order[x]].m;
            most = std::max(most, slice_ops[si]);
        }
        if ((r = ops_reserve(c, *ops, most, dp)) != IOC_OK) return r;
    }
    const auto t_res0 = std::chrono::steady_clock::now();
    IOC_TRY(ioc_reserve(c, c->a_ck, size_t(pl.arena_words) * 4));
    c->tm.align_arena_bytes = int64_t(pl.arena_words) * 4;
    c->tm.align_slices = int32_t(pl.slices.size());
    c->tm.align_version = 2;
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner v2: %u couples, checkpoint arena %.1f MB (%zu slice(s)) reserved in %.3f ms; corridor: %llu of %llu tiles skipped\n", pl.ncouples,
                double(pl.arena_words) * 4e-6, pl.slices.size(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_res0).count(),
                (unsigned long long)pl.tiles_skipped, (unsigned long long)pl.tiles_all);
    tr.mark("arena reserve");
    tile_counts(pl);
    if (getenv("IOC_V2_ITEMS_CHECK")) {
        const std::string differs = tile_lists_check(pl);
        if (!differs.empty()) return ioc_fail(c, IOC_ERR_STATE, differs);
    }
    tr.mark("tile_counts");

    o.deadline = 4;  // (blocks of slack on top of what a pair of one transcript needs to be decided: 2 per 512 windows of its threshold)
    if (const char* e = getenv("IOC_TRACE2_DEADLINE")) o.deadline = uint32_t(std::max(0, atoi(e)));
    if (const char* e = getenv("IOC_TRACE2_CYCLES")) o.deadline_cycles = (unsigned long long)std::max(0.0, atof(e));
    o.help_wgs = o.deadline ? std::min<uint32_t>(pl.max_pairs, uint32_t(o.n_cu)) : 0u;
    V2Dev t{};
    if ((r = v2_tables(c, pl, o.help_wgs, t)) != IOC_OK) return r;
    tr.mark("v2_tables");
    // The helper launch for the wrong candidates runs on a side stream BESIDE the first traceback launch (IOC_TRACE2_EARLY=0:
    // everything goes through the first launch, as before): their walks are the longest of the batch, and the first launch — one
    // pair's latency long, with the chip half empty — no longer waits for them to reach their deadline first.
    o.side_help = o.deadline && !(getenv("IOC_TRACE2_EARLY") && atoi(getenv("IOC_TRACE2_EARLY")) == 0);
    if (o.side_help && !c->side_stream) {
        IOC_CHK(c, hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
        for (auto& e : c->ev_side) IOC_CHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    EventSet evs;
    evs.v.assign(pl.slices.size() * 3, nullptr);
    for (auto& e : evs.v) IOC_CHK(c, hipEventCreate(&e));
    tr.mark("side stream, events");
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner v2: planning (couples, corridors, tile lists, tables) took the host %.3f ms\n",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_plan0).count());
    size_t evi = 0;
    bool bad = false;
    uint32_t link_sum[3] = {0, 0, 0};  // (IOC_TRACE: tiles computed, links without a left side, links with the left tile done)
    for (size_t si = 0; si < pl.slices.size() && !bad; ++si, evi += 3) {
        uint32_t xe = 0;
        if ((r = v2_slice(c, pl, t, si, o, P, d_order, d_score, d_count, &evs.v[evi], &xe, link_sum, ops ? &ops->dev : nullptr, tr)) != IOC_OK) return r;
        if (ops && !xe) {
            const uint32_t x0 = 2u * pl.slices[si].first, x1 = std::min(cnt, 2u * (pl.slices[si].first + pl.slices[si].second));
            if ((r = ops_fetch(c, *ops, dp, order + x0, d_order + x0, x1 - x0, slice_ops[si])) != IOC_OK) return r;
        }
        if ((r = v2_report(c, dp, order, pl, t, si, o.deadline)) != IOC_OK) return r;
        if (!xe && pl.tiles_skipped && getenv("IOC_V2_CERT_CHECK") && (r = v2_cert_check(c, dp, order, pl, t, si, P)) != IOC_OK) return r;
        bad = xe != 0;
    }
    add_elapsed(c, evs.v, evi);
    tr.mark("elapsed times");
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner v2: links: %u of %u (%u without a left side, %u with the left tile done)\n", link_sum[1] + link_sum[2], link_sum[0],
                link_sum[1], link_sum[2]);
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner v2: forward %.3f ms, traceback %.3f ms (device, all slices so far)%s\n", c->tm.ms_align_fwd,
                c->tm.ms_align_trace, bad ? " — a wait ran out: falling back to version 1" : "");
    *fell_back = bad;
    return IOC_OK;
}

// ---- ioc_align_pairs, stage by stage ------------------------------------------------------------------------------------

// which pairs a call may send where: everything (normal), the same without a corridor (the re-run of pairs the corridor could not
// vouch for), or version 1 alone (the re-run of pairs version 2's 16-bit window refused)
enum class AlnRoute { normal, every_tile, v1_only };

// the caller's answer arrays (each may be null)
struct AlnOut {
    int32_t* score;
    int64_t* windows;
    double* ratio;
    const AlnSink* ops = nullptr;  // an emitting call (ioc_align_pairs_ops): where the operation bytes go
    void set(size_t i, int32_t s, int64_t w, double r) const
    {
        if (score) score[i] = s;
        if (windows) windows[i] = w;
        if (ratio) ratio[i] = r;
    }
};

// the pairs of a call that need the device
struct AlnBatch {
    std::vector<AlnPairDev> dp;
    std::vector<uint32_t> back;   // device pair -> caller pair
    std::vector<uint32_t> order;  // the device pairs in the order the launches take them
    uint32_t max_n = 1, max_m = 1;
};

// 1. the device records; a pair with an empty sequence is answered here
int prepare_pairs(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, const AlnParams& P, const AlnOut& out, AlnBatch& b)
{
    const int32_t k = int32_t(P.k);
    // what the call refuses, before any answer is written (the accepted ranges: isonclust2_hip.h, next to ioc_align_pairs)
    if (!aln_params_ok(P.match, P.mismatch, P.gap_extend))
        return ioc_fail(c, IOC_ERR_ARG, "GPU aligner: gap_extend must be >= 0 and max(|match|, |mismatch|) + 2 gap_extend + 5 at most 2^24");
    for (int32_t i = 0; i < n_pairs; ++i) {
        IOC_TRY(ioc_pair_in_pool(c, pairs[i]));
        const int64_t n = ioc_seq_len(c, pairs[i].query), m = ioc_seq_len(c, pairs[i].ref);
        if (n + m >= (int64_t(1) << ALN_LEN_SHIFT))
            return ioc_fail(c, IOC_ERR_CAPACITY, "GPU aligner: sequences above 2^26 bases");
        if (n > 0 && m > 0 && !aln_span_ok(P.match, P.mismatch, P.gap_extend, n, m))
            return ioc_fail(c, IOC_ERR_ARG, "GPU aligner: (max(|match|, |mismatch|) + 2 gap_extend + 5) x (" + std::to_string(n) + " + " + std::to_string(m) +
                                                " bases) is above 2^30: the scores of this pair do not fit the kernels' 32-bit cells");
    }
    b.dp.reserve(size_t(n_pairs));
    for (int32_t i = 0; i < n_pairs; ++i) {
        const ioc_aln_pair& a = pairs[i];
        const int64_t n = ioc_seq_len(c, a.query), m = ioc_seq_len(c, a.ref);
        const double limit = std::floor((1.0 - a.e) * double(k));  // getAlnRatio, cluster.cpp:446
        const int32_t il = limit < -1.0 ? -1 : limit > 64.0 ? 64 : int32_t(limit);
        if (n == 0 || m == 0) {
            // nothing to align: the comparison string is n + m blanks
            const int64_t len = n + m;
            const int64_t cnt = (il <= 0 && len > k) ? len - k : 0;
            out.set(size_t(i), 0, cnt, n == 0 ? 0.0 : double(cnt) / double(n));
            if (out.ops) out.ops->answer_empty(size_t(i), n, m);  // (all of it one free end gap, and no walk)
            continue;
        }
        AlnPairDev d{};
        d.q_off = uint32_t(c->aln_offs[size_t(a.query)]);
        d.n = uint32_t(n);
        d.r_off = uint32_t(c->aln_offs[size_t(a.ref)]);
        d.m = uint32_t(m);
        d.gap_open = ioc_host_gap_open(a.e);
        d.e_sum = float(a.e);
        d.ilimit = il;
        d.rc = a.ref_revcomp ? 1u : 0u;
        d.stop_at = 0;
        if (c->aln_verdict_thr > 0.0 && n > 0 && !out.ops) {  // (an emitting call is always exact)
            // smallest count a with double(a) / double(n) >= threshold: the comparison the caller will make (getAlnRatio / slen)
            double a0 = std::ceil(c->aln_verdict_thr * double(n));
            while (a0 > 0 && (a0 - 1.0) / double(n) >= c->aln_verdict_thr) a0 -= 1.0;
            while (a0 / double(n) < c->aln_verdict_thr) a0 += 1.0;
            d.stop_at = a0 >= 1.0 && a0 < 4.0e9 ? uint32_t(a0) : 0u;
        }
        // the kernel family (aln_route, ioc_align_sink.h), in `pad`: 0 the comparing kernel — also for every pair with a letter
        // other than A C G T —, 1 the query-profile kernel of version 1, 2 version 2 may take the pair
        const bool four = !c->aln_other[size_t(a.query)] && !c->aln_other[size_t(a.ref)] && !getenv("IOC_ALIGN_NO_PROFILE");
        d.pad = four ? uint32_t(aln_route(P.match, P.mismatch, P.gap_extend, d.gap_open)) : uint32_t(ALN_ROUTE_COMPARE);
        b.dp.push_back(d);
        b.back.push_back(uint32_t(i));
        b.max_n = std::max(b.max_n, d.n);
        b.max_m = std::max(b.max_m, d.m);
    }
    return IOC_OK;
}

// 2. the order of the launches (stable sorts and partitions: order only, never a result)
void order_pairs(AlnBatch& b, const ioc_aln_pair* pairs)
{
    const std::vector<AlnPairDev>& dp = b.dp;
    const uint32_t np = uint32_t(dp.size());
    std::vector<uint32_t>& order = b.order;
    // heaviest pairs first
    order.resize(np);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        return uint64_t(dp[x].n) * dp[x].m > uint64_t(dp[y].n) * dp[y].m;
    });
    // Pairs with the same tile grid (coarse rows x strips) in the order of their summed error rates: a couple's corridor is as wide as
    // its less similar pair needs (align_v2_run), so like goes with like.
    {
        auto rows = [&](uint32_t x) { return uint64_t((dp[x].n + 511u) / 512u); };
        auto cols = [&](uint32_t x) { return uint64_t((dp[x].m + 511u) / 512u); };
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
            const uint64_t tx = rows(x) * cols(x), ty = rows(y) * cols(y);
            if (tx != ty) return tx > ty;  // (heaviest first, as before — by tiles)
            if (rows(x) != rows(y)) return rows(x) > rows(y);
            return dp[x].e_sum > dp[y].e_sum;
        });
    }
    // The caller's similarity hints (ioc_aln_pair::reserved, 0 = none): pairs hinted far below the batch's median — a quarter of
    // it — are taken for unrelated and sorted behind the others, so that version 2 couples them with each other: a couple with
    // an unrelated pair gets no corridor, and a pair of one transcript coupled with it pays for every tile too (config 3: 19 %
    // of the couples hold a wrong candidate when they are coupled by size alone, 10 % of the pairs are one).
    {
        std::vector<int32_t> hp;
        for (uint32_t x = 0; x < np; ++x)
            if (pairs[b.back[x]].reserved > 0) hp.push_back(pairs[b.back[x]].reserved);
        if (hp.size() >= 8 && !getenv("IOC_ALIGN_NO_HINTS")) {
            std::nth_element(hp.begin(), hp.begin() + long(hp.size() / 2), hp.end());
            const int64_t med = hp[hp.size() / 2];
            std::stable_partition(order.begin(), order.end(), [&](uint32_t x) {
                const int64_t h = pairs[b.back[x]].reserved;
                return !(h > 0 && h * 4 < med);
            });
        }
    }
    // trace variant: version 2's pairs first, then the other pairs of the query-profile kernel, the comparing kernel's after them
    std::stable_partition(order.begin(), order.end(), [&](uint32_t x) { return dp[x].pad != 0; });
    std::stable_partition(order.begin(), order.end(), [&](uint32_t x) { return dp[x].pad == uint32_t(ALN_ROUTE_V2); });
}

// 3. waves per pair: plan_waves (ioc_align_plan.h)

// 4. version 2 takes the pairs it may (aln_v2_ok) — the front of `order`; *n_v2: how many it answered (0 when a bounded wait ran out
// and they all go to version 1)
int run_v2(ioc_ctx* c, const AlnBatch& b, const AlnParams& P, const AlnPlanOpts& po, int32_t* d_score, uint32_t* d_count, AlnRoute route, uint32_t* n_v2,
           const AlnSink* oh, StageTrace& tr)
{
    const uint32_t np = uint32_t(b.dp.size());
    uint32_t n = 0;
    while (n < np && b.dp[b.order[n]].pad == uint32_t(ALN_ROUTE_V2)) ++n;
    bool fell_back = false;
    OpsRun ops{oh, b.back.data()};
    const int r = align_v2_run(c, b.dp, b.order.data(), n, static_cast<const uint32_t*>(c->a_order.p), P, po, d_score, d_count, route != AlnRoute::every_tile,
                               &fell_back, oh ? &ops : nullptr, tr);
    if (r != IOC_OK) return r;
    if (fell_back) {
        c->tm.n_align_refused += n;
        n = 0;
    }
    *n_v2 = n;
    return IOC_OK;
}

// 5. the carry variant (IOC_ALIGN_VARIANT=carry): every pair, in slices when the whole batch would not fit the budget
int run_carry(ioc_ctx* c, const AlnBatch& b, uint32_t waves, const AlnParams& P, int32_t* d_score, uint32_t* d_count)
{
    const uint32_t np = uint32_t(b.dp.size()), NT = waves * 64;
    const uint64_t bnd_stride = 2ull * 6ull * b.max_n;
    const uint64_t lrow_entries = uint64_t((b.max_m + NT * ALN_C - 1) / (NT * ALN_C)) * NT;
    const uint64_t lrow_stride = lrow_entries * 4ull;
    // scratch is per workgroup
    const uint64_t budget = 8ull << 30;
    const uint64_t per_pair = (bnd_stride + lrow_stride) * 4ull;
    const uint32_t slice = uint32_t(std::min<uint64_t>(np, std::max<uint64_t>(1, budget / per_pair)));
    IOC_TRY(ioc_reserve(c, c->a_bnd, size_t(slice) * bnd_stride * 4));
    IOC_TRY(ioc_reserve(c, c->a_lrow, size_t(slice) * lrow_stride * 4));
    for (uint32_t first = 0; first < np; first += slice) {
        const uint32_t cnt = std::min(slice, np - first);
        hipLaunchKernelGGL(k_align_carry, dim3(cnt), dim3(NT), 0, c->stream, static_cast<const AlnPairDev*>(c->a_pairs.p),
                           static_cast<const uint32_t*>(c->a_order.p) + first, static_cast<const uint8_t*>(c->a_pool.p), P,
                           static_cast<uint32_t*>(c->a_bnd.p), bnd_stride, static_cast<uint32_t*>(c->a_lrow.p), lrow_stride, d_score, d_count);
        IOC_CHK(c, hipGetLastError());
    }
    return IOC_OK;
}

// ---- 6. version 1 ---------------------------------------------------------------------------------------------------------

// The static LDS of a k_align_fwd variant (`fallback` when the runtime cannot tell), and the most dynamic LDS one of its
// workgroups may reserve on top: more than the default 64 KB per workgroup needs the kernel attribute, asked for once per
// variant and context (best effort).
size_t fwd_lds_limit(ioc_ctx* c, bool prof, const void* kfn, size_t fallback, size_t* stat)
{
    hipFuncAttributes fa{};
    *stat = fallback;
    if (hipFuncGetAttributes(&fa, kfn) == hipSuccess) *stat = fa.sharedSizeBytes;
    size_t& lim = prof ? c->aln_lds_max : c->aln_lds_max2;
    if (lim == 0) {
        int mx = 0;
        (void)hipDeviceGetAttribute(&mx, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device);
        lim = 64 * 1024 > *stat ? 64 * 1024 - *stat : 1;
        if (mx > 72 * 1024 && hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, mx - int(*stat)) == hipSuccess)
            lim = size_t(mx) - *stat;
        (void)hipGetLastError();
    }
    return lim;
}

// version 1's forward pass over the pairs o[0 .. cnt) of a slice (k_align_fwd, see there for the arguments)
struct V1Fwd {
    ioc_ctx* c;
    bool prof;
    AlnParams P;
    uint64_t lrow_stride;
    int operator()(const uint32_t* o, uint32_t cnt, uint32_t wv, uint32_t wgw, uint32_t nwg, uint32_t nmain, uint32_t wtail, size_t lds,
                   uint32_t lrow_first, const AlnCross& X) const
    {
        const AlnPairDev* dpairs = static_cast<const AlnPairDev*>(c->a_pairs.p);
        const uint8_t* dpool = static_cast<const uint8_t*>(c->a_pool.p);
        int2* dck = static_cast<int2*>(c->a_ck.p);
        const AlnCk* dcko = static_cast<const AlnCk*>(c->a_cko.p);
        int2* lr = static_cast<int2*>(c->a_lrow.p) + uint64_t(lrow_first) * lrow_stride;
        int4* dends = static_cast<int4*>(c->a_ends2.p);
        if (prof)
            hipLaunchKernelGGL(k_align_fwd<true>, dim3(nwg), dim3(wgw * 64), lds, c->stream, dpairs, o, cnt, wv, nmain, wtail, dpool, P, dck, dcko, lr,
                               lrow_stride, dends, X);
        else
            hipLaunchKernelGGL(k_align_fwd<false>, dim3(nwg), dim3(wgw * 64), lds, c->stream, dpairs, o, cnt, wv, nmain, wtail, dpool, P, dck, dcko, lr,
                               lrow_stride, dends, X);
        IOC_CHK(c, hipGetLastError());
        return IOC_OK;
    }
};

// The tail generation of a slice — its pairs from `first_cnt` on — split over `groups` workgroups each, the first band of a
// workgroup waiting on a flag for the row checkpoints of the band above.  `inl`: in the SAME launch as the ordinary workgroups
// (n_main of them), behind them; otherwise in a launch of its own.  The waits are bounded: when one runs out (the workgroups
// were not all resident) the tail is done again the usual way.
int v1_cross_tail(ioc_ctx* c, const AlnBatch& b, const V1Fwd& fwd, const std::pair<uint32_t, uint32_t>& sl, uint32_t waves, uint32_t wg_waves,
                  uint32_t n_main, uint32_t ppw, uint32_t groups, bool inl, size_t lds_pad, const void* kfn)
{
    hipStream_t s = c->stream;
    const uint32_t* ord = static_cast<const uint32_t*>(c->a_order.p) + sl.first;
    const uint32_t first_cnt = n_main * ppw, rest = sl.second - first_cnt, nb = 4 * groups;
    // flags are indexed [band][strip] with every pair's OWN strip count: a pair with fewer cells than the slice's first one may
    // still have the longer reference, so the slot holds the largest count of the pairs that are actually split
    uint32_t strips = 1;
    for (uint32_t x = first_cnt; x < sl.second; ++x) strips = std::max(strips, (b.dp[b.order[sl.first + x]].m + 64 * FW_C - 1) / (64 * FW_C));
    AlnCross X;
    X.groups = groups;
    X.flag_stride = nb * strips;
    const size_t fbytes = size_t(rest) * X.flag_stride * 4, bbytes = size_t(rest) * nb * sizeof(int2);
    int r;
    IOC_TRY(ioc_reserve(c, c->a_xflags, fbytes + bbytes + 64));
    X.err = static_cast<uint32_t*>(c->a_xflags.p);
    X.flags = X.err + 16;
    X.best = reinterpret_cast<int2*>(reinterpret_cast<uint8_t*>(c->a_xflags.p) + 64 + fbytes);
    IOC_CHK(c, hipMemsetAsync(c->a_xflags.p, 0, 64 + fbytes, s));
    if (inl && first_cnt) {
        // one launch: ordinary workgroups, then the split pairs behind them
        X.first_wg = n_main;
        X.first_pair = first_cnt;
        if ((r = fwd(ord, sl.second, waves, wg_waves, n_main + rest * groups, n_main + rest * groups, waves, lds_pad, 0, X)) != IOC_OK) return r;
    } else {
        if (first_cnt && (r = fwd(ord, first_cnt, waves, wg_waves, n_main, n_main, waves, lds_pad, 0, AlnCross{})) != IOC_OK) return r;
        size_t stat = 0, xlds = 0;  // more than half a CU's LDS: the dispatcher cannot stack two of them
        const size_t lim = fwd_lds_limit(c, fwd.prof, kfn, 52 * 1024, &stat), want = 84 * 1024;
        if (want > stat && want - stat <= lim) xlds = (want - stat) & ~size_t(255);
        if ((r = fwd(ord + first_cnt, rest, 4, 4, rest * groups, rest * groups, 4, xlds, first_cnt, X)) != IOC_OK) return r;
    }
    uint32_t xe = 0;
    IOC_CHK(c, hipMemcpyAsync(&xe, X.err, 4, hipMemcpyDeviceToHost, s));
    IOC_CHK(c, hipStreamSynchronize(s));
    if (xe) {  // a wait ran out: the tail again, the usual way
        if ((r = fwd(ord + first_cnt, rest, 4, 4, rest, rest, 4, 0, first_cnt, AlnCross{})) != IOC_OK) return r;
        c->tm.n_align_refused += rest;
    }
    return IOC_OK;
}

// one slice of version 1: the forward pass (ordinary workgroups, a partly filled second generation, or the split tail) and the
// traceback, events ev[0 .. 3) around them
int v1_slice(ioc_ctx* c, const AlnBatch& b, const std::pair<uint32_t, uint32_t>& sl, const WavePlan& wp, const AlnParams& P, int n_cu,
             uint64_t lrow_stride, int32_t* d_score, uint32_t* d_count, const hipEvent_t* ev, const AlnOpsDev* od)
{
    hipStream_t s = c->stream;
    const uint32_t waves = wp.waves;
    const uint32_t* ord = static_cast<const uint32_t*>(c->a_order.p) + sl.first;
    // Every workgroup lives for the whole launch (equal-sized pairs), so the launch ends with the
    // fullest CU: cap the residency at ceil(workgroups / CUs) per CU with an LDS reservation, or the
    // dispatcher may stack 8 workgroups on some CUs and leave others with 3.
    const bool prof = b.dp[b.order[sl.first]].pad != 0;
    const void* kfn = prof ? reinterpret_cast<const void*>(k_align_fwd<true>) : reinterpret_cast<const void*>(k_align_fwd<false>);
    const V1Fwd fwd{c, prof, P, lrow_stride};
    size_t lds_pad = 0;
    const uint32_t wg_waves = waves > 4 ? waves : 4, ppw = wg_waves / waves;
    uint32_t n_wg = (sl.second + ppw - 1) / ppw, n_main = n_wg, wpp_tail = waves;
    {   // a second, partly filled generation of workgroups: give its pairs twice the waves
        int occ = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kfn, int(wg_waves * 64), 0) != hipSuccess) occ = 0;
        (void)hipGetLastError();
        const uint32_t gen = uint32_t(occ > 0 ? occ : 3) * uint32_t(n_cu);  // resident workgroups
        if (n_wg > gen && n_wg < gen + gen / 2 && 2 * waves <= wg_waves) {
            n_main = gen;
            wpp_tail = 2 * waves;
            const uint32_t rest = sl.second - n_main * ppw, ppw_tail = wg_waves / wpp_tail;
            n_wg = n_main + (rest + ppw_tail - 1) / ppw_tail;
        }
    }
    const uint32_t per_cu = (n_main + uint32_t(n_cu) - 1) / uint32_t(n_cu);
    if (per_cu * wg_waves < 32) {
        // per-workgroup LDS (static + reservation) halfway between 160 KB / (per_cu + 1) and 160 KB / per_cu
        size_t stat = 0;
        const size_t lim = fwd_lds_limit(c, prof, kfn, 48 * 1024, &stat);
        const size_t want = size_t(160u * 1024u) * (2 * per_cu + 1) / (2 * per_cu * (per_cu + 1));
        lds_pad = want > stat + 1024 ? (want - stat - 512) & ~size_t(255) : 0;
        lds_pad = std::min(lds_pad, lim > 1 ? lim : 0);
    }
    IOC_CHK(c, hipEventRecord(ev[0], s));
    // The tail generation runs on a mostly empty chip: its pairs are split over SEVERAL workgroups each
    // (4 x 4 = 16 bands on 4 CUs; an 8-wave workgroup lands on one CU, two waves per SIMD, and was slower).
    uint32_t groups = 1;
    // the whole slice the tail's way: forced (tests), or a handful of pairs on an otherwise idle chip
    const bool force_cross = getenv("IOC_ALIGN_FORCE_CROSS") != nullptr || (wp.few_pairs && waves == 4);
    if (force_cross && wg_waves == 4) {
        n_main = 0;
        n_wg = 1;
    }
    // Default: in the SAME launch, behind the ordinary workgroups, so that a split pair starts on whatever CU
    // frees up first (config 3: 105.2 -> 96.0 ms).  A launch of its own (one workgroup per CU by an LDS reservation) was
    // measured slower — it cannot backfill, 112 ms — and is left to slices without ordinary workgroups (the forced split).
    // IOC_ALIGN_NO_CROSS_TAIL=1 keeps the tail pairs whole with twice the waves (the first version).
    // Workgroups of a launch are handed out in index order and a workgroup only waits for a smaller index;
    // the split ones are at most two thirds of an XCD's slots, so they can never fill an XCD with waiters.
    const bool inl = !force_cross;
    if (n_main < n_wg && wg_waves == 4 && !getenv("IOC_ALIGN_NO_CROSS_TAIL")) {
        const AlnPairDev& big = b.dp[b.order[sl.first]];
        const uint32_t strips = (big.m + 64 * FW_C - 1) / (64 * FW_C), tiles = (big.n + TILE - 1) / TILE;
        groups = force_cross ? 4 : 2;  // (behind a full generation 4 was measured slower: 99 ms)
        if (const char* eg = getenv("IOC_ALIGN_CROSS_GROUPS")) groups = uint32_t(std::max(1, std::min(4, atoi(eg))));
        while (groups > 1 && (strips < 4 * groups || tiles < 8 * groups)) groups >>= 1;  // bands = 4 * groups
        const uint32_t rest = sl.second - n_main * ppw;
        // one workgroup per CU (two on a CU run at half speed and hold up the whole chain of their pair), all
        // resident together
        // (in-launch: at most 2 split workgroups per CU's worth, i.e. 64 of an XCD's 96 slots — waiters cannot
        // fill an XCD; a launch of its own: one per CU)
        while (groups > 1 && uint64_t(rest) * groups > uint64_t(inl ? 2 : 1) * uint64_t(n_cu)) groups >>= 1;
    }
    int r;
    if (groups > 1) {
        if ((r = v1_cross_tail(c, b, fwd, sl, waves, wg_waves, n_main, ppw, groups, inl, lds_pad, kfn)) != IOC_OK) return r;
    } else {
        if (force_cross && n_main == 0) {  // (the forced split did not fit this slice)
            n_wg = (sl.second + ppw - 1) / ppw;
            n_main = n_wg;
        }
        if ((r = fwd(ord, sl.second, waves, wg_waves, n_wg, n_main, wpp_tail, lds_pad, 0, AlnCross{})) != IOC_OK) return r;
    }
    IOC_CHK(c, hipEventRecord(ev[1], s));
    const uint32_t tr_wg = (sl.second + TR_WAVES - 1) / TR_WAVES;  // (an LDS reservation that caps the workgroups per CU changed nothing here)
    if (od)
        hipLaunchKernelGGL(k_align_trace_ops, dim3(tr_wg), dim3(64 * TR_WAVES), 0, s, static_cast<const AlnPairDev*>(c->a_pairs.p), ord,
                           static_cast<const uint8_t*>(c->a_pool.p), P, static_cast<const int2*>(c->a_ck.p), static_cast<const AlnCk*>(c->a_cko.p),
                           static_cast<const int4*>(c->a_ends2.p), d_score, d_count, sl.second, *od);
    else
        hipLaunchKernelGGL(k_align_trace, dim3(tr_wg), dim3(64 * TR_WAVES), 0, s, static_cast<const AlnPairDev*>(c->a_pairs.p), ord,
                           static_cast<const uint8_t*>(c->a_pool.p), P, static_cast<const int2*>(c->a_ck.p), static_cast<const AlnCk*>(c->a_cko.p),
                           static_cast<const int4*>(c->a_ends2.p), d_score, d_count, sl.second);
    IOC_CHK(c, hipGetLastError());
    IOC_CHK(c, hipEventRecord(ev[2], s));
    return IOC_OK;
}

// Version 1 takes the pairs from order[n_v2] on: pairs with other letters, pairs the 16-bit window refused, the whole batch
// should a bounded wait of version 2 run out, and everything under IOC_ALIGN_V1=1 or IOC_ALIGN_ARENA=fat.
int run_v1(ioc_ctx* c, const AlnBatch& b, uint32_t n_v2, const WavePlan& wp, const AlnParams& P, int32_t* d_score, uint32_t* d_count, const AlnSink* oh)
{
    hipStream_t s = c->stream;
    const uint32_t np = uint32_t(b.dp.size());
    int r;
    uint64_t budget = 0;
    if ((r = ck_budget(c, &budget, oh ? oh->pile_bytes() : 0)) != IOC_OK) return r;
    const uint64_t lrow_stride = uint64_t((b.max_m + 64 * FW_C - 1) / (64 * FW_C)) * 64;  // int2 per pair
    // (the forward pass addresses a pair's row checkpoints by a 32-bit offset in ints: 2^29 int2 units = 4 GB per pair,
    // reads of ~260 kb against each other)
    for (const AlnPairDev& d : b.dp)
        if (v1_row_units(d) >= (uint64_t(1) << 29))
            return ioc_fail(c, IOC_ERR_CAPACITY, "alignment of " + std::to_string(d.n) + " x " + std::to_string(d.m) + " bases: row checkpoints above 4 GB per pair");
    V1Plan pl = plan_v1(b.dp, b.order.data(), n_v2, budget, oh != nullptr);
    OpsRun ops{oh, b.back.data()};
    if (oh) {
        ops.end.swap(pl.ops_end);
        if ((r = ops_reserve(c, ops, pl.ops_most, b.dp)) != IOC_OK) return r;
    }
    const auto t_res0 = std::chrono::steady_clock::now();
    IOC_TRY(ioc_reserve(c, c->a_ck, size_t(pl.arena) * 8));
    c->tm.align_arena_bytes = int64_t(pl.arena) * 8;
    c->tm.align_slices = int32_t(pl.slices.size());
    c->tm.align_version = 1;
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner: checkpoint arena %.1f MB (%zu slice(s)) reserved in %.3f ms\n", double(pl.arena) * 8e-6, pl.slices.size(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_res0).count());
    IOC_TRY(ioc_reserve(c, c->a_cko, size_t(np) * sizeof(AlnCk)));
    IOC_TRY(ioc_reserve(c, c->a_ends2, size_t(np) * sizeof(int4)));
    IOC_TRY(ioc_reserve(c, c->a_lrow, size_t(pl.max_cnt) * lrow_stride * 8));
    IOC_CHK(c, hipMemcpyAsync(c->a_cko.p, pl.cko.data(), size_t(np) * sizeof(AlnCk), hipMemcpyHostToDevice, s));
    const int n_cu = compute_units(c);
    EventSet evs;
    evs.v.assign(pl.slices.size() * 3, nullptr);
    for (auto& e : evs.v) IOC_CHK(c, hipEventCreate(&e));
    for (size_t si = 0; si < pl.slices.size(); ++si) {
        if ((r = v1_slice(c, b, pl.slices[si], wp, P, n_cu, lrow_stride, d_score, d_count, &evs.v[3 * si], oh ? &ops.dev : nullptr)) != IOC_OK) return r;
        if (oh && (r = ops_fetch(c, ops, b.dp, b.order.data() + pl.slices[si].first, static_cast<const uint32_t*>(c->a_order.p) + pl.slices[si].first,
                                  pl.slices[si].second, pl.slice_ops[si])) != IOC_OK)
            return r;
    }
    IOC_CHK(c, hipStreamSynchronize(s));
    add_elapsed(c, evs.v, evs.v.size());
    if (getenv("IOC_TRACE"))
        fprintf(stderr, "[ioc]   aligner: forward %.3f ms, traceback %.3f ms (device, all slices so far)\n", c->tm.ms_align_fwd, c->tm.ms_align_trace);
    return IOC_OK;
}

// ---- 7. read back -------------------------------------------------------------------------------------------------------

// what the corridor model learns from a batch (ioc_ctx::aln_fit): related pairs long enough to have had a corridor
void learn_corridor(ioc_ctx* c, const AlnBatch& b, const AlnParams& P, const std::vector<int32_t>& hs, const std::vector<uint32_t>& hc)
{
    if (c->aln_fit_sig[0] != P.match || c->aln_fit_sig[1] != P.mismatch || c->aln_fit_sig[2] != P.gap_extend) {
        for (auto& f : c->aln_fit) f = CorridorFit();
        c->aln_fit_sig[0] = P.match, c->aln_fit_sig[1] = P.mismatch, c->aln_fit_sig[2] = P.gap_extend;
    }
    for (size_t x = 0; x < b.dp.size(); ++x) {
        const AlnPairDev& d = b.dp[x];
        const uint32_t len = std::max(d.n, d.m);
        if (hc[x] == 0xFFFFFFFFu || len < 4096u || !(d.e_sum > 0.0f) || std::min(d.n, d.m) * 10u < len * 9u) continue;
        const double rho = double(hs[x]) / double(len), e = double(d.e_sum);
        if (rho * 2.0 < double(P.match)) continue;  // (not a pair of one transcript)
        CorridorFit& f = c->aln_fit[std::max(2, std::min(5, d.gap_open)) - 2];
        if (f.n >= 1e6) continue;  // (enough)
        f.n += 1.0, f.se += e, f.sr += rho, f.see += e * e, f.ser += e * rho, f.srr += rho * rho;
        f.e_lo = std::min(f.e_lo, e), f.e_hi = std::max(f.e_hi, e);
    }
}

// the statistics of the call and its answers (score, windows) on the host
int read_results(ioc_ctx* c, const AlnBatch& b, uint32_t n_v2, const int32_t* d_score, const uint32_t* d_count, std::vector<int32_t>& hs,
                 std::vector<uint32_t>& hc)
{
    const uint32_t np = uint32_t(b.dp.size());
    c->tm.n_align_pairs += np;
    for (auto& d : b.dp) c->tm.n_align_cells += int64_t(d.n) * int64_t(d.m);
    for (uint32_t x = n_v2; x < np; ++x)  // (version 1: every cell; version 2 counts its tiles)
        c->tm.n_align_cells_computed += int64_t(b.dp[b.order[x]].n) * int64_t(b.dp[b.order[x]].m);
    hs.resize(np);
    hc.resize(np);
    IOC_CHK(c, hipMemcpyAsync(hs.data(), d_score, size_t(np) * 4, hipMemcpyDeviceToHost, c->stream));
    IOC_CHK(c, hipMemcpyAsync(hc.data(), d_count, size_t(np) * 4, hipMemcpyDeviceToHost, c->stream));
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    return IOC_OK;
}

// ---- 8. answers and re-runs ---------------------------------------------------------------------------------------------

int align_pairs(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                const AlnOut& out, AlnRoute route);

// the caller's pairs `idx` once more, by `route`, their answers in the caller's arrays
int align_again(ioc_ctx* c, const ioc_aln_pair* pairs, const std::vector<int32_t>& idx, const AlnParams& P, AlnRoute route, const AlnOut& out)
{
    std::vector<ioc_aln_pair> sub(idx.size());
    std::vector<int32_t> sc(idx.size());
    std::vector<int64_t> sw(idx.size());
    std::vector<double> sr(idx.size());
    for (size_t x = 0; x < idx.size(); ++x) sub[x] = pairs[idx[x]];
    // (emitting call: the re-run writes straight into the regions of the caller's pairs — the bytes of the run that counted — and
    // adds into the same tables, at their own rows)
    const AlnSubSink sub_ops = out.ops ? out.ops->subset(idx) : AlnSubSink();
    const int r = align_pairs(c, int32_t(sub.size()), sub.data(), int32_t(P.k), P.match, P.mismatch, P.gap_extend,
                              AlnOut{sc.data(), sw.data(), sr.data(), out.ops ? &sub_ops.sink : nullptr}, route);
    if (r != IOC_OK) return r;
    for (size_t x = 0; x < idx.size(); ++x) out.set(size_t(idx[x]), sc[x], sw[x], sr[x]);
    if (out.ops) out.ops->take_back(idx, sub_ops);
    return IOC_OK;
}

// The answers into the caller's arrays; version 2's pairs that came back without one are run again.  The statistics count
// the two re-runs differently (kept as they have always been): a pair the corridor could not vouch for counts once in
// n_align_pairs / n_align_cells (its re-run's counts are taken back), a pair the 16-bit window refused counts twice there and
// once more in n_align_refused.  align_version / align_slices / align_arena_bytes are the last run's, a re-run's included.
int scatter_results(ioc_ctx* c, const AlnBatch& b, const ioc_aln_pair* pairs, bool v2, const AlnParams& P, const std::vector<int32_t>& hs,
                    const std::vector<uint32_t>& hc, const AlnOut& out)
{
    std::vector<int32_t> again;       // pairs version 2 refused: scores outside its 16-bit window
    std::vector<int32_t> again_full;  // pairs whose result the corridor cannot vouch for (V2Couple): every tile this time
    for (size_t x = 0; x < b.dp.size(); ++x) {
        const uint32_t i = b.back[x];
        if (v2 && hc[x] == 0xFFFFFFFFu && hs[x] == INT32_MIN) {
            again.push_back(int32_t(i));
            continue;
        }
        if (v2 && hc[x] == 0xFFFFFFFFu && hs[x] == INT32_MIN + 1) {
            again_full.push_back(int32_t(i));
            continue;
        }
        out.set(i, hs[x], int64_t(hc[x]), double(hc[x]) / double(b.dp[x].n));  // getAlnRatio: aligned / slen
    }
    int r;
    if (!again_full.empty()) {
        const int64_t pairs_so_far = c->tm.n_align_pairs, cells_so_far = c->tm.n_align_cells;
        if ((r = align_again(c, pairs, again_full, P, AlnRoute::every_tile, out)) != IOC_OK) return r;
        c->tm.n_align_pairs = pairs_so_far;
        c->tm.n_align_cells = cells_so_far;
        if (getenv("IOC_TRACE")) fprintf(stderr, "[ioc]   aligner v2: %zu of %zu pairs run again without a corridor\n", again_full.size(), b.dp.size());
    }
    if (!again.empty()) {
        if ((r = align_again(c, pairs, again, P, AlnRoute::v1_only, out)) != IOC_OK) return r;
        c->tm.n_align_refused += int64_t(again.size());
    }
    return IOC_OK;
}

// Version 2 (ioc_align_v2.inc) takes the query-profile pairs: two pairs per wave, tiles scheduled by dataflow, coarse checkpoints.
// IOC_ALIGN_V1=1 keeps everything on version 1.  IOC_ALIGN_ARENA=fat: a long-lived process that can spare the HBM (35 MB per
// 16.7 kb pair, 56 GB for config 3's batch, allocated once and kept) takes version 1 — fine checkpoints straight from the forward
// pass, a traceback half as long, ~6 % less time per batch.  The default is the lean version: a `cluster` process that starts by
// allocating tens of GB pays seconds for the driver to hand them out.
int align_pairs(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                const AlnOut& out, AlnRoute route)
{
    if (!c || n_pairs < 0 || (n_pairs > 0 && !pairs)) return IOC_ERR_ARG;
    if (k < 1 || k > 32) return ioc_fail(c, IOC_ERR_CAPACITY, "GPU aligner: window length k must be in 1..32");
    IOC_CHK(c, hipSetDevice(c->device));
    if (n_pairs == 0) return IOC_OK;
    const AlnParams P{match, mismatch, gap_extend, uint32_t(k), 1u << (32 - k)};
    AlnBatch b;
    int r;
    StageTrace tr;
    if ((r = prepare_pairs(c, n_pairs, pairs, P, out, b)) != IOC_OK) return r;
    tr.mark("prepare_pairs");
    const uint32_t np = uint32_t(b.dp.size());
    if (np == 0) return IOC_OK;
    order_pairs(b, pairs);
    tr.mark("order_pairs");
    const char* ev = getenv("IOC_ALIGN_VARIANT");
    const bool carry = ev && strcmp(ev, "carry") == 0 && !out.ops;  // (the carry variant has no walk: an emitting call takes the traced route)
    const AlnPlanOpts po = plan_opts();
    const WavePlan wp = plan_waves(b.max_n, b.max_m, np, carry, po);
    IOC_TRY(ioc_reserve(c, c->a_pairs, size_t(np) * sizeof(AlnPairDev)));
    IOC_TRY(ioc_reserve(c, c->a_order, size_t(np) * 4));
    IOC_TRY(ioc_reserve(c, c->a_out, size_t(np) * 8));
    IOC_CHK(c, hipMemcpyAsync(c->a_pairs.p, b.dp.data(), size_t(np) * sizeof(AlnPairDev), hipMemcpyHostToDevice, c->stream));
    IOC_CHK(c, hipMemcpyAsync(c->a_order.p, b.order.data(), size_t(np) * 4, hipMemcpyHostToDevice, c->stream));
    int32_t* d_score = static_cast<int32_t*>(c->a_out.p);
    uint32_t* d_count = reinterpret_cast<uint32_t*>(d_score + np);
    const char* arena_mode = getenv("IOC_ALIGN_ARENA");
    const bool v2 = route != AlnRoute::v1_only && !carry && !getenv("IOC_ALIGN_V1") && !(arena_mode && strcmp(arena_mode, "fat") == 0);
    uint32_t n_v2 = 0;
    tr.mark("pairs and order up");
    if (v2 && (r = run_v2(c, b, P, po, d_score, d_count, route, &n_v2, out.ops, tr)) != IOC_OK) return r;
    if (carry)
        r = run_carry(c, b, wp.waves, P, d_score, d_count);
    else if (n_v2 < np)
        r = run_v1(c, b, n_v2, wp, P, d_score, d_count, out.ops);
    if (r != IOC_OK) return r;
    std::vector<int32_t> hs;
    std::vector<uint32_t> hc;
    tr.mark("version 1 / carry");
    if ((r = read_results(c, b, n_v2, d_score, d_count, hs, hc)) != IOC_OK) return r;
    tr.mark("read_results");
    // (the corridor model learns from the pairs of a call's own version-2 run, never from a re-run's)
    if (v2 && route == AlnRoute::normal) learn_corridor(c, b, P, hs, hc);
    r = scatter_results(c, b, pairs, v2, P, hs, hc, out);
    tr.mark("scatter_results");
    return r;
}

}  // namespace

extern "C" {

int ioc_align_set_pool(ioc_ctx* c, int32_t n_seqs, const char* seqs, const int64_t* offs)
{
    if (!c || n_seqs < 0 || (n_seqs > 0 && (!seqs || !offs))) return IOC_ERR_ARG;
    IOC_CHK(c, hipSetDevice(c->device));
    c->res_pool_ready = false;
    c->aln_qual_set = false;
    c->aln_offs.assign(offs, offs + (n_seqs > 0 ? n_seqs + 1 : 0));
    if (n_seqs == 0) return IOC_OK;
    if (offs[0] != 0) return ioc_fail(c, IOC_ERR_ARG, "sequence pool offsets must start at 0");
    for (int32_t i = 0; i < n_seqs; ++i)
        if (offs[i + 1] < offs[i]) return ioc_fail(c, IOC_ERR_ARG, "sequence pool offsets must be ascending");
    const int64_t total = offs[n_seqs];
    if (total >= (int64_t(1) << 32)) return ioc_fail(c, IOC_ERR_CAPACITY, "sequence pool above 4 GiB");
    int r = ioc_reserve(c, c->a_pool, size_t(total));
    if (r != IOC_OK) return r;
    IOC_CHK(c, hipMemcpyAsync(c->a_pool.p, seqs, size_t(total), hipMemcpyHostToDevice, c->stream));
    // which sequences hold something else than A C G T
    IOC_TRY(ioc_reserve(c, c->a_ends, size_t(n_seqs + 1) * 8 + size_t(n_seqs)));
    int64_t* d_offs = static_cast<int64_t*>(c->a_ends.p);
    uint8_t* d_flags = reinterpret_cast<uint8_t*>(d_offs + n_seqs + 1);
    IOC_CHK(c, hipMemcpyAsync(d_offs, offs, size_t(n_seqs + 1) * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_seq_flags, dim3(uint32_t(n_seqs)), dim3(256), 0, c->stream,
                       static_cast<const uint8_t*>(c->a_pool.p), d_offs, d_flags);
    IOC_CHK(c, hipGetLastError());
    c->aln_other.assign(size_t(n_seqs), 0);
    IOC_CHK(c, hipMemcpyAsync(c->aln_other.data(), d_flags, size_t(n_seqs), hipMemcpyDeviceToHost, c->stream));
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    return IOC_OK;
}

int ioc_align_set_pool_qual(ioc_ctx* c, const char* quals, int64_t n_bytes)
{
    if (!c) return IOC_ERR_ARG;
    c->aln_qual_set = false;
    if (!quals) return IOC_OK;
    const int64_t total = c->aln_offs.empty() ? 0 : c->aln_offs.back();
    if (n_bytes != total) return ioc_fail(c, IOC_ERR_ARG, "ioc_align_set_pool_qual: " + std::to_string(n_bytes) + " quality bytes for a pool of " + std::to_string(total));
    IOC_CHK(c, hipSetDevice(c->device));
    IOC_TRY(ioc_reserve(c, c->a_qual, size_t(total)));
    if (total > 0) IOC_CHK(c, hipMemcpyAsync(c->a_qual.p, quals, size_t(total), hipMemcpyHostToDevice, c->stream));
    IOC_CHK(c, hipStreamSynchronize(c->stream));
    c->aln_qual_set = true;
    return IOC_OK;
}

int ioc_align_set_verdict_threshold(ioc_ctx* c, double aligned_threshold)
{
    if (!c) return IOC_ERR_ARG;
    c->aln_verdict_thr = aligned_threshold > 0.0 ? aligned_threshold : -1.0;
    return IOC_OK;
}

int ioc_align_pairs(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch,
                    int32_t gap_extend, int32_t* out_score, int64_t* out_windows, double* out_ratio)
{
    return align_pairs(c, n_pairs, pairs, k, match, mismatch, gap_extend, AlnOut{out_score, out_windows, out_ratio}, AlnRoute::normal);
}

}  // extern "C"

// what the entry points of ioc_align_sinks.cpp call
int ioc_align_pairs_sink(ioc_ctx* c, int32_t n_pairs, const ioc_aln_pair* pairs, int32_t k, int32_t match, int32_t mismatch, int32_t gap_extend,
                         int32_t* out_score, int64_t* out_windows, double* out_ratio, const AlnSink* sink)
{
    return align_pairs(c, n_pairs, pairs, k, match, mismatch, gap_extend, AlnOut{out_score, out_windows, out_ratio, sink}, AlnRoute::normal);
}

extern "C" {

// (ioc_ctx_prewarm)
hipError_t iock_warm_align()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(k_fwd2_ends));
}

}  // extern "C"
