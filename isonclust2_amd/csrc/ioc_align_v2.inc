// ioc_align_v2.inc — version 2 of the two-pass aligner (included by ioc_align_gpu.hip inside its anonymous namespace).
//
// What changed against k_align_fwd / k_align_trace (same recurrence, same results bit for bit):
//
//  * TWO PAIRS PER WAVE.  Every register of the forward pass holds two 16-bit scores: the low half belongs to pair A, the
//    high half to pair B of a COUPLE (two pairs of similar size), both at the same (row, column) of their own matrices.
//    v_pk_add_i16 / v_pk_max_i16 issue at the rate of their 32-bit cousins, so a cell costs 3.5 instead of 5 VALU.  16 bits
//    hold a score relative to a wave-uniform base per half that follows the sweep (rebased every 16 steps, guarded: a pair
//    that leaves the window is flagged and goes to the 32-bit kernel).
//  * DATAFLOW SCHEDULING instead of generations of equal workgroups.  The (band, strip) tiles of all couples form ONE list,
//    ordered by anti-diagonal; persistent waves take the next tile off an atomic counter, wait (bounded) for the flags of the
//    tile above and the tile to the left, compute, publish their flag.  A tile only ever waits for tiles earlier in the
//    list, which running waves hold: no residency assumption, no barrier, no tail generation.
//  * COARSE CHECKPOINTS ONLY: (Hq, F*) of every 512th row and (Hq, E*) of every 512th column, as the registers hold them
//    (one word = both pairs) plus the bases: 4.4 MB per 16.7 kb pair instead of 35 MB (config 3: 7 GB instead of 56 GB),
//    and the store blocks run in a quarter of the steps.  The traceback recomputes the 128-pitch checkpoints of a
//    512 x 512 block when its walk enters it (about (n + m) / 512 x 2 blocks per pair) into a per-wave scratch, then
//    goes on as before.
//
//  * A CERTIFIED CORRIDOR (round 4).  Only the tiles around the diagonal are computed; the result is vouched for per pair by a
//    bound on what a path through a skipped cell can score, a probe launch over the first tile tells the pairs that will not pass
//    (V2Couple, k_fwd2_probe, k_fwd2_ends); a refuted pair runs again with every tile.  Results never depend on it.
//  * The wrong candidates' walks run beside the others' (k_fwd2_ends routes them by their score to k_trace2_help on a side stream),
//    a launch with few couples lets a tile follow its left neighbour row by row (v2_wait_rows).
//  * LINKS: a wave goes on from a tile into the tile below it, skew and registers as they are, where that takes no wait
//    (v2_fwd_body; IOC_ALIGN_V2_LINK=0: never).
//
// Slanted scores, Hq = H* - (go - ge), the profile in LDS, the look-ahead ring, the 4-row steps and the lane skew are
// those of k_align_fwd (see there).

constexpr int V2_BLK_C = 8;       // columns per lane in the traceback's block recompute (64 x 8 = CK2)
static_assert(CK2 == 64 * V2_BLK_C, "block geometry");

// bounded wait for a flag another workgroup sets: relaxed agent-scope polls, then ONE acquire by the wave (the caller's).
// Wave-uniform on purpose — every lane polls the same word (one request) and the loop condition is a scalar: with the poll
// inside `if (lane == 0)` the compiler built the surrounding persistent loop as a lane-divergent one (exit masks derived from
// the lane test), and a build of this kernel never left its last tile.
__device__ __forceinline__ bool v2_wait(const uint32_t* flag, uint32_t* err)
{
    uint32_t seen = 0;
    for (uint32_t it = 0; it < (1u << 22); ++it) {
        seen = uint32_t(__builtin_amdgcn_readfirstlane(int(__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))));
        if (seen) break;
        if ((it & 255u) == 255u && __builtin_amdgcn_readfirstlane(int(__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))) break;  // somebody gave up
        __builtin_amdgcn_s_sleep(8);
    }
    if (!seen) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (every lane the same word, the same value)
    return seen != 0;
}

// A launch with few couples (a second alignment round, a merge's representatives) is bound by the critical path of ONE tile grid:
// there a tile does not wait for the tile on its left to be DONE but for the rows of its right edge it is about to read
// (`prog`: 4-row blocks of that edge that are written, published every 16 steps; the tile's flag once it is done).  Wave-uniform,
// bounded like v2_wait.
__device__ __forceinline__ bool v2_wait_rows(const uint32_t* prog, const uint32_t* flag, uint32_t need, uint32_t* err, uint32_t& avail)
{
    bool ok = false;
    for (uint32_t it = 0; it < (1u << 22); ++it) {
        const uint32_t f = uint32_t(__builtin_amdgcn_readfirstlane(int(__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))));
        const uint32_t g = uint32_t(__builtin_amdgcn_readfirstlane(int(__hip_atomic_load(prog, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))));
        if (f || g >= need) {
            ok = true;
            avail = f ? 0xFFFFFFFFu : g;  // (what is known to be out: a later fetch below it needs neither a poll nor an acquire)
            break;
        }
        if ((it & 255u) == 255u && __builtin_amdgcn_readfirstlane(int(__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))) break;  // somebody gave up
        __builtin_amdgcn_s_sleep(4);
    }
    if (!ok) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return ok;
}

// the next tile off the queue: ONE returning atomic by lane 0, without a branch the compiler could see (EXEC is narrowed
// and restored inside the statement)
__device__ __forceinline__ uint32_t v2_dequeue(uint32_t* queue)
{
    uint32_t x = 0, one = 1;
    unsigned long long save;
    asm volatile(
        "s_mov_b64 %1, exec\n\t"
        "s_mov_b64 exec, 1\n\t"
        "global_atomic_add %0, %2, %3, off sc0\n\t"
        "s_waitcnt vmcnt(0)\n\t"
        "s_mov_b64 exec, %1"
        : "+v"(x), "=&s"(save)
        : "v"(queue), "v"(one)
        : "memory");
    return uint32_t(__builtin_amdgcn_readfirstlane(int(x)));
}

// ---- 16-bit halves of version 2: UNSIGNED, biased --------------------------------------------------------------------
// A half holds (score - base) + 32768 as a u16 (the bias lives inside `base`: score = half + base).  With every live value
// between 4768 and 60768 (the guard) a 32-bit add of two small increments or a 32-bit subtraction of the two gap penalties
// never carries from the low half into the high one, so the two plain ops of a cell are v_add_u32 / v_sub_u32 (3 cycles to
// issue) instead of their packed cousins (4.3); the four maxima stay v_pk_max_u16.  "No score" is 0: it only ever enters a
// max, and the rebase subtracts with saturation.
typedef unsigned short v2u __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2u as_v2u(uint32_t x) { return __builtin_bit_cast(v2u, x); }
__device__ __forceinline__ uint32_t u32_of(v2u x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ uint32_t umax2(uint32_t a, uint32_t b) { return u32_of(__builtin_elementwise_max(as_v2u(a), as_v2u(b))); }
__device__ __forceinline__ uint32_t umin2(uint32_t a, uint32_t b) { return u32_of(__builtin_elementwise_min(as_v2u(a), as_v2u(b))); }
__device__ __forceinline__ uint32_t usubs2(uint32_t a, uint32_t b) { return u32_of(__builtin_elementwise_sub_sat(as_v2u(a), as_v2u(b))); }
__device__ __forceinline__ uint32_t clampu16(int v) { return uint32_t(min(max(v, 0), 65535)); }
__device__ __forceinline__ uint32_t packu(uint32_t lo, uint32_t hi) { return lo | (hi << 16); }
__device__ __forceinline__ int v2_half(uint32_t w, int h) { return h ? int(w >> 16) : int(w & 0xFFFFu); }
constexpr int U16_BIAS = 32768;

// one row of 16 columns, both halves: 7 VALU per column pair — byte pair of the two profiles (v_perm_b32), diagonal + increment
// (v_add_u32), F* / T / E* / H* maxima (4 x v_pk_max_u16), Hq = H* - gd (v_sub_u32).  Everything that does not hang on the left
// neighbour is computed for the 16 columns first; the chain along the row is E* = max(E*, Hq), H* = max(T, E*), Hq = H* - gd.
// (Written column by column, with the next row's profile words prefetched, the scheduler pulled so much ahead that 70 registers
// spilled: 77 ms instead of 75.)
__device__ __forceinline__ void cells_u16(uint32_t (&Hq)[FW_C], uint32_t (&F)[FW_C], const uint4& xa, const uint4& xb, uint32_t& hql, uint32_t& el,
                                          uint32_t dgq, uint32_t gd2)
{
    const uint32_t xl[FW_C / 4] = {xa.x, xa.y, xa.z, xa.w}, xh[FW_C / 4] = {xb.x, xb.y, xb.z, xb.w};
    uint32_t T[FW_C];
#pragma unroll
    for (int c = 0; c < FW_C; ++c) {
        const uint32_t Fn = umax2(F[c], Hq[c]);
        const uint32_t sel = 0x0c000c00u | uint32_t(4 + (c & 3)) << 16 | uint32_t(c & 3);  // bytes (c & 3) of xl and xh, zero-extended into the halves
        const uint32_t inc = __builtin_amdgcn_perm(xh[c >> 2], xl[c >> 2], sel);
        T[c] = umax2((c ? Hq[c - 1] : dgq) + inc, Fn);
        F[c] = Fn;
    }
    uint32_t e = el, h = hql;
#pragma unroll
    for (int c = 0; c < FW_C; ++c) {
        e = umax2(e, h);
        h = umax2(T[c], e) - gd2;
        Hq[c] = h;
    }
    hql = h;
    el = e;
}

// a tile parameter out of the wave's LDS vector: ONE ds_read_b32 at a uniform address (a volatile C++ read of LDS compiles to
// a flat load with system scope; an ordinary one lets the compiler keep all of them in scalar registers again)
__device__ __forceinline__ uint32_t v2_par(uint32_t lds_byte_addr)
{
    uint32_t x;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(x) : "v"(lds_byte_addr) : "memory");
    return x;
}

__device__ __forceinline__ void v2_lds_store(uint32_t lds_byte_addr, uint32_t v)
{
    asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : : "v"(lds_byte_addr), "v"(v) : "memory");
}

// Parameters of the current tile that only the rare blocks need (the special rows, the checkpoint stores, the fetch of the
// left edge every 16 steps, the end of the tile) live in a wave-private LDS vector instead of ~45 scalar registers: the
// kernel had 110 - 124 SGPRs spilled into VGPR lanes around every branch.  A read is one ds_read_b32 at a uniform address.
enum V2Par : uint32_t {
    VP_N0 = 0, VP_N1, VP_M0, VP_M1, VP_GD0, VP_GD1, VP_LROW0, VP_LROW1, VP_BEST0, VP_BEST1, VP_PID0, VP_PID1,
    VP_RDAT_LO, VP_RDAT_HI, VP_RBASE_LO, VP_RBASE_HI, VP_CDAT_LO, VP_CDAT_HI, VP_CBASE_LO, VP_CBASE_HI,
    VP_MPAD, VP_NQ, VP_FLAG, VP_BAND, VP_STRIP, VP_COLIN_LO, VP_COLIN_HI, VP_RHI0, VP_RHI1,
    VP_COUPLE, VP_FLAG_PREV, VP_BND_PREV,  // (links: the couple's number; the flag and the first row block of the band a run has just left)
    VP_COUNT = 32
};

// The query profiles of every (couple, strip), made ONCE per batch: per pair, base code and lane the score increments of the lane's
// 16 columns as bytes (match / mismatch + 2 ge + gd, see cells_u16).  A tile reads its 10 KB with ten 16-byte loads per lane;
// building them in the tile cost ~500 instructions per tile start.  (Left behind by round 4's chained-strips experiment,
// profiles/r04_fwd_chain.txt.)
__global__ void __launch_bounds__(128)
k_fwd2_prof(const AlnPairDev* __restrict__ pairs, const V2Couple* __restrict__ couples, const uint8_t* __restrict__ pool, AlnParams P, uint4* __restrict__ prof)
{
    const V2Couple& cp = couples[blockIdx.x];
    const uint32_t p = blockIdx.y;
    if (p >= cp.nstrips) return;
    const uint32_t h = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const bool have = cp.pid[h] != 0xFFFFFFFFu;
    const AlnPairDev pr = pairs[have ? cp.pid[h] : cp.pid[0]];
    const uint32_t m = have ? pr.m : 0u;
    const uint8_t* r = pool + pr.r_off;
    const int ge = P.gap_extend, gd = pr.gap_open - ge;
    const int cm = P.match + 2 * ge + gd, cx = P.mismatch + 2 * ge + gd;
    const uint32_t jb = p * (64u * FW_C) + lane * FW_C;
    uint32_t rpk[FW_C / 4];
#pragma unroll
    for (int c4 = 0; c4 < FW_C / 4; ++c4) {
        uint32_t w = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) w |= (have ? ref_byte(r, m, pr.rc, jb + c4 * 4 + e) : 0u) << (8 * e);
        rpk[c4] = w;
    }
    const uint32_t bases = 'A' | ('C' << 8) | ('G' << 16) | ('T' << 24);
    uint4* out = prof + cp.prof + (uint64_t(p) * 2u + h) * 5u * 64u + lane;
#pragma unroll
    for (int code = 0; code < 5; ++code) {
        const uint32_t b = code < 4 ? (bases >> (8 * code)) & 0xFFu : 0x100u;  // 0x100: equals no byte
        uint32_t w4[FW_C / 4];
#pragma unroll
        for (int c4 = 0; c4 < FW_C / 4; ++c4) {
            uint32_t w = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) w |= uint32_t(((rpk[c4] >> (8 * e)) & 0xFFu) == b ? cm : cx) << (8 * e);
            w4[c4] = w;
        }
        out[uint32_t(code) * 64u] = uint4{w4[0], w4[1], w4[2], w4[3]};
    }
}

// A slice's list of tiles, written where the launches read it (tile_lists in ioc_align_gpu.hip is the definition of its order and
// the host's version of it; IOC_V2_ITEMS_CHECK compares the two): first the probe's tiles — of a couple with a corridor the grid
// of bands 0 .. probe_band by strips 0 .. probe_strip —, then every couple's full grid, each part anti-diagonal by anti-diagonal,
// couples side by side, bands ascending.  The list is a function of the grids alone; it takes a quarter of a million items and
// their upload off the host for every call.
// One workgroup per (anti-diagonal, part).  Where its anti-diagonal starts in the list: the tiles of every couple on the
// anti-diagonals before it, min(strips, dg - band) per band; where a couple's tiles start within it: a scan over the couples.
constexpr int V2_ITEMS_T = 256;
__global__ void __launch_bounds__(V2_ITEMS_T)
k_fwd2_items(const V2Couple* __restrict__ couples, uint32_t k_first, uint32_t n_couples, uint32_t n_probe, V2Item* __restrict__ items, uint32_t n_items)
{
    __shared__ uint32_t s_scan[V2_ITEMS_T];
    const uint32_t dg = blockIdx.x, tid = threadIdx.x;
    const bool probe = blockIdx.y == 0;
    auto grid = [&](uint32_t x, uint32_t& nb, uint32_t& ns) {
        const V2Couple& cp = couples[k_first + x];
        if (probe) {
            nb = cp.corridor ? uint32_t(cp.probe_band) + 1u : 0u;
            ns = uint32_t(cp.probe_strip) + 1u;
        } else {
            nb = cp.nbands;
            ns = cp.nstrips;
        }
    };
    uint32_t before = 0;
    for (uint32_t x = tid; x < n_couples; x += V2_ITEMS_T) {
        uint32_t nb, ns;
        grid(x, nb, ns);
        for (uint32_t b = 0; b < nb && b < dg; ++b) before += min(ns, dg - b);
    }
    s_scan[tid] = before;
    __syncthreads();
    for (uint32_t d = V2_ITEMS_T / 2; d; d >>= 1) {
        if (tid < d) s_scan[tid] += s_scan[tid + d];
        __syncthreads();
    }
    uint32_t running = s_scan[0] + (probe ? 0u : n_probe);
    __syncthreads();
    for (uint32_t x0 = 0; x0 < n_couples; x0 += V2_ITEMS_T) {
        const uint32_t x = x0 + tid;
        uint32_t cnt = 0, b_lo = 0;
        if (x < n_couples) {
            uint32_t nb, ns;
            grid(x, nb, ns);
            if (nb && dg <= nb + ns - 2u) {
                b_lo = dg >= ns ? dg - ns + 1u : 0u;
                cnt = min(dg, nb - 1u) - b_lo + 1u;
            }
        }
        s_scan[tid] = cnt;
        __syncthreads();
        for (uint32_t d = 1; d < V2_ITEMS_T; d <<= 1) {  // (inclusive scan)
            const uint32_t v = tid >= d ? s_scan[tid - d] : 0u;
            __syncthreads();
            s_scan[tid] += v;
            __syncthreads();
        }
        const uint32_t pos = running + s_scan[tid] - cnt;
        for (uint32_t i = 0; i < cnt; ++i)
            if (pos + i < n_items) items[pos + i] = V2Item{k_first + x, uint16_t(b_lo + i), uint16_t(dg - (b_lo + i))};
        running += s_scan[V2_ITEMS_T - 1];
        __syncthreads();
    }
}

// (the body of k_fwd2 and of k_fwd2_w2: the same code compiled for three waves per SIMD and 168 registers, or for two and no spills)
static __device__ __forceinline__ void
v2_fwd_body(const AlnPairDev* __restrict__ pairs, const V2Couple* __restrict__ couples, const V2Item* __restrict__ items, uint32_t n_items,
       uint32_t* __restrict__ queue, uint32_t* __restrict__ flags, uint32_t* __restrict__ err, const uint8_t* __restrict__ pool, AlnParams P,
       uint32_t* __restrict__ arena, int2* __restrict__ lrow, int2* __restrict__ bandbest, uint32_t* __restrict__ ovf_out, int guard,
       const uint4* __restrict__ prof, unsigned long long* __restrict__ cells_done, uint32_t* __restrict__ prog, uint32_t prog_every,
       uint32_t* __restrict__ claims, uint32_t link_mode)
{
    // LINKS (claims != nullptr).  A wave that is about to finish tile (b, p) goes on into (b + 1, p) with its lanes' skew and registers
    // as they are — the run is one tall tile, and the 63 steps of pipeline fill of (b + 1, p) are never issued — whenever that
    // needs NO WAIT: the tile has no left side (strip 0, or the leftmost strip of its band's corridor), or its left neighbour's
    // flag reads done at the moment of the decision.  (The general case does not fit: the list orders tiles by anti-diagonal, so
    // the left neighbour (b + 1, p - 1) was dequeued together with (b, p) and ends together with it — following it takes a wait
    // row by row.)  A tile is owned by whoever adds to its CLAIM word first — the wave that dequeued it, once its waits are over,
    // or the wave that runs into it —, the other leaves it alone.  The decision falls 32 steps before lane 0 leaves the band: from there the look-ahead
    // ring fetches the next band's left edge and query codes.  Everything per band switches there for the wave (rows of either
    // pair, last_band, the left edge, the flag, nsteps) or, where lanes of both bands are in flight, per lane by its row block
    // (`bnd`: the run-relative row block the newest band starts at): the best of the last column, the tile's publication
    // (once the last lane has left it: step bnd + 64) and the rows of its right edge that are out.  A run goes on while either
    // pair has rows further down; the half of a pair that has none is put back to the bias once per band (finish_prev).
    // link_mode 2 (the probe launch): only inside the probe's grid — a tile beyond it may get a wider corridor from k_fwd2_probe.
    uint32_t* const link_stats = queue + 4;  // tiles computed, links without a left side, links with the left tile done
    constexpr uint32_t NEVER = 0xFFFFFFFFu;
    __shared__ __attribute__((aligned(16))) uint32_t s_look_all[V2_WAVES][3][128];
    __shared__ __attribute__((aligned(16))) uint32_t s_prof_all[V2_WAVES][2][5][64][4];  // [wave][pair][base code][lane][4 words]
    __shared__ uint32_t s_par_all[V2_WAVES][VP_COUNT];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    uint32_t(*s_look)[128] = s_look_all[wv];
    uint32_t* s_par = s_par_all[wv];
    const uint32_t par_addr = uint32_t(reinterpret_cast<uintptr_t>(s_par));  // LDS byte address of the vector
    auto par = [&](uint32_t k) -> uint32_t { return v2_par(par_addr + 4u * k); };
    auto par64 = [&](uint32_t k) -> uint64_t { return uint64_t(par(k)) | (uint64_t(par(k + 1u)) << 32); };
    constexpr uint32_t strip_cols = 64u * FW_C;
    const int ge = P.gap_extend;
    auto qcode = [](uint32_t ch) -> uint32_t {  // byte offset of a query base's profile row
        const uint32_t code = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
        return code * 1024u;
    };
    uint32_t it = v2_dequeue(queue);
    while (it < n_items) {
        uint32_t band, p, r_lo, nblk[2];
        bool vh[2], last_band[2];
        bool left_ok = true;  // (corridor: the tile to the left is computed, or this is strip 0)
        bool top_none = false;  // (corridor: nothing above this tile — the lanes' top row is "no score")
        bool left_rows = false;  // (few couples: the tile to the left is waited for row by row, v2_wait_rows)
        uint32_t left_idx = 0, nblk_band = 0, left_avail = 0;
        uint32_t bnd = 0;           // (links) the row block of the run at which its newest band starts
        uint32_t link_at = NEVER;   // (links) the step at which the run decides about the next band
        const uint8_t* q[2];
        int base[2];
        uint32_t gd2;
        uint32_t Hp[FW_C], F[FW_C];
        uint32_t dg;
        uint64_t cb_off = 0;       // ... and of their bases
        uint64_t co_off = 0;       // (lanes 31 / 63) word offset of this lane's coarse-column entries of the band's first row block
        uint64_t rd_off = 0;       // word offset of this lane's 16 columns in coarse row 0 of the couple (Hq plane)
        uint64_t rb_off = 0;       // ... and of its int2 of bases
        uint32_t mpad = 0, ncr = 0;  // row pitch, coarse rows the couple stores
        {   // ---- tile setup: everything of the couple that is needed once, or rarely, stays inside this block or goes to s_par ----
            const V2Item item = items[it];
            const V2Couple cp = couples[item.couple];
            band = item.band;
            p = item.strip;
            // (corridor: a tile outside its couple's corridor is not computed; a tile the probe launch did is done)
            // (links: ... and a tile a run went on into, or is about to, is that run's)
            if (p < cp.plo[band] || p > cp.phi[band] ||
                __builtin_amdgcn_readfirstlane(int(__hip_atomic_load(&flags[cp.flag0 + band * cp.nstrips + p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) != 0 ||
                (claims != nullptr &&
                 __builtin_amdgcn_readfirstlane(int(__hip_atomic_load(&claims[cp.flag0 + band * cp.nstrips + p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) != 0)) {
                it = v2_dequeue(queue);
                continue;
            }
            // the tile above and the tile to the left have published their checkpoints?  (a wait that ran out flags the launch: the
            // host runs the batch again the old way; the tile still runs, on whatever is there, so that nobody behind it waits for ever)
            // (corridor: a neighbour that is not computed is neither waited for nor read — its side of the tile is "no score")
            const bool top_in = band > 0 && p >= cp.plo[band - 1u] && p <= cp.phi[band - 1u];
            const bool left_in = p > cp.plo[band];
            left_ok = p == 0 || left_in;
            top_none = band > 0 && !top_in;
            const bool corner_in = band > 0 && p > 0 && p - 1u >= cp.plo[band - 1u] && p - 1u <= cp.phi[band - 1u];
            if (top_in) (void)v2_wait(&flags[cp.flag0 + (band - 1u) * cp.nstrips + p], err);
            left_rows = prog != nullptr && left_in;
            left_idx = cp.flag0 + band * cp.nstrips + (p - 1u);
            {   // (row blocks of the band: the larger pair's)
                const uint32_t rows_b = min(max(cp.pid[0] != 0xFFFFFFFFu ? pairs[cp.pid[0]].n : 0u, cp.pid[1] != 0xFFFFFFFFu ? pairs[cp.pid[1]].n : 0u),
                                            uint32_t(cp.bstart[band + 1u]) * uint32_t(CK2));
                const uint32_t r0_b = uint32_t(cp.bstart[band]) * uint32_t(CK2);
                nblk_band = rows_b > r0_b ? (rows_b - r0_b + FW_R - 1) / FW_R : 0u;
            }
            if (left_in && !left_rows) (void)v2_wait(&flags[left_idx], err);
            if (left_rows) (void)v2_wait_rows(&prog[left_idx], &flags[left_idx], min(32u, nblk_band), err, left_avail);  // (the first two fetches: 128 rows)
            // (links: the tile is this wave's only if it is the first to claim it — the wave that ran the tile above may have gone
            // on into it while this one waited.  Claimed AFTER the waits: a wave that merely waits on a tile does not keep a run out of it.)
            if (claims != nullptr && v2_dequeue(&claims[left_idx + 1u]) != 0u) {
                it = v2_dequeue(queue);
                continue;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            r_lo = uint32_t(cp.bstart[band]) * uint32_t(CK2);  // (both pairs: bands start on the same coarse rows)
            const uint32_t jb = p * strip_cols + lane * FW_C;
            uint32_t n[2], m[2], r_hi[2];
            int gd[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const bool have = cp.pid[h] != 0xFFFFFFFFu;
                const AlnPairDev pr = pairs[have ? cp.pid[h] : cp.pid[0]];
                n[h] = have ? pr.n : 0u;
                m[h] = have ? pr.m : 0u;
                q[h] = pool + pr.q_off;
                gd[h] = pr.gap_open - ge;
                r_hi[h] = min(n[h], uint32_t(cp.bstart[band + 1u]) * uint32_t(CK2));
                nblk[h] = r_hi[h] > r_lo ? (r_hi[h] - r_lo + FW_R - 1) / FW_R : 0u;
                const uint32_t nstr = (m[h] + strip_cols - 1) / strip_cols;
                vh[h] = have && p < nstr && nblk[h] > 0;
                last_band[h] = vh[h] && r_hi[h] == n[h];
            }
            gd2 = packu(uint32_t(gd[0]), uint32_t(gd[1]));
            // (links: a band further down with rows of a pair that has columns here — then this band is whole: a multiple of 128 row blocks)
            if (claims != nullptr && band + 1u < cp.nbands && nblk_band >= 128u &&
                max(vh[0] ? n[0] : 0u, vh[1] ? n[1] : 0u) > uint32_t(cp.bstart[band + 1u]) * uint32_t(CK2))
                link_at = nblk_band - 32u;
            mpad = cp.mpad;
            rd_off = cp.rdat + jb;
            rb_off = cp.rbase + uint64_t(jb / 16u) * 2u;
            {
                uint32_t nmx = max(n[0], n[1]);
                ncr = nmx ? (nmx - 1u) / uint32_t(CK2) : 0u;
            }
            {
                const uint64_t e0 = uint64_t((jb + FW_C) / CK2 - ((jb + FW_C) >= uint32_t(CK2) ? 1u : 0u)) * cp.nq + r_lo / 4u;  // (only lanes 31 / 63 use it)
                co_off = cp.cdat + e0 * 8u;
                cb_off = cp.cbase + e0 * 2u;
            }
            const uint64_t colin = p ? uint64_t(p * (strip_cols / CK2) - 1u) * cp.nq : 0;
            // (the LDS of this wave may still be read by its own previous tile's last instructions: program order is enough)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) {
                s_par[VP_N0] = n[0];
                s_par[VP_N1] = n[1];
                s_par[VP_M0] = m[0];
                s_par[VP_M1] = m[1];
                s_par[VP_GD0] = uint32_t(gd[0]);
                s_par[VP_GD1] = uint32_t(gd[1]);
                s_par[VP_LROW0] = cp.lrow0[0];
                s_par[VP_LROW1] = cp.lrow0[1];
                s_par[VP_BEST0] = cp.best0[0];
                s_par[VP_BEST1] = cp.best0[1];
                s_par[VP_PID0] = cp.pid[0];
                s_par[VP_PID1] = cp.pid[1];
                s_par[VP_RDAT_LO] = uint32_t(cp.rdat);
                s_par[VP_RDAT_HI] = uint32_t(cp.rdat >> 32);
                s_par[VP_RBASE_LO] = uint32_t(cp.rbase);
                s_par[VP_RBASE_HI] = uint32_t(cp.rbase >> 32);
                s_par[VP_CDAT_LO] = uint32_t(cp.cdat);
                s_par[VP_CDAT_HI] = uint32_t(cp.cdat >> 32);
                s_par[VP_CBASE_LO] = uint32_t(cp.cbase);
                s_par[VP_CBASE_HI] = uint32_t(cp.cbase >> 32);
                s_par[VP_MPAD] = cp.mpad;
                s_par[VP_NQ] = cp.nq;
                s_par[VP_FLAG] = cp.flag0 + band * cp.nstrips + p;
                s_par[VP_BAND] = band;
                s_par[VP_STRIP] = p;
                s_par[VP_COLIN_LO] = uint32_t(colin);
                s_par[VP_COLIN_HI] = uint32_t(colin >> 32);
                s_par[VP_RHI0] = r_hi[0];
                s_par[VP_RHI1] = r_hi[1];
                s_par[VP_COUPLE] = item.couple;
                s_par[VP_FLAG_PREV] = 0;
                s_par[VP_BND_PREV] = 0;
            }
            // ---- top edge: row 0 of the matrices, or the coarse row the band above wrote ----
            int Ha[2][FW_C], Fa[2][FW_C], dga[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (!vh[h]) {
#pragma unroll
                    for (int c = 0; c < FW_C; ++c) Ha[h][c] = Fa[h][c] = 0;
                    dga[h] = 0;
                } else if (r_lo > 0 && !top_in) {  // (corridor: nothing above)
#pragma unroll
                    for (int c = 0; c < FW_C; ++c) Ha[h][c] = Fa[h][c] = ALN_NEG;
                    dga[h] = ALN_NEG;
                } else if (r_lo == 0) {
                    const int b0 = ge * int(jb) - gd[h];
#pragma unroll
                    for (int c = 0; c < FW_C; ++c) {
                        Ha[h][c] = b0 + ge * (c + 1);
                        Fa[h][c] = ALN_NEG;
                    }
                    dga[h] = b0;
                } else {
                    const uint32_t ckr = r_lo / CK2 - 1u;
                    const uint32_t* rh = arena + cp.rdat + uint64_t(2u * ckr) * cp.mpad;
                    const uint32_t* rf = rh + cp.mpad;
                    const int2* rb = reinterpret_cast<const int2*>(arena + cp.rbase) + uint64_t(ckr) * (cp.mpad / 16u);
                    const int2 bb = jb < cp.mpad ? rb[jb / 16u] : int2{0, 0};
                    const int bs = h ? bb.y : bb.x;
#pragma unroll
                    for (int c = 0; c < FW_C; ++c) {
                        int2 v{0, 0};
                        if (jb + c < m[h]) v = int2{v2_half(rh[jb + c], h) + bs, v2_half(rf[jb + c], h) + bs};
                        Ha[h][c] = v.x;
                        Fa[h][c] = v.y;
                    }
                    if (lane == 0 && p > 0 && !corner_in) {
                        dga[h] = ALN_NEG;  // (corridor: the tile above and to the left is not computed)
                    } else if (jb > 0 && jb <= m[h]) {
                        const int2 bl = rb[(jb - 1u) / 16u];
                        dga[h] = v2_half(rh[jb - 1u], h) + (h ? bl.y : bl.x);
                    } else {
                        dga[h] = ge * int(r_lo) - gd[h];  // column 0 holds H = 0
                    }
                }
                if (vh[h] && r_lo > 0 && !top_in) {
                    // (corridor, nothing above: the scores enter from the left — the first row's entry of the coarse column the tile
                    // to the left wrote sits at the bias)
                    const uint64_t e = colin + r_lo / 4u;
                    const uint32_t* d = arena + cp.cdat + e * 8u;
                    const int2 bb = reinterpret_cast<const int2*>(arena + cp.cbase)[e];
                    base[h] = v2_half(d[0], h) + (h ? bb.y : bb.x) - U16_BIAS;
                } else
                base[h] = __builtin_amdgcn_readfirstlane(Ha[h][0]) - U16_BIAS;  // lane 0, first column of the strip, sits at the bias
            }
#pragma unroll
            for (int c = 0; c < FW_C; ++c) {
                const bool in0 = vh[0] && jb + c < m[0], in1 = vh[1] && jb + c < m[1];
                // (columns right of the matrix: the bias, they only ever follow their left neighbours)
                Hp[c] = packu(in0 ? clampu16(Ha[0][c] - base[0]) : uint32_t(U16_BIAS), in1 ? clampu16(Ha[1][c] - base[1]) : uint32_t(U16_BIAS));
                F[c] = packu(in0 ? clampu16(Fa[0][c] - base[0]) : uint32_t(U16_BIAS), in1 ? clampu16(Fa[1][c] - base[1]) : uint32_t(U16_BIAS));
            }
            dg = packu(clampu16(dga[0] - base[0]), clampu16(dga[1] - base[1]));
            // ---- query profiles of the strip, one per pair: out of the batch's profile arena (k_fwd2_prof) ----
            {
                const uint4* pp = prof + cp.prof + uint64_t(p) * (2u * 5u * 64u) + lane;
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int code = 0; code < 5; ++code) {
                        const uint4 w = pp[(uint32_t(h) * 5u + uint32_t(code)) * 64u];
                        *reinterpret_cast<uint4*>(&s_prof_all[wv][h][code][lane][0]) = w;
                    }
            }
        }
        // ---- per-lane facts of the tile (VGPRs) ----
        const uint32_t jb = p * strip_cols + lane * FW_C;
        uint32_t nsteps = max(nblk[0], nblk[1]) + 63u;  // (links: grows with every band the run goes on into)
        uint32_t lanef = 0;  // bit h: has columns of pair h; bit 2 + h: owns the last column of pair h; bit 4: stores a coarse column
        int lastc[2];
        uint32_t ncl[2];
        bool strip_has_lastc = false;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        {
            const uint32_t jr = jb + FW_C;
            bool any_right = false;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t mh = par(VP_M0 + h);
                const bool hc = vh[h] && jb < mh;
                ncl[h] = vh[h] ? min(64u, (mh - p * strip_cols + FW_C - 1) / FW_C) : 0u;
                lastc[h] = (vh[h] && mh - 1 >= jb && mh - 1 < jb + FW_C) ? int(mh - 1 - jb) : -1;
                strip_has_lastc = strip_has_lastc || (vh[h] && uint64_t(p + 1u) * strip_cols >= mh);
                any_right = any_right || (vh[h] && jr < mh);
                lanef |= (hc ? 1u : 0u) << h;
                lanef |= (lastc[h] >= 0 ? 4u : 0u) << h;
            }
            if ((jr % CK2) == 0 && any_right) lanef |= 16u;  // lanes 31 and 63: the right edge is a coarse column with columns of some pair to its right
        }
        const uint8_t* profA = reinterpret_cast<const uint8_t*>(&s_prof_all[wv][0][0][lane][0]);
        const uint8_t* profB = reinterpret_cast<const uint8_t*>(&s_prof_all[wv][1][0][lane][0]);
        // left edge of the strip, absolute and slanted: column 0 of the matrices or the coarse column the tile to the left wrote
        auto left_edge = [&](int h, uint32_t row) {
            int2 v{ge * int(row + 1) - int(par(VP_GD0 + h)), ALN_NEG};
            if (!left_ok) v = int2{ALN_NEG, ALN_NEG};
            else if (vh[h] && p > 0 && row < par(VP_RHI0 + h)) {
                const uint64_t e = par64(VP_COLIN_LO) + row / 4u;
                const uint32_t* d = arena + par64(VP_CDAT_LO) + e * 8u;
                const int2 bb = reinterpret_cast<const int2*>(arena + par64(VP_CBASE_LO))[e];
                const int bs = h ? bb.y : bb.x;
                v = int2{v2_half(d[row & 3u], h) + bs, v2_half(d[4u + (row & 3u)], h) + bs};
            }
            return v;
        };
        uint32_t qn = 0;
        int2 en[2] = {{0, 0}, {0, 0}};
        uint32_t hl[FW_R], el[FW_R];
        uint32_t qc[FW_R];
#pragma unroll
        for (int rr = 0; rr < FW_R; ++rr) {
            hl[rr] = packu(U16_BIAS, U16_BIAS);
            el[rr] = 0;
            qc[rr] = 0;
        }
        auto publish = [&](uint32_t blk) {  // relative to the bases of NOW (the rebase keeps the ring current)
            s_look[0][(blk & 1u) * 64u + lane] = packu(clampu16(en[0].x - base[0]), clampu16(en[1].x - base[1]));
            s_look[1][(blk & 1u) * 64u + lane] = packu(clampu16(en[0].y - base[0]), clampu16(en[1].y - base[1]));
            s_look[2][(blk & 1u) * 64u + lane] = qn;
        };
        auto fetch = [&](uint32_t blk) {
            const uint32_t row = r_lo + blk * 64u + lane;
            uint32_t qq[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                qq[h] = qcode((vh[h] && row < par(VP_RHI0 + h)) ? q[h][row] : 0u);
                en[h] = left_edge(h, row);
            }
            qn = qq[0] | (qq[1] << 16);
        };
        fetch(0);
        publish(0);
        fetch(1);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        uint4 nxh, nxe, nxq;
        nxh = *reinterpret_cast<const uint4*>(&s_look[0][0]);
        nxe = *reinterpret_cast<const uint4*>(&s_look[1][0]);
        nxq = *reinterpret_cast<const uint4*>(&s_look[2][0]);
        {   // (the query codes of a step are shifted in at the end of the step before: here for step 0)
            const uint32_t q4[FW_R] = {nxq.x, nxq.y, nxq.z, nxq.w};
#pragma unroll
            for (int rr = 0; rr < FW_R; ++rr) qc[rr] = from_left_or(qc[rr], q4[rr]);
        }
        int bc[2] = {ALN_NEG, ALN_NEG};  // best of the last column inside this band (true score), first row wins ties
        uint32_t bc_i[2] = {0, 0};
        uint32_t ovf = 0;

        // (links) the band the run has left is out: the best of the last column of a pair that ended in it (a pair that goes on
        // wrote its own when its lane crossed), every store of the wave, the release, the tile's flag — as at the end of a tile
        auto finish_prev = [&]() {
            const uint32_t bp = uint32_t(__builtin_amdgcn_readfirstlane(int(par(VP_BND_PREV))));
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (lastc[h] >= 0 && nblk[h] <= bnd && nblk[h] > bp) bandbest[par(VP_BEST0 + h) + band - 1u] = int2{bc[h], int(bc_i[h])};
            const uint32_t prev_flag = uint32_t(__builtin_amdgcn_readfirstlane(int(par(VP_FLAG_PREV))));
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(&flags[prev_flag], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // A half without rows in the newest band is idle in every lane by now.  It starts the band the way a tile of its own would:
            // at the bias.  (Nothing reads it; but it is not rebased with the live half, and left to itself down a long run the low
            // one could drift to the top of its 16 bits and carry into the high one.)
            uint32_t keep = 0xFFFFFFFFu, fill = 0u;
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (!vh[h] || nblk[h] <= bnd) {
                    keep &= ~(0xFFFFu << (16 * h));
                    fill |= uint32_t(U16_BIAS) << (16 * h);
                }
            if (keep != 0xFFFFFFFFu) {
#pragma unroll
                for (int c = 0; c < FW_C; ++c) {
                    Hp[c] = (Hp[c] & keep) | fill;
                    F[c] = (F[c] & keep) | fill;
                }
#pragma unroll
                for (int rr = 0; rr < FW_R; ++rr) {
                    hl[rr] = (hl[rr] & keep) | fill;
                    el[rr] &= keep;
                }
                dg = (dg & keep) | fill;
            }
        };
        // (links) the decision, wave-uniform, at step link_at = 32 steps before lane 0 leaves the band: no loop, no sleep, no wait
        auto link_decide = [&]() {
            const V2Couple* cq = couples + uint32_t(__builtin_amdgcn_readfirstlane(int(par(VP_COUPLE))));
            const uint32_t nb = band + 1u;  // (< nbands: link_at is only set then)
            const uint32_t lo = cq->plo[nb], hi = cq->phi[nb];
            const uint32_t fi = cq->flag0 + nb * cq->nstrips + p;
            bool go = p >= lo && p <= hi;
            if (link_mode == 2u) go = go && nb <= uint32_t(cq->probe_band) && p <= uint32_t(cq->probe_strip);
            uint32_t kind = 0;
            if (go) {
                if (p == 0u || p == lo) kind = 1u;
                else if (__builtin_amdgcn_readfirstlane(int(__hip_atomic_load(&flags[fi - 1u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) != 0) kind = 2u;
                go = kind != 0u && __builtin_amdgcn_readfirstlane(int(__hip_atomic_load(&flags[fi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) == 0 &&
                     v2_dequeue(&claims[fi]) == 0u;
            }
            link_at = NEVER;
            if (!go) return;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            const uint32_t bend = uint32_t(cq->bstart[nb + 1u]) * uint32_t(CK2);
            uint32_t nn[2], rh[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                nn[h] = uint32_t(__builtin_amdgcn_readfirstlane(int(par(VP_N0 + h))));
                rh[h] = min(nn[h], bend);
                if (vh[h]) {  // (a pair that ended higher up keeps its rows; one that never had any keeps none)
                    nblk[h] = (rh[h] - r_lo + FW_R - 1) / FW_R;
                    last_band[h] = rh[h] == nn[h];
                }
            }
            const uint32_t old_flag = par(VP_FLAG);
            v2_lds_store(par_addr + 4u * VP_FLAG_PREV, old_flag);
            v2_lds_store(par_addr + 4u * VP_BND_PREV, bnd);
            v2_lds_store(par_addr + 4u * VP_FLAG, fi);
            v2_lds_store(par_addr + 4u * VP_BAND, nb);
            v2_lds_store(par_addr + 4u * VP_RHI0, rh[0]);
            v2_lds_store(par_addr + 4u * VP_RHI1, rh[1]);
            bnd = nblk_band;
            nblk_band = (min(max(nn[0], nn[1]), bend) - r_lo + FW_R - 1) / FW_R;
            nsteps = max(nblk[0], nblk[1]) + 63u;
            band = nb;
            left_ok = p == 0u || p > lo;
            left_rows = false;  // (no left side, or a left tile that is done)
            if (nb + 1u < cq->nbands && max(vh[0] ? nn[0] : 0u, vh[1] ? nn[1] : 0u) > bend) link_at = nblk_band - 32u;
            (void)v2_dequeue(link_stats);  // (one more tile)
            (void)v2_dequeue(link_stats + kind);
        };

        // (first: the step may be the first of a group of 16 — rebase, publish, fetch; the loop below runs two steps per
        // iteration from an even number, so only the first of the two can be)
        auto step = [&](const uint32_t s, auto first) __attribute__((always_inline)) {
            if (decltype(first)::value && (s & (64 / FW_R - 1)) == 0) {
                if (s == link_at) link_decide();
                if (bnd != 0u && s == bnd + 64u) finish_prev();  // (lane 63 stored the last row block of the band above at step bnd + 62)
                if (s) {
                    // ---- rebase: advance each base by the first column of a lane that is inside its band ----
                    int dl[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const uint32_t lr = s + 1u > nblk[h] ? min(63u, s + 1u - nblk[h]) : 0u;
                        const int ref = __builtin_amdgcn_readlane(int(Hp[0]), int(lr));
                        dl[h] = max(v2_half(uint32_t(ref), h) - U16_BIAS, 0);
                        if (!vh[h] || lr >= ncl[h]) dl[h] = 0;
                        base[h] += dl[h];
                    }
                    const uint32_t d2 = packu(uint32_t(dl[0]), uint32_t(dl[1]));
                    {   // guard (lanes inside a band only: the registers of the others are idle)
                        uint32_t mx = Hp[0], mn = Hp[0];
#pragma unroll
                        for (int c = 1; c < FW_C; ++c) {
                            mx = umax2(mx, Hp[c]);
                            mn = umin2(mn, Hp[c]);
                        }
                        const int bi = int(s) - int(lane);
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int hi_v = v2_half(mx, h) - U16_BIAS, lo_v = v2_half(mn, h) - U16_BIAS;
                            // (a lane about to start under a missing top row still holds that row: "no score", not a score out of the window)
                            if ((lanef >> h & 1u) && bi >= (top_none ? 1 : 0) && uint32_t(bi) < nblk[h] && (hi_v > guard || lo_v < -guard)) {
#ifdef IOC_V2_GUARD_DEBUG
                                if (!(ovf >> h & 1u)) printf("guard: item %u band %u strip %u half %d lane %u step %u hi %d lo %d left_ok %d base %d\n", it, band, p, h, lane, s, hi_v, lo_v, int(left_ok), base[h]);
#endif
                                ovf |= 1u << h;
                            }
                        }
                    }
#pragma unroll
                    for (int c = 0; c < FW_C; ++c) {
                        Hp[c] = usubs2(Hp[c], d2);
                        F[c] = usubs2(F[c], d2);
                    }
                    dg = usubs2(dg, d2);
#pragma unroll
                    for (int rr = 0; rr < FW_R; ++rr) {
                        hl[rr] = usubs2(hl[rr], d2);
                        el[rr] = usubs2(el[rr], d2);
                    }
                    nxh = uint4{usubs2(nxh.x, d2), usubs2(nxh.y, d2), usubs2(nxh.z, d2), usubs2(nxh.w, d2)};
                    nxe = uint4{usubs2(nxe.x, d2), usubs2(nxe.y, d2), usubs2(nxe.z, d2), usubs2(nxe.w, d2)};
                    const uint32_t cur = ((s / (64 / FW_R)) & 1u) * 64u + lane;  // the block of the ring that is being consumed
                    s_look[0][cur] = usubs2(s_look[0][cur], d2);
                    s_look[1][cur] = usubs2(s_look[1][cur], d2);
                }
                const uint32_t blk = s / (64 / FW_R) + 1u;
                if (prog != nullptr && s >= 64u && (prog_every <= 1u || (s / 16u) % prog_every == 0u)) {
                    // (few couples: the 4-row blocks whose entries of this strip's right edge — lane 63's, written up to the step
                    // before — are out: the tile on the right reads them while this one goes on)
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    // (links: counted from the start of the band lane 63 is in — the newest of the run from step bnd + 64)
                    if (s >= bnd + 64u)
                        __hip_atomic_store(&prog[uint32_t(__builtin_amdgcn_readfirstlane(int(par(VP_FLAG))))], s - 63u - bnd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    else
                        __hip_atomic_store(&prog[uint32_t(__builtin_amdgcn_readfirstlane(int(par(VP_FLAG_PREV))))],
                                           s - 63u - uint32_t(__builtin_amdgcn_readfirstlane(int(par(VP_BND_PREV)))), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                publish(blk);
                if (left_rows) {  // (the rows the next fetch reads: 64 of them, two blocks of the ring ahead)
                    const uint32_t need_rows = min(16u * (blk + 2u), nblk_band);
                    if (need_rows > left_avail) {
                        (void)v2_wait_rows(&prog[left_idx], &flags[left_idx], need_rows, err, left_avail);
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    }
                }
                fetch(blk + 1u);
            }
            {
                // (qc of this step was shifted at the end of the previous one, and row 0's profile words are on their way)
                const uint32_t h4[FW_R] = {nxh.x, nxh.y, nxh.z, nxh.w}, e4[FW_R] = {nxe.x, nxe.y, nxe.z, nxe.w};
#pragma unroll
                for (int rr = 0; rr < FW_R; ++rr) {
                    hl[rr] = from_left_or(hl[rr], h4[rr]);
                    el[rr] = from_left_or(el[rr], e4[rr]);
                }
                const uint32_t nx = ((s + 1u) * FW_R) & 127u;
                nxh = *reinterpret_cast<const uint4*>(&s_look[0][nx]);
                nxe = *reinterpret_cast<const uint4*>(&s_look[1][nx]);
                nxq = *reinterpret_cast<const uint4*>(&s_look[2][nx]);
            }
            const int bi = int(s) - int(lane);
            bool act[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) act[h] = (lanef >> h & 1u) && bi >= 0 && uint32_t(bi) < nblk[h];
            if (act[0] || act[1]) {
                // wave-uniform: the special path is right for every lane (its extras are guarded per lane and half)
                const bool special = strip_has_lastc || (last_band[0] && s + 1u >= nblk[0] && s + 1u - nblk[0] < 64u) ||
                                     (last_band[1] && s + 1u >= nblk[1] && s + 1u - nblk[1] < 64u);
                auto row_cells = [&](int rr) __attribute__((always_inline)) {
                    const uint32_t hl_in = hl[rr];
                    const uint4 xa = *reinterpret_cast<const uint4*>(profA + (qc[rr] & 0xFFFFu));
                    const uint4 xb = *reinterpret_cast<const uint4*>(profB + (qc[rr] >> 16));
                    cells_u16(Hp, F, xa, xb, hl[rr], el[rr], dg, gd2);
                    dg = hl_in;
                };
                // ONE copy of the cells; what the last column / last row add comes after each row, behind a branch (four rows in one
                // basic block let the scheduler pull so much ahead that registers spilled, for no gain: the kernel is bound by issue)
#pragma unroll
                for (int rr = 0; rr < FW_R; ++rr) {
                    row_cells(rr);
                    if (special) {

#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const uint32_t i = r_lo + uint32_t(bi) * FW_R + rr;  // 0-based row
                            const uint32_t nh = par(VP_N0 + h), mh = par(VP_M0 + h);
                            const int gdh = int(par(VP_GD0 + h));
                            if (rr == 0 && bnd != 0u && uint32_t(bi) == bnd && act[h] && lastc[h] >= 0) {
                                // (links: this lane's first row block of the band the run went on into — the best of the band above is complete)
                                bandbest[par(VP_BEST0 + h) + band - 1u] = int2{bc[h], int(bc_i[h])};
                                bc[h] = ALN_NEG;
                                bc_i[h] = 0;
                            }
                            if (act[h] && i < nh) {  // (rows of the band: i < r_hi <= n)
                                if (lastc[h] >= 0) {
                                    const uint32_t lc = uint32_t(lastc[h]);
                                    const bool b0 = lc & 1u, b1 = lc & 2u, b2 = lc & 4u, b3 = lc & 8u;
                                    const uint32_t s0 = b0 ? Hp[1] : Hp[0], s1 = b0 ? Hp[3] : Hp[2], s2 = b0 ? Hp[5] : Hp[4], s3 = b0 ? Hp[7] : Hp[6],
                                                   s4 = b0 ? Hp[9] : Hp[8], s5 = b0 ? Hp[11] : Hp[10], s6 = b0 ? Hp[13] : Hp[12], s7 = b0 ? Hp[15] : Hp[14];
                                    const uint32_t u0 = b1 ? s1 : s0, u1 = b1 ? s3 : s2, u2 = b1 ? s5 : s4, u3 = b1 ? s7 : s6;
                                    const uint32_t v0 = b2 ? u1 : u0, v1 = b2 ? u3 : u2;
                                    int hm = v2_half(b3 ? v1 : v0, h) + base[h];
                                    hm += gdh - ge * int(i + 1u + mh);  // true H(i + 1, m)
                                    if (hm > bc[h]) {
                                        bc[h] = hm;
                                        bc_i[h] = i + 1u;
                                    }
                                }
                                if (i + 1u == nh) {  // last row: this lane's best cell, first column wins ties
                                    int br = ALN_NEG;
                                    uint32_t bj = 0;
                                    const int b0 = base[h] + gdh - ge * int(nh + jb);
#pragma unroll
                                    for (int c = 0; c < FW_C; ++c) {
                                        const int ht = v2_half(Hp[c], h) + b0 - ge * (c + 1);  // true H(n, jb + c + 1)
                                        if (jb + c < mh && ht > br) {
                                            br = ht;
                                            bj = jb + c + 1;
                                        }
                                    }
                                    lrow[par(VP_LROW0 + h) + p * 64u + lane] = int2{br, int(bj)};
                                }
                            }
                        }
                    }
                }
                const uint32_t ib = uint32_t(bi);  // row block of the band
                if (lanef & 16u) {  // a coarse column (rows past a pair's end carry junk in that half: nobody reads it)
                    // (entry = 8 words of data; its bases sit in the matching int2 of the cbase array, which lies a fixed number
                    // of words behind the data array: both indexed by the same entry number)
                    uint32_t* d = arena + co_off + uint64_t(ib) * 8u;
                    uint4* co = reinterpret_cast<uint4*>(d);
                    co[0] = uint4{hl[0], hl[1], hl[2], hl[3]};
                    co[1] = uint4{el[0], el[1], el[2], el[3]};
                    reinterpret_cast<int2*>(arena + cb_off)[ib] = int2{base[0], base[1]};
                }
                // a coarse row: the registers go out as they are, with the bases of the moment
                const uint32_t i1 = (ib + 1u) * FW_R;  // rows of the band that are done
                if ((i1 % CK2) == 0) {
                    // (one lane in every other step gets here.  A coarse row goes out for BOTH halves whenever the couple stores
                    // it: a half whose pair ends higher up writes junk nobody reads)
                    const uint32_t ckr1 = (r_lo + i1) / CK2;  // coarse row number, 1-based
                    if (ckr1 <= ncr) {
                        uint32_t* rh = arena + rd_off + uint64_t(2u * (ckr1 - 1u)) * mpad;
                        uint4* oh = reinterpret_cast<uint4*>(rh);
                        uint4* of = reinterpret_cast<uint4*>(rh + mpad);
#pragma unroll
                        for (int c = 0; c < FW_C; c += 4) {
                            oh[c / 4] = uint4{Hp[c], Hp[c + 1], Hp[c + 2], Hp[c + 3]};
                            of[c / 4] = uint4{F[c], F[c + 1], F[c + 2], F[c + 3]};
                        }
                        reinterpret_cast<int2*>(arena + rb_off)[uint64_t(ckr1 - 1u) * (mpad / 16u)] = int2{base[0], base[1]};
                    }
                }
            }
            {   // the next step's query codes, and the first of its profile rows
                const uint32_t q4[FW_R] = {nxq.x, nxq.y, nxq.z, nxq.w};
#pragma unroll
                for (int rr = 0; rr < FW_R; ++rr) qc[rr] = from_left_or(qc[rr], q4[rr]);
            }
        };
        {
            uint32_t s = 0;
            for (; s + 1u < nsteps; s += 2) {
                step(s, std::true_type{});
                step(s + 1u, std::false_type{});
            }
            for (; s < nsteps; ++s) step(s, std::true_type{});
        }
        if (bnd != 0u && nsteps <= bnd + 64u) finish_prev();  // (links: a last band of one row block — the loop ended before step bnd + 64)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            // (links: a pair without rows in the run's newest band wrote the best of its last band when that band was left)
            if (lastc[h] >= 0 && (bnd == 0u || nblk[h] > bnd)) bandbest[par(VP_BEST0 + h) + band] = int2{bc[h], int(bc_i[h])};
            if ((ovf >> h) & 1u) {
                const uint32_t pidh = par(VP_PID0 + h);
                if (pidh != 0xFFFFFFFFu) atomicOr(&ovf_out[pidh], 1u);
            }
        }
        if (lane == 0) {  // (statistics: the cells this tile computed, ioc_timings::n_align_cells_computed)
            unsigned long long cells = 0;
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (vh[h]) cells += (unsigned long long)(par(VP_RHI0 + h) - r_lo) * (unsigned long long)min(strip_cols, par(VP_M0 + h) - p * strip_cols);
            atomicAdd(cells_done, cells);
            atomicAdd(link_stats, 1u);  // (the run's first tile; the tiles it went on into were counted as they were entered)
        }
        // ---- publish: every store of the wave has landed, then the release, then the flag ----
        const uint32_t my_flag = uint32_t(__builtin_amdgcn_readfirstlane(int(par(VP_FLAG))));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(&flags[my_flag], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (every lane the same word, the same value)
        it = v2_dequeue(queue);
    }
}

#define V2_FWD_ARGS                                                                                                                        \
    const AlnPairDev *__restrict__ pairs, const V2Couple *__restrict__ couples, const V2Item *__restrict__ items, uint32_t n_items,        \
        uint32_t *__restrict__ queue, uint32_t *__restrict__ flags, uint32_t *__restrict__ err, const uint8_t *__restrict__ pool, AlnParams P, \
        uint32_t *__restrict__ arena, int2 *__restrict__ lrow, int2 *__restrict__ bandbest, uint32_t *__restrict__ ovf_out, int guard,     \
        const uint4 *__restrict__ prof, unsigned long long *__restrict__ cells_done, uint32_t *__restrict__ prog, uint32_t prog_every,  \
        uint32_t *__restrict__ claims, uint32_t link_mode
__global__ void __launch_bounds__(64 * V2_WAVES) __attribute__((amdgpu_waves_per_eu(3, 8))) k_fwd2(V2_FWD_ARGS)
{
    v2_fwd_body(pairs, couples, items, n_items, queue, flags, err, pool, P, arena, lrow, bandbest, ovf_out, guard, prof, cells_done, prog, prog_every, claims,
                link_mode);
}
// A launch that puts two workgroups on a compute unit (align_v2_run: the corridor's launches are bound by tiles in flight) has 256
// registers per lane to itself: the same body without the 19 registers k_fwd2 keeps in scratch.
__global__ void __launch_bounds__(64 * V2_WAVES) __attribute__((amdgpu_waves_per_eu(2, 2))) k_fwd2_w2(V2_FWD_ARGS)
{
    v2_fwd_body(pairs, couples, items, n_items, queue, flags, err, pool, P, arena, lrow, bandbest, ovf_out, guard, prof, cells_done, prog, prog_every, claims,
                link_mode);
}


// per pair: i, j, state, window bits, pushed, count, flag (0 done / not parked, 1 parked by the first traceback launch, 2 sent to the
// helper launch before any traceback: see k_fwd2_ends), - | the two launches' walk records (IOC_V2_TRACE_TIMES)
constexpr uint32_t V2_RESUME_WORDS = 16;
// ... and, in words of their own behind the lists of walks, where a walk's time went, per launch (IOC_V2_TRACE_TIMES): cycles / 256 for
// its blocks (waiting or recomputing), its tiles' recomputation and its walk loop | blocks of <= 64 columns, << 16: of <= 64 rows |
// systolic steps of the blocks it recomputed itself | ... of those of <= 64 columns | systolic steps of its tiles
constexpr uint32_t V2_SPLIT_WORDS = 24;

// After the probe launch (V2Couple): does either pair of the couple look like a wrong candidate?  Then the couple gets every tile.
// And: at the score per row the probe saw, will the pairs beat the certificate of the corridor the host planned (half width B0)?
// If not the corridor is widened here to what that rate asks for (+ 3 % + 512 columns), up to 0.4 of the length — or given up: a
// second pass over the refuted pairs costs more than the tiles the corridor saves.
__global__ void __launch_bounds__(64)
k_fwd2_probe(const AlnPairDev* __restrict__ pairs, V2Couple* __restrict__ couples, V2PairEnd* __restrict__ pe, const uint32_t* __restrict__ arena, AlnParams P)
{
    V2Couple& cp = couples[blockIdx.x];
    if (!cp.corridor) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t strip_cols = 64u * FW_C;
    const uint32_t R = uint32_t(cp.bstart[cp.probe_band + 1u]) * uint32_t(CK2);  // rows done at the end of the probe band
    const uint32_t ckr = R / uint32_t(CK2) - 1u;
    const uint32_t* rh = arena + cp.rdat + uint64_t(2u * ckr) * cp.mpad;
    const int2* rb = reinterpret_cast<const int2*>(arena + cp.rbase) + uint64_t(ckr) * (cp.mpad / 16u);
    bool wrong = false;
    uint32_t nmax = 0, mmax = 0, need = 0, need_raw = 0;
    for (int h = 0; h < 2; ++h) {
        if (cp.pid[h] == 0xFFFFFFFFu) continue;
        const AlnPairDev pr = pairs[cp.pid[h]];
        nmax = max(nmax, pr.n);
        mmax = max(mmax, pr.m);
        const int gd = pr.gap_open - P.gap_extend;
        int mx = INT32_MIN;
        const uint32_t x0 = uint32_t(cp.probe_strip) * strip_cols, x1 = min(pr.m, x0 + strip_cols);
        for (uint32_t x = x0 + lane; x < x1; x += 64) {
            const int2 bb = rb[x / 16u];
            mx = max(mx, v2_half(rh[x], h) + (h ? bb.y : bb.x) + gd - P.gap_extend * int(R + x + 1u));  // the true H(R, x + 1)
        }
        for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
        if (pr.n < R || x1 <= x0 || mx < P.match * int(R) / 4) {
            wrong = true;
        } else {
            // score S ~ rate x min(n, m); the certificate asks S > match (len - B): B > len - 0.97 S / match, + 512
            const float len = float(max(pr.n, pr.m)), rate = float(mx) / float(R);
            const float b = len - 0.97f * rate * float(min(pr.n, pr.m)) / float(P.match) + 512.0f;
            need = max(need, uint32_t(max(b, 0.0f)));
            // (the same without the margins: the probe's own guess of the least half width that passes)
            need_raw = max(need_raw, uint32_t(max(len - rate * float(min(pr.n, pr.m)) / float(P.match), 0.0f)));
        }
    }
    const uint32_t len_max = max(nmax, mmax);
    const uint32_t B0 = cp.b0;
    // The host planned B0 from the pairs' summed error rates (align_v2_run: a line fitted to the pairs seen so far, 4.5 sigma below
    // it), which predicts a pair's score to +- 0.9 %; the 1024 rows of the probe do to +- 2.6 %.  So the probe overrules the plan only
    // where it CONTRADICTS it — its own guess of the least passing width lies beyond the planned one — and then with its margins.
    if (!wrong && need_raw > B0 && need > B0) {
        // a wider corridor, planned like the host's (align_v2_run): the probe's tiles stay inside it (need >= B0)
        if (float(need) > 0.4f * float(len_max)) {
            wrong = true;
        } else if (lane == 0) {
            long long beff = 0x7FFFFFFFFFFFll;
            uint32_t skipped = 0;
            for (uint32_t b = 0; b < cp.nbands; ++b) {
                const uint32_t r0 = uint32_t(cp.bstart[b]) * uint32_t(CK2), r1 = min(nmax, uint32_t(cp.bstart[b + 1u]) * uint32_t(CK2));
                const uint32_t c_lo = r0 > need ? r0 - need : 0u;
                const unsigned long long c_hi = min((unsigned long long)mmax, (unsigned long long)r1 + need);
                const uint32_t lo = c_lo / strip_cols, hi = uint32_t((max(c_hi, 1ull) - 1ull) / strip_cols);
                cp.plo[b] = uint16_t(min(lo, uint32_t(cp.plo[b])));  // (never narrower than planned)
                cp.phi[b] = uint16_t(max(hi, uint32_t(cp.phi[b])));
                skipped += uint32_t(cp.plo[b]) + (cp.nstrips - 1u - uint32_t(cp.phi[b]));
                if (cp.plo[b] > 0) beff = min(beff, (long long)r0 - (long long)cp.plo[b] * strip_cols);
                if ((unsigned long long)(uint32_t(cp.phi[b]) + 1u) * strip_cols < mmax) beff = min(beff, (long long)(uint32_t(cp.phi[b]) + 1u) * strip_cols - (long long)r1);
            }
            for (int h = 0; h < 2; ++h)
                if (cp.pid[h] != 0xFFFFFFFFu) {
                    const AlnPairDev pr = pairs[cp.pid[h]];
                    const long long ct = (long long)P.match * max(0ll, (long long)max(pr.n, pr.m) - beff - 1ll);
                    pe[cp.pid[h]].cert = beff == 0x7FFFFFFFFFFFll ? INT32_MIN : int32_t(min(ct, 0x7FFFFFFFll));
                    // (a tapered plan: the one width `need` joined with it, the start bound of the grid as it is now)
                    if (pe[cp.pid[h]].start != INT32_MAX) pe[cp.pid[h]].start = v2_start_bound(cp, pr.n, pr.m, P.match);
                }
            if (skipped * 5u < cp.nbands * cp.nstrips) cp.corridor = 2u;  // (not worth it: open the grid below)
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    if ((wrong || __hip_atomic_load(&cp.corridor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 2u) && lane == 0) {
        for (uint32_t b = 0; b < uint32_t(V2_MAX_BANDS); ++b) {
            cp.plo[b] = 0;
            cp.phi[b] = uint16_t(min(65535u, cp.nstrips - 1u));
        }
        cp.corridor = 0;
        for (int h = 0; h < 2; ++h)
            if (cp.pid[h] != 0xFFFFFFFFu) pe[cp.pid[h]].cert = INT32_MIN;
    }
}

// The exit bound of every pair with a tapered corridor (V2PairEnd::exit), after the main launch: the pair's exit cells are the
// computed cells with a right, lower or lower-right neighbour that exists in the pair's own matrix and is skipped —
//   * the right edge of tile (b, phi[b]) where the pair has columns beyond it: the coarse column the tile wrote;
//   * the bottom row of a tile (b, p) whose tile (b + 1, p) is skipped, where the pair has rows below it: the band's coarse row —
// about n + m words per pair, read out of the arena as k_fwd2_probe reads them (true H = half + base + gd - ge (i + j); the zero
// half is "no score").  With plo and phi as the probe left them: no checkpoint of a skipped tile is read — the arena holds an
// earlier call's words there.  Plain loads, one maximum per wave at the end; blockIdx.y takes every gridDim.y-th band.
constexpr int V2_CERT_T = 256, V2_CERT_Y = 8;
__global__ void __launch_bounds__(V2_CERT_T)
k_fwd2_cert(const AlnPairDev* __restrict__ pairs, const V2Couple* __restrict__ couples, const uint32_t* __restrict__ order, uint32_t count, V2PairEnd* __restrict__ pe,
            const uint32_t* __restrict__ arena, AlnParams P)
{
    const uint32_t pslot = blockIdx.x;
    if (pslot >= count) return;
    const uint32_t pid = order[pslot];
    const V2PairEnd e = pe[pid];
    if (e.cert == INT32_MIN || e.start == INT32_MAX) return;  // (no corridor, or the parent bound alone)
    const V2Couple& cp = couples[e.couple];
    if (!cp.corridor) return;
    const AlnPairDev pr = pairs[pid];
    const int h = cp.pid[0] == pid ? 0 : 1;
    const uint32_t n = pr.n, m = pr.m, strip_cols = 64u * FW_C;
    const long long ge = P.gap_extend, gd = pr.gap_open - P.gap_extend, match = P.match;
    const uint32_t* cdat = arena + cp.cdat;
    const int2* cbase = reinterpret_cast<const int2*>(arena + cp.cbase);
    long long best = INT32_MIN;
    for (uint32_t b = blockIdx.y; b < cp.nbands; b += gridDim.y) {
        const uint32_t r0 = uint32_t(cp.bstart[b]) * uint32_t(CK2), R = uint32_t(cp.bstart[b + 1u]) * uint32_t(CK2);
        if (r0 >= n) break;
        const uint32_t r1 = min(n, R), lo = cp.plo[b], hi = cp.phi[b];
        const unsigned long long j = (hi + 1ull) * strip_cols;  // the right edge's column
        if (j < m) {
            const unsigned long long cc = j / uint32_t(CK2) - 1u;
            for (uint32_t row = r0 + threadIdx.x; row < r1; row += V2_CERT_T) {
                const unsigned long long en = cc * cp.nq + row / 4u;
                const int half = v2_half(cdat[en * 8u + (row & 3u)], h);
                if (half == 0) continue;
                const int2 bb = cbase[en];
                const long long i = row + 1u, H = half + (long long)(h ? bb.y : bb.x) + gd - ge * (i + (long long)j);
                best = max(best, H + match * min((long long)n - i, (long long)m - (long long)j));
            }
        }
        if (b + 1u < cp.nbands && R < n) {
            const uint32_t ckr = R / uint32_t(CK2) - 1u, lo2 = cp.plo[b + 1u], hi2 = cp.phi[b + 1u];
            const uint32_t* rh = arena + cp.rdat + uint64_t(2u * ckr) * cp.mpad;
            const int2* rb = reinterpret_cast<const int2*>(arena + cp.rbase) + uint64_t(ckr) * (cp.mpad / 16u);
            for (uint32_t p = lo; p <= hi; ++p) {
                if (p >= lo2 && p <= hi2) continue;
                const uint32_t x1 = uint32_t(min((unsigned long long)m, (p + 1ull) * strip_cols));
                for (uint32_t x = p * strip_cols + threadIdx.x; x < x1; x += V2_CERT_T) {
                    const int half = v2_half(rh[x], h);
                    if (half == 0) continue;
                    const int2 bb = rb[x / 16u];
                    const long long jj = x + 1u, H = half + (long long)(h ? bb.y : bb.x) + gd - ge * ((long long)R + jj);
                    best = max(best, H + match * min((long long)n - (long long)R, (long long)m - jj));
                }
            }
        }
    }
    int v = int(min(best, 0x7FFFFFFFll));
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63u) == 0 && v != INT32_MIN) atomicMax(&pe[pid].exit, v);
}

__global__ void __launch_bounds__(64)
k_fwd2_ends(const AlnPairDev* __restrict__ pairs, const V2Couple* __restrict__ couples, const uint32_t* __restrict__ order, uint32_t count, const V2PairEnd* __restrict__ pe,
            const int2* __restrict__ lrow, const int2* __restrict__ bandbest, const uint32_t* __restrict__ ovf, int4* __restrict__ ends,
            uint32_t* __restrict__ resume, uint32_t* __restrict__ early, const int route_below, const uint32_t route_cap)
{
    const uint32_t pslot = blockIdx.x;
    if (pslot >= count) return;
    const uint32_t pid = order[pslot], lane = threadIdx.x;
    const AlnPairDev pr = pairs[pid];
    const V2PairEnd e = pe[pid];
    const uint32_t n = pr.n, m = pr.m;
    const uint32_t nstrips = (m + 64u * FW_C - 1) / (64u * FW_C);
    int br = 0;  // H(n, 0)
    uint32_t bj = 0;
    for (uint32_t x = lane; x < nstrips * 64u; x += 64) {
        if (uint64_t(x) * FW_C >= m) continue;
        const int2 v = lrow[e.lrow0 + x];
        if (v.x > br || (v.x == br && uint32_t(v.y) < bj)) {
            br = v.x;
            bj = uint32_t(v.y);
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
        for (uint32_t b = 0; b < e.nbands; ++b) {
            if (uint64_t(couples[e.couple].bstart[b]) * CK2 >= n) break;
            const int2 bb = bandbest[e.best0 + b];
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
        // (corridor: the result stands only if it beats what a path through a skipped cell can reach — else flag 2: run again without)
        // (a tapered corridor: ... or the larger of the start bound and the exit cells' bound, if that is less — V2PairEnd)
        const int cert = e.start == INT32_MAX ? e.cert : min(e.cert, max(e.start, e.exit));
        const bool refuted = e.cert != INT32_MIN && fin <= cert;
        ends[pid] = int4{fin, int(bi), int(bjj), int(ovf[pid] & 1u) | (refuted ? 2 : 0)};
        // Verdict mode: a WRONG candidate (10 % of a sahlin batch's pairs) aligns with a score of ~0.02 per base where a pair of one
        // transcript has ~1.7 (IOC_V2_TRACE_TIMES prints both), its walk wanders through four times the blocks, and it is decided
        // last ("cannot reach the threshold any more").  Such a pair does not wait for the first traceback launch to park it:
        // it goes to the helper launch at once, which runs BESIDE the first launch.  (A guess about cost only: either launch walks
        // any pair to the same result.)  Long walks only (the helper launch takes one walk per workgroup: a walk of a few blocks is
        // better off among the thousands of the first launch), and no more of them than that launch has workgroups.
        // (... and every long walk of a launch with no more pairs than the helper launch has workgroups — a second, small
        // alignment round: with helpers a pair of one transcript is decided in half the time, and the chip has nothing else to do)
        if (route_below > 0 && pr.stop_at && !(ovf[pid] & 1u) && !refuted && min(n, m) >= 8u * uint32_t(CK2) &&
            (fin < route_below * int(min(n, m)) / 4 || count <= route_cap)) {
            const uint32_t slot = atomicAdd(&early[0], 1u);  // (the count may pass the cap: its readers take the minimum)
            if (slot < route_cap) {
                resume[size_t(pid) * V2_RESUME_WORDS + 6] = 2u;
                early[1u + slot] = pslot;
            }
        }
    }
}

// ---- pass 2 ------------------------------------------------------------------------------------------------------------
// One wave per pair, as k_align_trace; the 128-pitch checkpoints a tile needs come out of a per-wave scratch that holds those
// of ONE 512 x 512 block, recomputed (32-bit, on the slanted scores, from the block's coarse top row and left column) when the
// walk enters the block: fine rows k = 0..3 at block row 128 k (k = 0: the coarse row itself, or row 0 of the matrix), each
// 1 + 512 entries (entry 0 = the column left of the block: the diagonal input of the block's first column), and fine
// columns k = 0..3 at block column 128 k, 512 entries each.
struct V2Scratch {
    int2 frow[CK2 / TILE][CK2 + 8];
    int2 fcol[CK2 / TILE][CK2];
};

__device__ __forceinline__ int2 v2_ld(const int2* p)
{
    // scratch written by other lanes of this wave a moment ago: past the L1
    const int x = __hip_atomic_load(&p->x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int y = __hip_atomic_load(&p->y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return int2{x, y};
}

// Helper protocol of the second launch (HELP = true): one pair per workgroup, wave 0 walks, waves 1..10 recompute blocks ahead
// of it.  On entering a block B the walker posts (B, entry point); a helper then makes the block at its role's fixed offset
// from B — the two blocks the walk can enter next (above, left) and the three it can enter after those (two above, diagonal,
// two left): by the time the walk arrives anywhere, the block was asked for one request earlier.  A block takes a helper about
// as long as the walker spends in one, so every role has TWO helpers that take the requests in turn (even / odd): none is
// ever late.  A helper keeps its last two results and publishes (request, block) per buffer; the walker takes any published
// block with its coordinates from the last two requests — the extents asked for only ever shrink along a walk — waits for a
// helper that is on it, and recomputes the block itself otherwise.
constexpr uint32_t V2_NROLE = 5, V2_NHELP = 2 * V2_NROLE, V2_HBUF = 2, V2_HWAVES = 1 + V2_NHELP;
enum V2Help : uint32_t { VH_SEQ = 0, VH_RB, VH_CB, VH_I, VH_J, VH_QUIT, VH_WORK = 8 /* [h][seq, rb, cb] */, VH_SLOT = VH_WORK + 3 * V2_NHELP /* [h][b][seq, rb, cb] */,
                         VH_COUNT = VH_SLOT + 3 * V2_NHELP * V2_HBUF };

// HELP = false: four pairs per workgroup, one wave each.  max_blocks > 0: a walk that is still undecided when it needs more
// than max_blocks blocks parks its state in `resume` and leaves — the second launch (HELP = true) takes it on with helper
// waves: by then the pairs of one transcript are done (verdict mode: ~15 blocks) and the chip is all but empty, so the wrong
// candidates, whose walks wander off the diagonal through ~60 full blocks, get six waves each.
// EMIT (ioc_align_pairs_ops): the walk also writes its operation bytes (OpsOut) and is always exact — no stop_at, so it is never
// parked and never routed to the helper launch by k_fwd2_ends; global stores only, the LDS is the non-emitting variant's.
template <bool HELP, bool EMIT>
__device__ __forceinline__ void trace2_body(const AlnPairDev* __restrict__ pairs, const uint32_t* __restrict__ order, const uint8_t* __restrict__ pool,
                                            const AlnParams& P, const uint32_t* __restrict__ arena, const V2Couple* __restrict__ couples, const V2PairCk* __restrict__ pck,
                                            const int4* __restrict__ ends, V2Scratch* __restrict__ scratch, V2Scratch* __restrict__ hscratch,
                                            uint32_t* __restrict__ resume, uint32_t* __restrict__ park, uint32_t* __restrict__ split,
                                            int32_t* __restrict__ out_score, uint32_t* __restrict__ out_count, const uint32_t count, const uint32_t max_blocks,
                                            const unsigned long long max_cycles, const uint32_t pslot, const uint32_t wv, const uint32_t want,
                                            const typename OpsOut<EMIT>::Dev od)
{
    constexpr int NW = HELP ? int(V2_HWAVES) : TR_WAVES, NDIRS = HELP ? 1 : TR_WAVES;  // (only a walker keeps direction nibbles)
    // LDS of a wave: the left column and the query bytes of the TILE the walk is in (walkers only: one 12-byte record per row), and
    // ONE area that holds, by turns, what the recomputation of a block needs (its left column, its query codes, the profile of its
    // columns: 8.5 KB) and the direction nibbles of a tile (8 KB, and behind them the 128 reference bytes of the tile's columns: the
    // walk tells identical from different bases by the bytes themselves) — a walker does the one, then the other.  10 KB per
    // walker instead of 16.5: a compute unit that holds a workgroup of the helper launch still has room for one of the first
    // launch (they run side by side).
    constexpr uint32_t B_LEFT = uint32_t(CK2) * 8u, B_Q = uint32_t(CK2) * 4u, B_PROF = 5u * 64u * uint32_t(V2_BLK_C / 4) * 4u;
    constexpr uint32_t D_BYTES = uint32_t(TILE) * uint32_t(TR_C) / 4u * 64u * 2u;
    constexpr uint32_t U_BYTES = (B_LEFT + B_Q + B_PROF) > D_BYTES + uint32_t(TILE) ? (B_LEFT + B_Q + B_PROF) : D_BYTES + uint32_t(TILE);
    __shared__ __attribute__((aligned(16))) uint8_t s_union_all[NW][U_BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_tile_all[NDIRS][uint32_t(TILE) * 12u];  // (walkers: the tile's left column, its query bytes)
    __shared__ uint32_t s_help[VH_COUNT];
    if (pslot >= count) return;
    uint16_t(*dirs)[64] = reinterpret_cast<uint16_t(*)[64]>(&s_union_all[wv][0]);
    int2* const b_left = reinterpret_cast<int2*>(&s_union_all[wv][0]);                        // a block's left column
    uint32_t* const b_q = reinterpret_cast<uint32_t*>(&s_union_all[wv][B_LEFT]);             // ... its query bytes as profile-row offsets
    uint32_t* const b_prof = reinterpret_cast<uint32_t*>(&s_union_all[wv][B_LEFT + B_Q]);    // ... the query profile of its columns: [code][lane][V2_BLK_C / 4]
    struct TRec {  // a tile's row as its first lane takes it in: (Hq, E*) of the column left of the tile, the query byte
        int hq, e;
        uint32_t q;
    };
    static_assert(sizeof(TRec) == 12, "a row's record");
    TRec* const s_rec = reinterpret_cast<TRec*>(&s_tile_all[HELP ? 0u : wv][0]);
    uint8_t* const s_rb = &s_union_all[wv][D_BYTES];  // ... and the reference bytes of its columns (behind the nibbles, for the walk)
    const uint32_t pid = order[pslot];
    const AlnPairDev pr = pairs[pid];
    const V2PairCk ck = pck[pid];
    const int hf = int(ck.half);
    const bool corridor = __builtin_amdgcn_readfirstlane(int(couples[ck.couple].corridor)) != 0;
    uint32_t* const rs = resume + size_t(pid) * V2_RESUME_WORDS;
    {   // helper launch: the walks with the flag it was started for (1: parked by the first launch, 2: sent here by k_fwd2_ends);
        // first launch: everything but the latter
        const uint32_t fl = uint32_t(__builtin_amdgcn_readfirstlane(int(rs[6])));
        if (HELP ? fl != want : fl == 2u) return;
    }
    V2Scratch* scp = &scratch[pslot];  // where the current block's fine checkpoints are (a helper's buffer, when it made them)
    const unsigned long long t_begin = __builtin_amdgcn_s_memtime();
    uint32_t n_blocks = 0, n_diag = 0, n_tiles = 0, n_gapsteps = 0;  // (IOC_V2_TRACE_TIMES: what this pair's walk was made of)
    // ... and where its time went: getting a block (waiting for a helper's, or recomputing it), recomputing tiles, walking them
    unsigned long long t_blk = 0, t_tile = 0, t_walk = 0;
    unsigned long long t_own = 0, t_own_thin_c = 0, t_own_thin_r = 0;  // (of t_blk: recomputing blocks itself; in blocks of <= 64 columns / rows)
    uint32_t n_thin_c = 0, n_thin_r = 0, n_bsteps = 0, n_bsteps_thin = 0, n_tsteps = 0;  // (blocks of <= 64 columns / rows; systolic steps)
    uint32_t* const sp = split + size_t(pid) * V2_SPLIT_WORDS + (HELP ? V2_SPLIT_WORDS / 2u : 0u);
    auto split_out = [&]() {  // (lane 0, at the end of the walk in this launch)
        sp[0] = uint32_t(t_blk >> 8);
        sp[1] = uint32_t(t_tile >> 8);
        sp[2] = uint32_t(t_walk >> 8);
        sp[3] = n_thin_c | (n_thin_r << 16);
        sp[4] = n_bsteps;
        sp[5] = n_bsteps_thin;
        sp[6] = n_tsteps;
        sp[7] = uint32_t(t_own >> 8);
        sp[8] = uint32_t(t_own_thin_c >> 8);
        sp[9] = uint32_t(t_own_thin_r >> 8);
    };
    const uint32_t n = pr.n, m = pr.m;
    const int go = pr.gap_open, il = pr.ilimit;
    const uint8_t* __restrict__ q = pool + pr.q_off;
    const uint8_t* __restrict__ r = pool + pr.r_off;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t k = P.k, kmask = k >= 32 ? 0xFFFFFFFFu : ((1u << k) - 1u);
    const int4 en = ends[pid];
    if (en.w & 3) {  // the packed forward pass left its 16-bit window: the host sends the pair to the 32-bit kernel; or (2) the
        if (lane == 0) {  // corridor's result does not stand: the host runs the pair again without a corridor
            out_score[pid] = (en.w & 1) ? INT32_MIN : INT32_MIN + 1;
            out_count[pid] = 0xFFFFFFFFu;
            OpsOut<EMIT>{}.none(od, pid);
        }
        return;
    }
    const int gd = go - P.gap_extend, ge = P.gap_extend;
    FwdConst K;
    K.ge = ge;
    K.gd = gd;
    K.cm = P.match + 2 * ge + gd;
    K.cx = P.mismatch + 2 * ge + gd;
    uint32_t i = uint32_t(en.y), j = uint32_t(en.z);
    int state = 0;  // 0 = H, 1 = E, 2 = F
    WinStat ws;
    OpsOut<EMIT> ops;
    ops.begin(od, pid, n + m);
    if (!EMIT && HELP && want == 1u) {  // the walk the first launch parked
        i = rs[0];
        j = rs[1];
        state = int(rs[2]);
        ws.wb = rs[3];
        ws.pushed = rs[4];
        ws.cnt = rs[5];
    } else {
        ws.blanks((m - j) + (n - i), kmask, k, il);  // trailing end gaps are the tail of the string
        ops.fill('d', m - j, lane);
        ops.fill('i', n - i, lane);
    }
    uint32_t blk_r = 0xFFFFFFFFu, blk_c = 0xFFFFFFFFu;  // the block whose fine checkpoints the scratch holds
    // coarse checkpoints, decoded: row R (a multiple of CK2, > 0), 0-based column index x; column C, 0-based row index y
    auto coarse_row = [&](uint32_t R, uint32_t x) {
        const uint32_t ckr = R / CK2 - 1u;
        const uint32_t* rh = arena + ck.rdat + uint64_t(2u * ckr) * ck.mpad;
        const int2 bb = reinterpret_cast<const int2*>(arena + ck.rbase)[uint64_t(ckr) * (ck.mpad / 16u) + x / 16u];
        const int bs = hf ? bb.y : bb.x;
        return int2{v2_half(rh[x], hf) + bs, v2_half(rh[ck.mpad + x], hf) + bs};
    };
    auto coarse_col = [&](uint32_t C, uint32_t y) {
        const uint64_t e = uint64_t(C / CK2 - 1u) * ck.nq + y / 4u;
        const uint32_t* d = arena + ck.cdat + e * 8u;
        const int2 bb = reinterpret_cast<const int2*>(arena + ck.cbase)[e];
        const int bs = hf ? bb.y : bb.x;
        return int2{v2_half(d[y & 3u], hf) + bs, v2_half(d[4u + (y & 3u)], hf) + bs};
    };

    // Corridor: a block lies in ONE tile of the forward pass (bands are whole coarse rows, a strip is two coarse columns); what
    // that tile took for "no score" because its neighbour above / to the left / above-left was not computed is "no score"
    // in the block too (the checkpoints of a skipped tile were never written)
    auto block_edges = [&](const uint32_t Rb, const uint32_t Cb, bool& top_ok, bool& left_ok, bool& corner_ok) __attribute__((always_inline)) {
        top_ok = left_ok = corner_ok = true;
        if (corridor) {
            const V2Couple& cq = couples[ck.couple];
            auto band_of = [&](uint32_t row) {
                const uint32_t cr = row / uint32_t(CK2);
                uint32_t b = 0;
                while (b + 1u < cq.nbands && uint32_t(cq.bstart[b + 1u]) <= cr) ++b;
                return b;
            };
            auto in = [&](uint32_t b, uint32_t p) { return p >= cq.plo[b] && p <= cq.phi[b]; };
            const uint32_t ps = Cb / (64u * FW_C), pl = Cb ? (Cb - 1u) / (64u * FW_C) : 0u;
            const uint32_t bb = band_of(Rb), bt = Rb ? band_of(Rb - 1u) : 0u;
            if (Rb) top_ok = in(bt, ps);
            if (Cb) left_ok = in(bb, pl);
            if (Rb && Cb) corner_ok = in(bt, pl);
        }
    };

    // the fine checkpoints of the block (Rb, Cb) — rows Rb + 1 .. Rb + brows, columns Cb + 1 .. Cb + bcols — recomputed into dst
    // from the coarse row above and the coarse column to the left (uses this wave's LDS: b_left, b_q, b_prof)
    auto recompute_block_c = [&](auto cpl, auto rps, const uint32_t Rb, const uint32_t Cb, const uint32_t brows, const uint32_t bcols, V2Scratch& dst) __attribute__((always_inline)) {
        constexpr int BC = decltype(cpl)::value;  // columns per lane
        constexpr int RS = decltype(rps)::value;  // rows per step
        static_assert(RS == FW_R || RS == FW_R / 2, "a step's rows of the left column are one or two 16-byte LDS reads");
        // (an opaque copy: what a variant derives from the lane stays inside it.  Derived from `lane` itself it is hoisted out of the
        // walk's loop for both variants at once — 144 registers in k_trace2_help instead of 111, and three helper waves and a
        // first-launch wave no longer share a SIMD's 512)
        const uint32_t ln = opaque(lane);
        bool top_ok, left_ok, corner_ok;
        block_edges(Rb, Cb, top_ok, left_ok, corner_ok);
        // fine row 0 and fine column 0: the coarse checkpoints (or the matrix edges)
        for (uint32_t x = ln; x <= bcols; x += 64) {  // entry x = column Cb + x (x = 0: left of the block)
            int2 v;
            if (Rb == 0)
                v = int2{ge * int(Cb + x) - gd, ALN_NEG};              // row 0: H = 0
            else if (Cb + x == 0)
                v = int2{ge * int(Rb) - gd, ALN_NEG};                  // column 0: H = 0
            else if (x ? top_ok : corner_ok)
                v = coarse_row(Rb, Cb + x - 1u);
            else
                v = int2{ALN_NEG, ALN_NEG};
            dst.frow[0][x] = v;
        }
        for (uint32_t y = ln; y < brows; y += 64) {  // entry y = row Rb + 1 + y
            int2 v{ge * int(Rb + y + 1) - gd, ALN_NEG};  // column 0: H = 0, no gap to extend
            if (Cb) v = left_ok ? coarse_col(Cb, Rb + y) : int2{ALN_NEG, ALN_NEG};
            dst.fcol[0][y] = v;
            b_left[y] = v;
            const uint32_t ch = q[Rb + y];
            b_q[y] = (ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u) * uint32_t(64 * (BC / 4) * 4);  // byte offset of the profile row
        }
        for (uint32_t y = brows + ln; y < ((brows + 3u) & ~3u) + 4u && y < uint32_t(CK2); y += 64) {
            b_left[y] = int2{0, ALN_NEG};
            b_q[y] = 0;
        }
        const uint32_t jb8 = Cb + ln * BC;
        uint32_t rpk[BC / 4];
#pragma unroll
        for (int c4 = 0; c4 < BC / 4; ++c4) {
            uint32_t w = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) w |= ref_byte(r, m, pr.rc, jb8 + c4 * 4 + e) << (8 * e);
            rpk[c4] = w;
        }
        {   // the diagonal increments of this lane's BC columns for each query base, four to a word (k_align_fwd's profile)
            const uint32_t bases = 'A' | ('C' << 8) | ('G' << 16) | ('T' << 24);
#pragma unroll
            for (int code = 0; code < 5; ++code) {
                const uint32_t bq = code < 4 ? (bases >> (8 * code)) & 0xFFu : 0x100u;  // 0x100: equals no byte
#pragma unroll
                for (int c4 = 0; c4 < BC / 4; ++c4) {
                    uint32_t w = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) w |= uint32_t(((rpk[c4] >> (8 * e)) & 0xFFu) == bq ? K.cm : K.cx) << (8 * e);
                    b_prof[(uint32_t(code) * 64u + ln) * uint32_t(BC / 4) + uint32_t(c4)] = w;
                }
            }
        }
        const uint8_t* bprof = reinterpret_cast<const uint8_t*>(&b_prof[ln * uint32_t(BC / 4)]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        tr_wave_sync();
        int Hb[BC], Fb[BC];
        int dgb;
        {
            const uint32_t x0 = ln * BC;  // this lane's first column is entry x0 + 1
#pragma unroll
            for (int c = 0; c < BC; ++c) {
                int2 v{0, ALN_NEG};
                if (x0 + c + 1 <= bcols) v = v2_ld(&dst.frow[0][x0 + c + 1]);
                Hb[c] = v.x;
                Fb[c] = v.y;
            }
            dgb = x0 <= bcols ? v2_ld(&dst.frow[0][x0]).x : 0;
        }
        const uint32_t nactb = (bcols + BC - 1) / BC;
        const uint32_t nblkb = (brows + RS - 1) / RS, nstepb = nblkb + nactb - 1u;
        // entry 0 of the fine rows 1 .. 3: Hq(Rb + 128 k, Cb), the diagonal input of the first column below the row
        if (ln >= 1u && ln < uint32_t(CK2 / TILE) && ln * uint32_t(TILE) <= brows) dst.frow[ln][0] = int2{b_left[ln * uint32_t(TILE) - 1u].x, ALN_NEG};
        // Lane l has the row block s - l at step s: it works while l <= s < l + nblkb.  The loop is peeled as the tile step's is,
        // by what the lanes' activity takes: switching on (LO), all at work, switching off (HI), both at once in a block of fewer
        // row blocks than lanes.  Lane 0's inputs of step s + 1 are read at step s (PRE), by every lane at one address, while row
        // blocks are left.  Every address is a pointer that runs along; two steps to a round, so that what moves one lane per
        // step changes registers instead of being copied.
        if (ln < nactb) {
            int hl4[RS], el4[RS];
            uint32_t qc4[RS];
#pragma unroll
            for (int rr = 0; rr < RS; ++rr) {
                hl4[rr] = 0;
                el4[rr] = ALN_NEG;
                qc4[rr] = 0;
            }
            const int2* lp = b_left;
            const uint32_t* qp = b_q;
            uint4 nl0, nl1{}, nq4{};
            auto next_rows = [&]() __attribute__((always_inline)) {  // (Hq, E*) and the profile rows of the RS rows at lp / qp
                nl0 = *reinterpret_cast<const uint4*>(&lp[0]);
                if constexpr (RS == 4) {
                    nl1 = *reinterpret_cast<const uint4*>(&lp[2]);
                    nq4 = *reinterpret_cast<const uint4*>(&qp[0]);
                } else {
                    const uint2 q2 = *reinterpret_cast<const uint2*>(&qp[0]);
                    nq4.x = q2.x;
                    nq4.y = q2.y;
                }
            };
            next_rows();
            // fine column k at block column 128 k: the right edge of the lane whose columns end there, RS rows (16-byte stores)
            // per step; rows past brows up to the next multiple of RS lie inside the column and are never read
            const bool fine_col_lane = ((ln + 1u) * BC) % TILE == 0 && (ln + 1u) * BC < uint32_t(CK2);
            uint8_t* fcp = reinterpret_cast<uint8_t*>(&dst.fcol[fine_col_lane ? ((ln + 1u) * BC) / TILE : 0u][0]) - size_t(ln) * (RS * sizeof(int2));  // (row block s - ln)
            // fine row k at block row 128 k: a lane's BC columns when it has done 128 k / RS row blocks, k <= 3 and 128 k <= brows
            uint8_t* frp = reinterpret_cast<uint8_t*>(&dst.frow[1][1u + ln * BC]);
            const uint32_t fr_last = min(brows / uint32_t(RS), uint32_t((CK2 - TILE) / RS));
            uint32_t done = 0u - ln;  // row blocks this lane has done (a lane that has not begun: "negative")
            auto bstep = [&](auto lo, auto hi, auto pre, const uint32_t s) __attribute__((always_inline)) {
                {
                    const uint32_t h4[4] = {nl0.x, nl0.z, nl1.x, nl1.z}, e4[4] = {nl0.y, nl0.w, nl1.y, nl1.w},
                                   q4[4] = {nq4.x, nq4.y, nq4.z, nq4.w};  // (the first RS of them)
#pragma unroll
                    for (int rr = 0; rr < RS; ++rr) {
                        hl4[rr] = int(from_left_or(uint32_t(hl4[rr]), h4[rr]));
                        el4[rr] = int(from_left_or(uint32_t(el4[rr]), e4[rr]));
                        qc4[rr] = from_left_or(qc4[rr], q4[rr]);
                    }
                    if (decltype(pre)::value) {
                        lp += RS;
                        qp += RS;
                        next_rows();
                    }
                }
                ++done;
                bool act = true;
                if (decltype(lo)::value) act = ln <= s;
                if (decltype(hi)::value) act = act && int(ln) > int(s) - int(nblkb);
                if (act) {
#pragma unroll
                    for (int rr = 0; rr < RS; ++rr) {
                        const int hl_in = hl4[rr];
                        uint32_t xw[BC / 4];
                        if constexpr (BC == 8) {
                            const uint2 xw2 = *reinterpret_cast<const uint2*>(bprof + qc4[rr]);
                            xw[0] = xw2.x;
                            xw[1] = xw2.y;
                        } else {
                            static_assert(BC == 4, "one or two profile words per ln");
                            xw[0] = *reinterpret_cast<const uint32_t*>(bprof + qc4[rr]);
                        }
                        fwd_cells<BC, true>(Hb, Fb, xw, hl4[rr], el4[rr], dgb, qc4[rr], K);
                        dgb = hl_in;
                    }
                    if (fine_col_lane) {
                        reinterpret_cast<int4*>(fcp)[0] = int4{hl4[0], el4[0], hl4[1], el4[1]};
                        if constexpr (RS == 4) reinterpret_cast<int4*>(fcp)[1] = int4{hl4[2], el4[2], hl4[3], el4[3]};
                    }
                    if ((done & uint32_t(TILE / RS - 1)) == 0u && done <= fr_last) {
                        int2* f2 = reinterpret_cast<int2*>(frp);  // (entry 1 + BC ln: 8 bytes past a 16-byte boundary)
                        f2[0] = int2{Hb[0], Fb[0]};
#pragma unroll
                        for (int c = 1; c + 1 < BC; c += 2) *reinterpret_cast<int4*>(f2 + c) = int4{Hb[c], Fb[c], Hb[c + 1], Fb[c + 1]};
                        f2[BC - 1] = int2{Hb[BC - 1], Fb[BC - 1]};
                        frp += sizeof(dst.frow[0]);
                    }
                }
                fcp += RS * sizeof(int2);
            };
            auto run = [&](auto lo, auto hi, auto pre, uint32_t& s, const uint32_t end) __attribute__((always_inline)) {
                for (; s + 1u < end; s += 2) {
                    bstep(lo, hi, pre, s);
                    bstep(lo, hi, pre, s + 1u);
                }
                if (s < end) {
                    bstep(lo, hi, pre, s);
                    ++s;
                }
            };
            constexpr std::true_type yes{};
            constexpr std::false_type no{};
            uint32_t s = 0;
            run(yes, no, yes, s, min(nactb, nblkb) - 1u);
            run(no, no, yes, s, nblkb - 1u);    // (more row blocks than lanes)
            run(yes, yes, no, s, nactb - 1u);   // (fewer)
            run(no, yes, no, s, nstepb);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        tr_wave_sync();
        return nstepb;
    };

    // The same for a block of <= 64 columns, with the lanes along the ROWS.  The recurrence is symmetric: lane l takes the rows
    // 8 l + 1 .. 8 l + 8 of the block, one column per step, the lanes one step apart — bcols + lanes - 1 steps of 8 cells with
    // every lane that has rows at work, where the column shapes keep at most 16 lanes busy for 128 steps and more.  What changes
    // sides: a lane's profile is over its eight QUERY bases and is indexed by the column's reference base; the block's top row
    // (<= 65 entries, the profile row of each column's base beside them: b_q's place) enters at lane 0 as the left column does
    // there; a lane keeps (Hq, E*) of its rows from column to column and hands (Hq, F*) of its last row down.  Fine rows 1 .. 3
    // come out of lanes 15 / 31 / 47, one entry per step; such a block has no fine column but the coarse one.
    auto recompute_block_t = [&](const uint32_t Rb, const uint32_t Cb, const uint32_t brows, const uint32_t bcols, V2Scratch& dst) __attribute__((always_inline)) {
        constexpr int BR = V2_BLK_C;  // rows per lane
        static_assert(BR == 8, "two profile words per lane");
        const uint32_t ln = opaque(lane);
        bool top_ok, left_ok, corner_ok;
        block_edges(Rb, Cb, top_ok, left_ok, corner_ok);
        int4* const b_top = reinterpret_cast<int4*>(b_q);
        static_assert((64u + 1u) * sizeof(int4) <= B_Q, "the top row of a block of <= 64 columns");
        // fine row 0 and fine column 0: the coarse checkpoints (or the matrix edges), as recompute_block_c has them
        for (uint32_t x = ln; x <= bcols; x += 64) {  // entry x = column Cb + x (x = 0: left of the block)
            int2 v;
            if (Rb == 0)
                v = int2{ge * int(Cb + x) - gd, ALN_NEG};
            else if (Cb + x == 0)
                v = int2{ge * int(Rb) - gd, ALN_NEG};
            else if (x ? top_ok : corner_ok)
                v = coarse_row(Rb, Cb + x - 1u);
            else
                v = int2{ALN_NEG, ALN_NEG};
            dst.frow[0][x] = v;
            uint32_t po = 0;
            if (x) {
                const uint32_t ch = ref_byte(r, m, pr.rc, Cb + x - 1u);
                po = (ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u) * uint32_t(64 * (BR / 4) * 4);  // byte offset of the profile row
            }
            b_top[x] = int4{v.x, v.y, int(po), 0};
        }
        const uint32_t nact = (brows + BR - 1) / BR;
        for (uint32_t y = ln; y < brows; y += 64) {  // entry y = row Rb + 1 + y
            int2 v{ge * int(Rb + y + 1) - gd, ALN_NEG};
            if (Cb) v = left_ok ? coarse_col(Cb, Rb + y) : int2{ALN_NEG, ALN_NEG};
            dst.fcol[0][y] = v;
            b_left[y] = v;
        }
        for (uint32_t y = brows + ln; y < nact * BR; y += 64) b_left[y] = int2{0, ALN_NEG};
        {   // the diagonal increments of this lane's BR rows for each reference base, four to a word
            uint32_t qpk[BR / 4];
#pragma unroll
            for (int c4 = 0; c4 < BR / 4; ++c4) {
                uint32_t w = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t y = ln * BR + c4 * 4 + e;
                    w |= (y < brows ? uint32_t(q[Rb + y]) : 0u) << (8 * e);  // (0: equals no base)
                }
                qpk[c4] = w;
            }
            const uint32_t bases = 'A' | ('C' << 8) | ('G' << 16) | ('T' << 24);
#pragma unroll
            for (int code = 0; code < 5; ++code) {
                const uint32_t bq = code < 4 ? (bases >> (8 * code)) & 0xFFu : 0x100u;  // 0x100: equals no byte
#pragma unroll
                for (int c4 = 0; c4 < BR / 4; ++c4) {
                    uint32_t w = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) w |= uint32_t(((qpk[c4] >> (8 * e)) & 0xFFu) == bq ? K.cm : K.cx) << (8 * e);
                    b_prof[(uint32_t(code) * 64u + ln) * uint32_t(BR / 4) + uint32_t(c4)] = w;
                }
            }
        }
        const uint8_t* bprof = reinterpret_cast<const uint8_t*>(&b_prof[ln * uint32_t(BR / 4)]);
        tr_wave_sync();
        const uint32_t nstep = bcols + nact - 1u;
        if (ln >= 1u && ln < uint32_t(CK2 / TILE) && ln * uint32_t(TILE) <= brows) dst.frow[ln][0] = int2{b_left[ln * uint32_t(TILE) - 1u].x, ALN_NEG};
        if (ln < nact) {
            int Hr[BR], Er[BR];  // (Hq, E*) of this lane's rows in the column to the left
#pragma unroll
            for (int c = 0; c < BR; ++c) {
                const int2 v = b_left[ln * BR + c];
                Hr[c] = v.x;
                Er[c] = v.y;
            }
            const int dg_left = b_left[ln ? ln * BR - 1u : 0u].x;
            int dgt = ln ? dg_left : b_top[0].x;  // Hq of the row above in the column left of the block
            int out_h = 0, out_f = ALN_NEG;
            uint32_t out_p = 0;
            const int4* tp = b_top + 1;
            int4 nrec = tp[0];
            const bool fine_row_lane = ((ln + 1u) * BR) % TILE == 0 && (ln + 1u) * BR < uint32_t(CK2) && (ln + 1u) * BR <= brows;
            uint8_t* frp = reinterpret_cast<uint8_t*>(&dst.frow[fine_row_lane ? ((ln + 1u) * BR) / TILE : 0u][1]) - size_t(ln) * sizeof(int2);  // (column s - ln)
            // lane l has the column s - l at step s; peeled as the other shapes' loops are
            auto cstep = [&](auto lo, auto hi, auto pre, const uint32_t s) __attribute__((always_inline)) {
                int hu = int(from_left_or(uint32_t(out_h), uint32_t(nrec.x)));
                int fu = int(from_left_or(uint32_t(out_f), uint32_t(nrec.y)));
                const uint32_t po = from_left_or(out_p, uint32_t(nrec.z));
                if (decltype(pre)::value) nrec = tp[1];
                ++tp;
                bool act = true;
                if (decltype(lo)::value) act = ln <= s;
                if (decltype(hi)::value) act = act && int(ln) > int(s) - int(bcols);
                if (act) {
                    const int hu_in = hu;
                    const uint2 xw2 = *reinterpret_cast<const uint2*>(bprof + po);
                    const uint32_t xw[BR / 4] = {xw2.x, xw2.y};
                    fwd_cells<BR, true>(Hr, Er, xw, hu, fu, dgt, po, K);  // (down the column: F is what runs along, E what stays)
                    dgt = hu_in;
                    if (fine_row_lane) *reinterpret_cast<int2*>(frp) = int2{hu, fu};
                }
                frp += sizeof(int2);
                out_h = hu;
                out_f = fu;
                out_p = po;
            };
            auto run = [&](auto lo, auto hi, auto pre, uint32_t& s, const uint32_t end) __attribute__((always_inline)) {
                for (; s + 1u < end; s += 2) {
                    cstep(lo, hi, pre, s);
                    cstep(lo, hi, pre, s + 1u);
                }
                if (s < end) {
                    cstep(lo, hi, pre, s);
                    ++s;
                }
            };
            constexpr std::true_type yes{};
            constexpr std::false_type no{};
            uint32_t s = 0;
            run(yes, no, yes, s, min(nact, bcols) - 1u);
            run(no, no, yes, s, bcols - 1u);   // (more columns than lanes)
            run(yes, yes, no, s, nact - 1u);   // (fewer)
            run(no, yes, no, s, nstep);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        tr_wave_sync();
        return nstep;
    };

    // A block's step costs what its cells per lane cost, and a column shape runs rows / 4 + lanes - 1 of them: a block clipped to
    // half of its columns or fewer (every other block of a walk next to the diagonal is) takes 4 columns per lane — half the
    // cells in a step, at most 32 steps more — and one of <= 64 columns the lanes along its rows.  Same cells, same checkpoints
    // at the same places.  Returns the steps it ran.
    auto recompute_block = [&](const uint32_t Rb, const uint32_t Cb, const uint32_t brows, const uint32_t bcols, V2Scratch& dst) __attribute__((always_inline)) {
        if (bcols <= 64u) return recompute_block_t(Rb, Cb, brows, bcols, dst);
        if (bcols <= 64u * uint32_t(V2_BLK_C / 2))
            return recompute_block_c(std::integral_constant<int, V2_BLK_C / 2>{}, std::integral_constant<int, FW_R>{}, Rb, Cb, brows, bcols, dst);
        if (brows <= 64u)  // (fill is four fifths of such a block's steps: half the rows in a step)
            return recompute_block_c(std::integral_constant<int, V2_BLK_C>{}, std::integral_constant<int, FW_R / 2>{}, Rb, Cb, brows, bcols, dst);
        return recompute_block_c(std::integral_constant<int, V2_BLK_C>{}, std::integral_constant<int, FW_R>{}, Rb, Cb, brows, bcols, dst);
    };

    // verdict mode: the walk ends as soon as the count has reached stop_at (the windows still to come can only add) or cannot
    // reach it any more (every further column of the alignment ends at most one more window: at most i + j + k of them)
    const uint32_t stop_at = EMIT ? 0u : pr.stop_at;
    // ... or, second bound: a window that still counts holds >= il matches, a match column lies in at most k windows, and at most
    // min(i, j) match columns are left (plus what the k - 1 windows that reach back into the walked part find there): no more than
    // (k min(i, j) + (k - 1)^2) / il windows can follow.  With il of k = 9 of 11 that is 1.22 min(i, j) against i + j.
    // (floor(x / il) < y  <=>  x < y il: no division in the walk's loop; called with cnt_ < stop_at only)
    auto cannot_reach = [&](uint32_t cnt_, uint32_t i_, uint32_t j_) {
        const unsigned long long room = (unsigned long long)(stop_at - cnt_);
        if ((unsigned long long)i_ + j_ + k < room) return true;
        return il >= 1 && (unsigned long long)k * min(i_, j_) + (unsigned long long)((k - 1u) * (k - 1u)) < room * (unsigned long long)il;
    };
    bool decided = stop_at && (ws.cnt >= stop_at || cannot_reach(ws.cnt, i, j));
    const uint32_t help_addr = uint32_t(reinterpret_cast<uintptr_t>(&s_help[0]));  // LDS byte address of the protocol words
    uint32_t help_seq = 0, n_helped = 0;
    if (HELP) {
        if (wv == 0u) {
            for (uint32_t x = lane; x < uint32_t(VH_COUNT); x += 64) s_help[x] = 0u;
        }
        __syncthreads();
        if (wv != 0u) {
            // ---- helper h: the block dr blocks above and dc blocks to the left of the walker's current one ----
            const uint32_t h = wv - 1u, role = h % V2_NROLE, turn = h / V2_NROLE;  // (this helper's requests: seq % 2 == turn)
            const int dr = role == 0u ? 1 : role == 2u ? 2 : role == 3u ? 1 : 0;   // blocks up
            const int dc = role == 1u ? 1 : role == 3u ? 1 : role == 4u ? 2 : 0;   // blocks left
            uint32_t last = 0;
            for (;;) {
                uint32_t seq = 0;
                bool quit = false;
                for (uint32_t it = 0; it < (1u << 24); ++it) {
                    quit = v2_par(help_addr + 4u * VH_QUIT) != 0u;
                    seq = v2_par(help_addr + 4u * VH_SEQ);
                    if (quit || seq != last) break;
                    __builtin_amdgcn_s_sleep(8);
                }
                if (quit || seq == last) return;  // (the second: the walker never came back — nothing to wait for)
                const uint32_t qRb = v2_par(help_addr + 4u * VH_RB), qCb = v2_par(help_addr + 4u * VH_CB), qi = v2_par(help_addr + 4u * VH_I),
                               qj = v2_par(help_addr + 4u * VH_J);
                if (v2_par(help_addr + 4u * VH_SEQ) != seq) continue;  // (a newer request overtook the read: take that one)
                last = seq;
                if ((seq & 1u) != turn) continue;  // (the other helper of this role)
                if (qRb < uint32_t(dr * CK2) || qCb < uint32_t(dc * CK2)) continue;  // (off the matrix)
                const uint32_t tRb = qRb - uint32_t(dr * CK2), tCb = qCb - uint32_t(dc * CK2);
                // rows: the whole block once the walk has moved up, else what the entry point leaves; columns alike
                const uint32_t trows = dr ? uint32_t(CK2) : min(qi, qRb + uint32_t(CK2)) - qRb;
                const uint32_t tcols = dc ? uint32_t(CK2) : min(qj, qCb + uint32_t(CK2)) - qCb;
                const uint32_t wk = help_addr + 4u * (VH_WORK + 3u * h), buf = (seq >> 1) % V2_HBUF;
                const uint32_t sl = help_addr + 4u * (VH_SLOT + 3u * (h * V2_HBUF + buf));
                v2_lds_store(sl, 0u);  // (the buffer's old content goes)
                v2_lds_store(wk + 4u, tRb);
                v2_lds_store(wk + 8u, tCb);
                v2_lds_store(wk, seq);
                recompute_block(tRb, tCb, trows, tcols, hscratch[(size_t(HELP ? blockIdx.x : 0u) * V2_NHELP + size_t(h)) * V2_HBUF + size_t(buf)]);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                v2_lds_store(sl + 4u, tRb);
                v2_lds_store(sl + 8u, tCb);
                v2_lds_store(sl, seq);
                v2_lds_store(wk, 0u);
            }
        }
    }
    while (i > 0 && j > 0 && !decided) {
        const uint32_t r0 = ((i - 1) / TILE) * TILE, c0 = ((j - 1) / TILE) * TILE;
        const uint32_t rows = i - r0, cols = j - c0;
        const uint32_t Rb = (r0 / CK2) * CK2, Cb = (c0 / CK2) * CK2;
        if (Rb != blk_r || Cb != blk_c) {
            // ================= the block (Rb, Cb): rows Rb + 1 .. min(i, Rb + 512), columns Cb + 1 .. min(j, Cb + 512) =================
            blk_r = Rb;
            blk_c = Cb;
            ++n_blocks;
            n_diag += Rb == Cb ? 1u : 0u;
            const uint32_t brows = min(i, Rb + CK2) - Rb, bcols = min(j, Cb + CK2) - Cb;
            // (first launch) a walk that needs more than max_blocks blocks parks here: the second launch gives it helper waves
            // (verdict mode only: a walk that has to go to the end anyway gains nothing from a second launch that holds 256 walks
            // at a time.  A pair of one transcript is decided after about two blocks per 512 good windows it needs; max_blocks
            // is the slack on top of that.)
            if (!HELP && max_blocks && stop_at &&
                (n_blocks > 2u * (stop_at / uint32_t(CK2) + 1u) + max_blocks || (max_cycles && __builtin_amdgcn_s_memtime() - t_begin > max_cycles))) {
                if (lane == 0) {
                    rs[0] = i;
                    rs[1] = j;
                    rs[2] = uint32_t(state);
                    rs[3] = ws.wb;
                    rs[4] = ws.pushed;
                    rs[5] = ws.cnt;
                    rs[6] = 1u;
                    park[1u + atomicAdd(&park[0], 1u)] = pslot;  // (the second launch's work list)
                    const unsigned long long dt = __builtin_amdgcn_s_memtime() - t_begin;
                    rs[8] = uint32_t(dt >> 8);
                    rs[9] = (n_blocks - 1u) | (n_diag << 16);
                    rs[10] = n_tiles;
                    rs[11] = n_gapsteps;
                    split_out();
                }
                return;
            }
            const unsigned long long t_blk0 = __builtin_amdgcn_s_memtime();
            n_thin_c += bcols <= 64u ? 1u : 0u;
            n_thin_r += brows <= 64u ? 1u : 0u;
            bool have = false;
            if (HELP && help_seq) {
                // a helper's result for this block, out of the last two requests (help_seq: the one posted in the block before this)
                for (uint32_t it = 0; it < (1u << 22) && !have; ++it) {
                    bool working = false;
                    for (uint32_t h = 0; h < V2_NHELP && !have; ++h) {
                        for (uint32_t bq = 0; bq < V2_HBUF; ++bq) {
                            const uint32_t sl = help_addr + 4u * (VH_SLOT + 3u * (h * V2_HBUF + bq));
                            const uint32_t sq = v2_par(sl);
                            if (sq && sq + 1u >= help_seq && v2_par(sl + 4u) == Rb && v2_par(sl + 8u) == Cb) {
                                scp = &hscratch[(size_t(HELP ? blockIdx.x : 0u) * V2_NHELP + size_t(h)) * V2_HBUF + size_t(bq)];
                                have = true;
                                break;
                            }
                        }
                        const uint32_t wk = help_addr + 4u * (VH_WORK + 3u * h);
                        const uint32_t wq = v2_par(wk);
                        if (!have && wq && wq + 1u >= help_seq && v2_par(wk + 4u) == Rb && v2_par(wk + 8u) == Cb) working = true;
                    }
                    if (have || !working) break;
                    __builtin_amdgcn_s_sleep(4);
                }
                if (have) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    ++n_helped;
                }
            }
            if (!have) {
                scp = &scratch[pslot];
                const unsigned long long t_own0 = __builtin_amdgcn_s_memtime();
                const uint32_t bsteps = recompute_block(Rb, Cb, brows, bcols, *scp);  // (the steps it ran)
                const unsigned long long t_own1 = __builtin_amdgcn_s_memtime() - t_own0;
                n_bsteps += bsteps;
                n_bsteps_thin += bcols <= 64u ? bsteps : 0u;
                t_own += t_own1;
                t_own_thin_c += bcols <= 64u ? t_own1 : 0ull;
                t_own_thin_r += brows <= 64u ? t_own1 : 0ull;
            }
            if (HELP) {  // the blocks the walk can enter next: above and to the left of this one (entry point: the bounds of what they need)
                v2_lds_store(help_addr + 4u * VH_RB, Rb);
                v2_lds_store(help_addr + 4u * VH_CB, Cb);
                v2_lds_store(help_addr + 4u * VH_I, i);
                v2_lds_store(help_addr + 4u * VH_J, j);
                ++help_seq;
                v2_lds_store(help_addr + 4u * VH_SEQ, help_seq);
            }
            t_blk += __builtin_amdgcn_s_memtime() - t_blk0;
        }
        // ================= the tile (r0, c0) inside the block, as k_align_trace =================
        int cm = K.cm, cx = K.cx;
        asm volatile("" : "+v"(cm), "+v"(cx));
        const uint32_t kr = (r0 - Rb) / TILE, kc = (c0 - Cb) / TILE;
        ++n_tiles;
        const unsigned long long t_tile0 = __builtin_amdgcn_s_memtime();
        for (uint32_t x = lane; x < rows; x += 64) {
            const int2 v = v2_ld(&scp->fcol[kc][(r0 - Rb) + x]);
            s_rec[x] = TRec{v.x, v.y, q[r0 + x]};
        }
        const uint32_t jb = c0 + lane * TR_C;  // columns to the left of this lane's block
        uint32_t rpk[1];
        {
            uint32_t w = 0;
#pragma unroll
            for (int e = 0; e < TR_C; ++e) w |= ref_byte(r, m, pr.rc, jb + e) << (8 * e);
            rpk[0] = w;
        }
        if (TR_C == 4)
            reinterpret_cast<uint32_t*>(s_rb)[lane] = rpk[0];
        else
            reinterpret_cast<uint16_t*>(s_rb)[lane] = uint16_t(rpk[0]);
        uint32_t rb[TR_C];
#pragma unroll
        for (int c = 0; c < TR_C; ++c) rb[c] = (rpk[0] >> (8 * c)) & 0xFFu;
        int Hp[TR_C], F[TR_C];  // (Hq, F*) of the row above
        int dg;
        {
            const uint32_t x0 = (c0 - Cb) + lane * TR_C;  // entry of the column left of this lane's block
#pragma unroll
            for (int c = 0; c < TR_C; ++c) {
                int2 v{0, ALN_NEG};
                if (jb + c < m && x0 + c + 1 <= uint32_t(CK2)) v = v2_ld(&scp->frow[kr][x0 + c + 1]);
                Hp[c] = v.x;
                F[c] = v.y;
            }
            dg = x0 <= uint32_t(CK2) ? v2_ld(&scp->frow[kr][x0]).x : 0;
        }
        tr_wave_sync();
        const uint32_t nact = (cols + TR_C - 1) / TR_C;
        const uint32_t nsteps = rows + nact - 1;
        // Lane l has row s - l at step s: it works while l <= s < l + rows.  The loop is peeled by what that takes: lanes still
        // switching on (LO: l <= s is tested), all of them at work (nothing is), lanes switching off (HI: s - rows < l), and both
        // at once in a tile of fewer rows than lanes.  Lane 0's inputs of step s + 1 — one record — are read at step s (PRE) while
        // rows are left; the tile's last row and the steps behind it read nothing.  Every address is a pointer that runs along.
        if (lane < nact) {
            int out_h = 0, out_e = ALN_NEG;
            uint32_t out_q = 0;
            const TRec* rp = s_rec;
            TRec nrec = rp[0];
            uint8_t* dp = reinterpret_cast<uint8_t*>(&dirs[0][0]) + lane * uint32_t(TR_C / 2) - lane * (64u * uint32_t(TR_C / 2));  // (row s - lane, this lane's cells)
            auto tstep = [&](auto lo, auto hi, auto pre, const uint32_t s) __attribute__((always_inline)) {
                int hl = int(from_left_or(uint32_t(out_h), uint32_t(nrec.hq)));
                int el = int(from_left_or(uint32_t(out_e), uint32_t(nrec.e)));
                const uint32_t qc = from_left_or(out_q, nrec.q);
                if (decltype(pre)::value) nrec = rp[1];
                ++rp;
                bool act = true;
                if (decltype(lo)::value) act = lane <= s;
                if (decltype(hi)::value) act = act && int(lane) > int(s) - int(rows);
                if (act) {
                    const int hl_in = hl;
                    // a cell's nibble: 1 = not from the diagonal, 2 = nor from E (so from F), 4 = E extends, 8 = F extends; the cells
                    // of a lane from the top of the byte down.  Each bit is the sign of a difference whose operands are ordered
                    // (h >= hd, h >= E) or far from overflow (scores and ALN_NEG: |.| < 2^30), shifted in by one v_alignbit: no
                    // compare, no mask register, no select.
                    uint32_t acc = 0;
#pragma unroll
                    for (int c = 0; c < TR_C; ++c) {
                        const int E = max(el, hl);
                        const int Fn = max(F[c], Hp[c]);
                        const int hd = dg + (qc == rb[c] ? cm : cx);
                        // the host aligner's cell (ioc_align.cpp): H = diagonal, replaced by E if E > H, then by F if F > H
                        const int h = max(max(hd, E), Fn);
                        acc = __builtin_amdgcn_alignbit(acc, uint32_t(Hp[c]) - uint32_t(F[c]), 31);
                        acc = __builtin_amdgcn_alignbit(acc, uint32_t(hl) - uint32_t(el), 31);
                        acc = __builtin_amdgcn_alignbit(acc, uint32_t(E) - uint32_t(h), 31);
                        acc = __builtin_amdgcn_alignbit(acc, uint32_t(hd) - uint32_t(h), 31);
                        dg = Hp[c];
                        Hp[c] = h - gd;
                        F[c] = Fn;
                        hl = h - gd;
                        el = E;
                    }
                    dg = hl_in;
                    if (TR_C == 4)
                        *reinterpret_cast<uint16_t*>(dp) = uint16_t(acc);
                    else
                        *dp = uint8_t(acc);
                }
                dp += 64u * uint32_t(TR_C / 2);
                out_h = hl;
                out_e = el;
                out_q = qc;
            };
            auto run = [&](auto lo, auto hi, auto pre, uint32_t& s, const uint32_t end) __attribute__((always_inline)) {
                for (; s + 1u < end; s += 2) {
                    tstep(lo, hi, pre, s);
                    tstep(lo, hi, pre, s + 1u);
                }
                if (s < end) {
                    tstep(lo, hi, pre, s);
                    ++s;
                }
            };
            constexpr std::true_type yes{};
            constexpr std::false_type no{};
            uint32_t s = 0;
            run(yes, no, yes, s, min(nact, rows) - 1u);
            run(no, no, yes, s, rows - 1u);    // (rows > nact)
            run(yes, yes, no, s, nact - 1u);   // (rows < nact)
            run(no, yes, no, s, nsteps);
        }
        tr_wave_sync();
        const unsigned long long t_walk0 = __builtin_amdgcn_s_memtime();
        t_tile += t_walk0 - t_tile0;
        n_tsteps += nsteps;
        // the host aligner's traceback loop inside this tile (identical in every lane)
        auto nib = [&](uint32_t row, uint32_t col) {  // the nibble of the tile's cell (row, col), as the tile step packs it
            const uint32_t sh = 4u * (uint32_t(TR_C) - 1u - col % TR_C);
            return TR_C == 4 ? (uint32_t(dirs[row][col / TR_C]) >> sh) & 0xFu
                             : (uint32_t(reinterpret_cast<const uint8_t*>(&dirs[0][0])[row * 64u + col / TR_C]) >> sh) & 0xFu;
        };
        while (i > r0 && j > c0 && !decided) {
            const uint32_t cj = j - c0 - 1;
            const uint32_t ri = i - r0 - 1;
            if (state == 0) {
                const bool inr = i - r0 > lane && j - c0 > lane;
                uint32_t tl = 1u;
                bool mtl = false;
                if (inr) {
                    const uint32_t rl = ri - lane, cl = cj - lane;
                    tl = nib(rl, cl);
                    mtl = s_rec[rl].q == uint32_t(s_rb[cl]);  // (the tile step's own test: the query byte against ref_byte)
                }
                const bool dgl = inr && (tl & 1u) == 0u;
                const unsigned long long dm = __ballot(dgl);
                const uint32_t run = ~dm ? uint32_t(__builtin_ctzll(~dm)) : 64u;
                if (run > 0) {
                    const unsigned long long mb = __ballot(dgl && mtl) & (run == 64u ? ~0ull : ((1ull << run) - 1ull));
                    ws.push_run(mb, run, kmask, k, il, lane);
                    ops.run(mb, run, lane);
                    i -= run;
                    j -= run;
                } else {
                    state = (uint32_t(__builtin_amdgcn_readfirstlane(int(tl))) & 2u) ? 2 : 1;
                }
            } else {
                // a gap's steps at once: lane l looks at the l-th cell along the row (E, to the left) or the column (F, upwards); the
                // gap takes the cell the walk is in and goes on while the cells' extension bits say so — as far as the tile reaches
                const bool hor = state == 1;
                const uint32_t avail = min(hor ? cj + 1u : ri + 1u, 64u);
                bool ext = false;
                if (lane < avail) ext = (nib(hor ? ri : ri - lane, hor ? cj - lane : cj) & (hor ? 4u : 8u)) != 0u;
                const unsigned long long em = __ballot(ext);
                const uint32_t reach = ~em ? uint32_t(__builtin_ctzll(~em)) : 64u;  // (<= avail: the lanes beyond say no)
                const uint32_t g = reach < avail ? reach + 1u : avail;
                if (reach < avail) state = 0;  // (the cell that does not extend is the gap's first: H from here on)
                ws.push_run(0ull, g, kmask, k, il, lane);
                ops.fill(hor ? 'D' : 'I', g, lane);
                if (hor)
                    j -= g;
                else
                    i -= g;
                n_gapsteps += g;
            }
            decided = stop_at && (ws.cnt >= stop_at || cannot_reach(ws.cnt, i, j));
        }
        tr_wave_sync();
        t_walk += __builtin_amdgcn_s_memtime() - t_walk0;
    }
    if (HELP) v2_lds_store(help_addr + 4u * VH_QUIT, 1u);  // (the helpers leave)
    if (!decided) ws.blanks(i + j, kmask, k, il);  // leading end gaps
    if (EMIT) {  // (never decided early)
        ops.fill('d', j, lane);
        ops.fill('i', i, lane);
        ops.end(od, pid, lane);
    }
    if (lane == 0) {
        out_score[pid] = en.x;
        out_count[pid] = ws.cnt;
        // the pair's own scratch is free now: what the walk cost (read back by the host under IOC_V2_TRACE_TIMES only)
        const unsigned long long dt = __builtin_amdgcn_s_memtime() - t_begin;
        if (HELP) {  // (second launch: its own cycles and blocks behind the first launch's record)
            rs[12] = uint32_t(dt >> 8);
            rs[13] = n_blocks | (n_helped << 16);
            rs[14] = n_tiles;
            rs[15] = ws.cnt;
        } else {
            rs[8] = uint32_t(dt >> 8);
            rs[9] = n_blocks | (n_diag << 16);
            rs[10] = n_tiles;
            rs[11] = n_gapsteps;
            rs[15] = ws.cnt;
        }
        split_out();
    }
}

// Holds the first traceback launch back (it is queued behind this on its stream) until the workgroups of the helper launch for
// the wrong candidates — started a moment earlier on the side stream — have their places: a compute unit holds two traceback
// workgroups of either kind, and the helper workgroups that came second would wait for a first-launch workgroup to END.
// A bounded wait (~0.2 ms): nothing depends on it but the order of arrival.
__global__ void k_trace2_gate(const uint32_t* __restrict__ early, const uint32_t* __restrict__ gate, uint32_t grid)
{
    const uint32_t want = min(__hip_atomic_load(&early[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), grid);
    for (uint32_t it = 0; it < 4096u; ++it) {
        if (__hip_atomic_load(gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want) break;
        __builtin_amdgcn_s_sleep(8);
    }
}

// first launch: four pairs per workgroup, one wave each
#define V2_TRACE_ARGS                                                                                                                   \
    const AlnPairDev *__restrict__ pairs, const uint32_t *__restrict__ order, const uint8_t *__restrict__ pool, AlnParams P,             \
        const uint32_t *__restrict__ arena, const V2Couple *__restrict__ couples, const V2PairCk *__restrict__ pck,                      \
        const int4 *__restrict__ ends, V2Scratch *__restrict__ scratch, uint32_t *__restrict__ resume, uint32_t *__restrict__ park,      \
        uint32_t *__restrict__ split, int32_t *__restrict__ out_score, uint32_t *__restrict__ out_count, uint32_t count, uint32_t max_blocks,             \
        unsigned long long max_cycles
__global__ void __launch_bounds__(64 * TR_WAVES) k_trace2(V2_TRACE_ARGS)
{
    const uint32_t wv = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    trace2_body<false, false>(pairs, order, pool, P, arena, couples, pck, ends, scratch, nullptr, resume, park, split, out_score, out_count, count, max_blocks,
                              max_cycles, blockIdx.x * TR_WAVES + wv, wv, 0u, NoOpsDev{});
}
// ... emitting (ioc_align_pairs_ops)
__global__ void __launch_bounds__(64 * TR_WAVES) k_trace2_ops(V2_TRACE_ARGS, AlnOpsDev od)
{
    const uint32_t wv = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    trace2_body<false, true>(pairs, order, pool, P, arena, couples, pck, ends, scratch, nullptr, resume, park, split, out_score, out_count, count, max_blocks,
                             max_cycles, blockIdx.x * TR_WAVES + wv, wv, 0u, od);
}

// second launch: the parked walks (park[0] of them, listed behind it), one per workgroup of a walker and five helper waves; the
// grid is fixed (the host does not know the count), a workgroup takes every gridDim.x-th entry
#define V2_HELP_ARGS                                                                                                                    \
    const AlnPairDev *__restrict__ pairs, const uint32_t *__restrict__ order, const uint8_t *__restrict__ pool, AlnParams P,             \
        const uint32_t *__restrict__ arena, const V2Couple *__restrict__ couples, const V2PairCk *__restrict__ pck,                      \
        const int4 *__restrict__ ends, V2Scratch *__restrict__ scratch, V2Scratch *__restrict__ hscratch, uint32_t *__restrict__ resume, \
        uint32_t *__restrict__ park, uint32_t *__restrict__ split, int32_t *__restrict__ out_score, uint32_t *__restrict__ out_count,    \
        uint32_t count, uint32_t want, uint32_t *__restrict__ gate
__global__ void __launch_bounds__(64 * V2_HWAVES) k_trace2_help(V2_HELP_ARGS)
{
    const uint32_t wv = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    uint32_t n_parked = uint32_t(__builtin_amdgcn_readfirstlane(int(park[0])));
    if (want == 2u) n_parked = min(n_parked, gridDim.x);  // (k_fwd2_ends lists no more than one walk per workgroup)
    if (gate && threadIdx.x == 0) atomicAdd(gate, 1u);  // (this workgroup has its place on the chip: k_trace2_gate)
    for (uint32_t e = blockIdx.x; e < n_parked; e += gridDim.x) {
        const uint32_t pslot = uint32_t(__builtin_amdgcn_readfirstlane(int(park[1u + e])));
        trace2_body<true, false>(pairs, order, pool, P, arena, couples, pck, ends, scratch, hscratch, resume, park, split, out_score, out_count, count, 0u, 0ull, pslot, wv,
                                 want, NoOpsDev{});
        __syncthreads();  // (walker and helpers have left the pair: its LDS words are free)
    }
}
// ... emitting.  (An emitting call's pairs have no stop_at: nothing parks them and k_fwd2_ends routes none of them here, so this
// launch finds its lists empty today; it exists so that the emitting call's launches are the plain call's, whatever is routed where.)
__global__ void __launch_bounds__(64 * V2_HWAVES) k_trace2_help_ops(V2_HELP_ARGS, AlnOpsDev od)
{
    const uint32_t wv = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));
    uint32_t n_parked = uint32_t(__builtin_amdgcn_readfirstlane(int(park[0])));
    if (want == 2u) n_parked = min(n_parked, gridDim.x);
    if (gate && threadIdx.x == 0) atomicAdd(gate, 1u);
    for (uint32_t e = blockIdx.x; e < n_parked; e += gridDim.x) {
        const uint32_t pslot = uint32_t(__builtin_amdgcn_readfirstlane(int(park[1u + e])));
        trace2_body<true, true>(pairs, order, pool, P, arena, couples, pck, ends, scratch, hscratch, resume, park, split, out_score, out_count, count, 0u, 0ull, pslot, wv,
                                want, od);
        __syncthreads();
    }
}
