// ioc_align_trace.inc — version 1's traceback kernel, included by ioc_align_gpu.hip once per variant: ALN_TRACE_KERNEL names it,
// ALN_TRACE_EMIT (0 / 1) says whether the walk also writes its operation bytes (ioc_align_pairs_ops).  Two copies of the text
// rather than a template over a shared body: the non-emitting kernel is then compiled from the very tokens it always had, and its
// code stays what it was (a body function inlined into two kernels came out with other loop counters and another schedule).
__global__ void __launch_bounds__(64 * TR_WAVES)
ALN_TRACE_KERNEL(const AlnPairDev* __restrict__ pairs, const uint32_t* __restrict__ order, const uint8_t* __restrict__ pool,
                 AlnParams P, const int2* __restrict__ ck, const AlnCk* __restrict__ cko, const int4* __restrict__ ends,
                 int32_t* __restrict__ out_score, uint32_t* __restrict__ out_count, uint32_t count
#if ALN_TRACE_EMIT
                 ,
                 AlnOpsDev od
#endif
)
{
#if !ALN_TRACE_EMIT
    const NoOpsDev od{};
#endif
    // A workgroup is TR_WAVES = 4 independent waves, one pair each, with LDS of their own: a workgroup of four waves puts
    // one on every SIMD of its CU, whereas one-wave workgroups were seen three to a SIMD on some CUs (each of them then
    // half as fast: 14.5 against 7.6 ms) while other SIMDs held one.  No workgroup barrier anywhere: a wave only ever
    // reads what it wrote itself, in program order.
    __shared__ uint16_t dirs_all[TR_WAVES][TILE * TR_C / 4][64];  // TR_C nibbles per lane and row (TILE 128: used as bytes [row][lane])
    __shared__ int2 s_left_all[TR_WAVES][TILE];
    __shared__ uint32_t s_q_all[TR_WAVES][TILE];
    const uint32_t wv = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)));  // uniform: the pair's state stays in SGPRs
    const uint32_t pslot = blockIdx.x * TR_WAVES + wv;
    if (pslot >= count) return;
    uint16_t(*dirs)[64] = dirs_all[wv];
    int2* s_left = s_left_all[wv];
    uint32_t* s_q = s_q_all[wv];
    const uint32_t pid = order[pslot];
    const AlnPairDev pr = pairs[pid];
    const uint32_t n = pr.n, m = pr.m;
    const int go = pr.gap_open, il = pr.ilimit;
    const uint8_t* __restrict__ q = pool + pr.q_off;
    const uint8_t* __restrict__ r = pool + pr.r_off;
    const int2* __restrict__ rowck = ck + cko[pid].row_off;
    const int2* __restrict__ colck = ck + cko[pid].col_off;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t k = P.k, kmask = k >= 32 ? 0xFFFFFFFFu : ((1u << k) - 1u);
    const int4 en = ends[pid];
    uint32_t i = uint32_t(en.y), j = uint32_t(en.z);
    int state = 0;  // 0 = H, 1 = E, 2 = F
    WinStat ws;
    OpsOut<ALN_TRACE_EMIT != 0> ops;
    ops.begin(od, pid, n + m);
    ws.blanks((m - j) + (n - i), kmask, k, il);  // trailing end gaps are the tail of the string
    ops.fill('d', m - j, lane);
    ops.fill('i', n - i, lane);

    while (i > 0 && j > 0) {
        const uint32_t r0 = ((i - 1) / TILE) * TILE, c0 = ((j - 1) / TILE) * TILE;
        const uint32_t rows = i - r0, cols = j - c0;
        // The tile is recomputed on the forward pass's own SLANTED scores (see fwd_cells: X* = X + ge (i + j), Hq = H* - gd),
        // exactly as the checkpoints hold them: a gap extension costs nothing, an opening is already inside Hq, so a cell is
        // two max + max3 + add + sub, and every decision of the host aligner's cell is a comparison of the same operands
        // (E extended <=> E* > Hq of the left cell; H from the diagonal <=> H* equals it, which wins ties, else from E if
        // equal to E*, else from F) — 18 VALU per cell where the unslanted form took 24.  This kernel is bound by VALU
        // issue on the SIMDs that hold two of its waves.
        const int gd = go - P.gap_extend, ge = P.gap_extend;
        int cm = P.match + 2 * ge + gd, cx = P.mismatch + 2 * ge + gd;
        asm volatile("" : "+v"(cm), "+v"(cx));  // kept in VGPRs: the select below cannot take two scalars, and the compiler would copy them over in every step
        for (uint32_t x = lane; x < rows; x += 64) {
            s_q[x] = q[r0 + x];
            int2 le{ge * int(r0 + x + 1) - gd, ALN_NEG};  // column 0: H = 0, no gap to extend
            if (c0) le = colck[uint64_t(c0 / TILE - 1) * col_pitch(n) + r0 + x];  // (Hq, E*) as passed between lanes
            s_left[x] = le;
        }
        const uint32_t jb = c0 + lane * TR_C;  // columns to the left of this lane's block
        uint32_t rpk[1];
        {
            uint32_t w = 0;
#pragma unroll
            for (int e = 0; e < TR_C; ++e) w |= ref_byte(r, m, pr.rc, jb + e) << (8 * e);
            rpk[0] = w;
        }
        int Hp[TR_C], F[TR_C];  // (Hq, F*) of the row above
        int dg = ge * int(r0 + jb) - gd;  // Hq(r0, jb) where H = 0: row 0, or column 0
        if (r0 == 0) {
#pragma unroll
            for (int c = 0; c < TR_C; ++c) {
                Hp[c] = ge * int(jb + c + 1) - gd;
                F[c] = ALN_NEG;
            }
        } else {
            const int* roh = reinterpret_cast<const int*>(rowck + uint64_t(r0 / TILE - 1) * row_pitch(m));
            const int* rof = roh + row_pitch(m);
#pragma unroll
            for (int c = 0; c < TR_C; ++c) {
                int2 v{0, ALN_NEG};
                if (jb + c < m) v = int2{roh[jb + c], rof[jb + c]};
                Hp[c] = v.x;
                F[c] = v.y;
            }
            if (jb > 0 && jb <= m) dg = roh[jb - 1];
        }
        tr_wave_sync();
        const uint32_t nact = (cols + TR_C - 1) / TR_C;
        const uint32_t nsteps = rows + nact - 1;
        int out_h = 0, out_e = ALN_NEG;
        uint32_t out_q = 0;
        // lane 0's inputs of a step (left edge and query byte of row s) are read one step AHEAD, by every lane at one address,
        // and enter the wave as the `old` operand of the shifts
        int2 nle = s_left[0];
        uint32_t nq = s_q[0];
        auto tstep = [&](const uint32_t s) __attribute__((always_inline)) {
            int hl = int(from_left_or(uint32_t(out_h), uint32_t(nle.x)));
            int el = int(from_left_or(uint32_t(out_e), uint32_t(nle.y)));
            uint32_t qc = from_left_or(out_q, nq);
            {
                const uint32_t sn = s + 1u < rows ? s + 1u : rows - 1u;  // (rows past the end are never looked at)
                nle = s_left[sn];
                nq = s_q[sn];
            }
            const int ri = int(s) - int(lane);
            if (ri >= 0 && uint32_t(ri) < rows && lane < nact) {
                const int hl_in = hl;
                uint32_t bits = 0;
#pragma unroll
                for (int c = 0; c < TR_C; ++c) {
                    const bool ex = el > hl;
                    const int E = max(el, hl);
                    const bool fx = F[c] > Hp[c];
                    const int Fn = max(F[c], Hp[c]);
                    const bool mt = qc == ((rpk[0] >> (8 * c)) & 0xFFu);
                    const int hd = dg + (mt ? cm : cx);
                    const int h = max(max(hd, E), Fn);
                    // the host aligner's cell (ioc_align.cpp): H = diagonal, replaced by E if E > H, then by F if F > H
                    const uint32_t from = h == hd ? (mt ? 0u : 3u << (4 * c)) : (h == E ? 1u << (4 * c) : 2u << (4 * c));
                    bits |= from | (ex ? 4u << (4 * c) : 0u) | (fx ? 8u << (4 * c) : 0u);
                    dg = Hp[c];
                    Hp[c] = h - gd;
                    F[c] = Fn;
                    hl = h - gd;
                    el = E;
                }
                dg = hl_in;
                if (TR_C == 4)
                    dirs[ri][lane] = uint16_t(bits);
                else
                    reinterpret_cast<uint8_t*>(&dirs[0][0])[uint32_t(ri) * 64u + lane] = uint8_t(bits);  // (TILE 128: a byte per lane and row, row-major)
            }
            out_h = hl;
            out_e = el;
            out_q = qc;
        };
        {   // two steps per iteration (the compiler does not unroll a loop with wave-level operations): fewer register copies
            uint32_t s = 0;
#if IOC_TR_STEP_UNROLL == 4
            for (; s + 3u < nsteps; s += 4) {
                tstep(s);
                tstep(s + 1u);
                tstep(s + 2u);
                tstep(s + 3u);
            }
#endif
            for (; s + 1u < nsteps; s += 2) {
                tstep(s);
                tstep(s + 1u);
            }
            if (s < nsteps) tstep(s);
        }
        tr_wave_sync();
        // the host aligner's traceback loop inside this tile (identical in every lane)
        while (i > r0 && j > c0) {
            const uint32_t cj = j - c0 - 1;
            const uint32_t ri = i - r0 - 1;
            const uint32_t t = TR_C == 4 ? (uint32_t(dirs[ri][cj / TR_C]) >> (4 * (cj % TR_C))) & 0xFu
                                         : (uint32_t(reinterpret_cast<const uint8_t*>(&dirs[0][0])[ri * 64u + cj / TR_C]) >> (4 * (cj % TR_C))) & 0xFu;
            if (state == 0) {
                // look ahead along the diagonal: lane l reads the cell l steps up-left; the run of diagonal moves
                // from here on goes into the window counter at once
                const bool inr = i - r0 > lane && j - c0 > lane;
                uint32_t tl = 1u;
                if (inr) {
                    const uint32_t rl = ri - lane, cl = cj - lane;
                    tl = (TR_C == 4 ? (uint32_t(dirs[rl][cl / TR_C]) >> (4 * (cl % TR_C)))
                                    : (uint32_t(reinterpret_cast<const uint8_t*>(&dirs[0][0])[rl * 64u + cl / TR_C]) >> (4 * (cl % TR_C)))) & 3u;
                }
                const bool dgl = inr && (tl == 0u || tl == 3u);
                const unsigned long long dm = __ballot(dgl);
                const uint32_t run = ~dm ? uint32_t(__builtin_ctzll(~dm)) : 64u;
                if (run > 0) {
                    const unsigned long long mb = __ballot(dgl && tl == 0u) & (run == 64u ? ~0ull : ((1ull << run) - 1ull));
                    ws.push_run(mb, run, kmask, k, il, lane);
                    ops.run(mb, run, lane);
                    i -= run;
                    j -= run;
                } else {
                    state = (t & 3u) == 1u ? 1 : 2;
                }
            } else if (state == 1) {
                ws.push(0u, kmask, k, il);
                ops.step('D', lane);
                if (!(t & 4u)) state = 0;
                --j;
            } else {
                ws.push(0u, kmask, k, il);
                ops.step('I', lane);
                if (!(t & 8u)) state = 0;
                --i;
            }
        }
        tr_wave_sync();
    }
    ws.blanks(i + j, kmask, k, il);  // leading end gaps
    ops.fill('d', j, lane);
    ops.fill('i', i, lane);
    ops.end(od, pid, lane);
    if (lane == 0) {
        out_score[pid] = en.x;
        out_count[pid] = ws.cnt;
    }
}
