// ioc_window_variants.hip — two exons at one junction: the voters of a kept insertion site split in two where they are two exons,
// every read re-keyed and the isoforms counted again (ioc_planes_insert_window_variants; the definition is
// ioc_host_insert_window_variants, ioc_align.cpp).  Behind the kernels of ioc_insert_windows.hip, which are used unchanged: k_win_align
// runs round A and, over the far voters of the sites that reach it, round B.
//
//   k_win_agree         a wave per alignment of a round, a lane per template row in chunks of 64.  It reads the voter's base plane in
//                       the template's frame, as k_win_align left it, and the template's bytes: eq rows hold the template's channel,
//                       del rows IOC_ALLELE_DEL, every other row is an 'X' and the voter's bases that no row took are 'I'
//                       (winvar_plane_agreement) — the four counts of the alignment's bytes, so nothing is aligned or walked a second
//                       time.  The agreement and the NEAR flag go to the alignment's (pair, site) entry.
//   k_win_template_far  a wave per site: n_far by ballot and, where round B runs, the lower median of the far voters
//                       (win_lower_median, ioc_win_stage.h, k_win_template's ranking over another set).
//   k_win_decide        a wave per site over its members, 64 at a time: the counts by ballot, the decision, the record, and in a
//                       second pass the variant byte of every (pair, site) entry of the site.
//   k_win_rekey         a wave per pair, a lane per kept site: the state of key2 (winvar_state), key2 and mask2 by an OR over the wave.
//   k_winvar_support, k_winvar_isoforms, k_winvar_record
//                       key_support, key_isoform and key_tallies (ioc_read_stage.h) over (pre_key, key2) and (pre_mask, mask2).
// No atomics and no LDS: every output byte has one writer and is a function of the inputs alone.  Every plane byte, pool byte, entry
// and record is held against the sizes passed.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ioc_internal.h"
#include "ioc_ops_pileup.h"
#include "ioc_read_stage.h"
#include "ioc_wave.h"
#include "ioc_win_stage.h"
#include "ioc_window_variants.h"

namespace {

constexpr uint32_t WAVES = IOC_WINVAR_WAVES;
typedef unsigned long long u64;

__global__ void __launch_bounds__(64 * WAVES)
k_win_agree(const IocWinItem* __restrict__ items, const uint64_t* __restrict__ at, uint32_t n_items, const uint8_t* __restrict__ pool, uint64_t pool_bytes,
            const uint8_t* __restrict__ base_planes, uint64_t plane_bytes, int32_t* __restrict__ agree, uint8_t* __restrict__ flag, uint64_t n_entries,
            int32_t min_agree)
{
    const uint32_t lane = threadIdx.x & 63u, x = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (x >= n_items) return;  // (whole waves: there is no barrier below)
    const IocWinItem it = items[x];
    const uint64_t e = at[x];
    const uint32_t qlen = it.qlen, tlen = it.tlen;
    if (e >= n_entries || qlen < 1u || qlen > uint32_t(IOC_WIN_MAX) || tlen < 1u || tlen > uint32_t(IOC_WIN_MAX)) return;  // (what k_win_align left alone)
    if (it.t_off + tlen > pool_bytes || it.plane + tlen + 1u > plane_bytes) return;
    uint32_t eq = 0, del = 0;
    for (uint32_t j0 = 0; j0 < tlen; j0 += 64u) {
        const uint32_t j = j0 + lane;
        const bool row = j < tlen;
        const uint32_t b = row ? base_planes[it.plane + j] : uint32_t(IOC_ALLELE_NONE);
        const uint32_t t = row ? PileAcc::channel(pool[it.t_off + j]) : 0u;
        eq += uint32_t(__popcll(__ballot(row && b == t)));
        del += uint32_t(__popcll(__ballot(row && b == uint32_t(IOC_ALLELE_DEL))));
    }
    if (lane != 0u) return;
    // (a plane that is not this alignment's could have more rows that took a base than the voter has bases: no agreement then)
    const bool whole = tlen - del <= qlen;
    const int32_t a = whole ? winvar_plane_agreement(qlen, tlen, eq, del) : INT32_MIN;
    agree[e] = a;
    flag[e] = whole && winvar_near(a, qlen, tlen, min_agree) ? WINVAR_NEAR : WINVAR_FAR;
}

// what the kernels over a site know of it: its segment, its place among the segment's sites and the segment's members
struct SiteAt {
    uint32_t g, k, mb, me;
    bool ok;
};
__device__ __forceinline__ SiteAt site_at(const IocWinDev& w, u64 x)
{
    SiteAt s{0, 0, 0, 0, false};
    if (x >= w.n_sites) return s;
    s.g = uint32_t(w.site_seg[x]);
    if (s.g >= w.n_segs) return s;
    const u64 k64 = x - u64(w.site_off[s.g]);
    if (k64 >= u64(IOC_INSERTS_MAX) || k64 >= w.stride) return s;
    s.k = uint32_t(k64), s.mb = w.mem_off[s.g], s.me = w.mem_off[s.g + 1u], s.ok = true;
    return s;
}
// what lane holds of member m of a site's segment: its pair, its entry (n_slots: none), and its class and length at the site
struct SiteMember {
    uint32_t pair = 0xFFFFFFFFu, cls_len = 0;
    u64 entry = ~0ull;
};
__device__ __forceinline__ SiteMember site_member(const IocWinDev& w, const SiteAt& s, uint32_t m)
{
    SiteMember r;
    if (m >= s.me) return r;
    r.pair = w.members[m];
    const u64 at = u64(r.pair) * w.stride + s.k;
    if (r.pair < w.n_pairs && at < w.n_slots) r.entry = at, r.cls_len = w.slots[at].cls_len;
    return r;
}

__global__ void __launch_bounds__(64 * WAVES)
k_win_template_far(IocWinVarDev v, WinVarRule rule)
{
    const uint32_t lane = threadIdx.x & 63u;
    const u64 x = u64(blockIdx.x) * WAVES + (threadIdx.x >> 6);
    const SiteAt s = site_at(v.w, x);
    if (!s.ok) return;
    auto far = [&](uint32_t m, uint32_t& pair, uint32_t& len) {
        const SiteMember r = site_member(v.w, s, m);
        pair = r.pair, len = win_slot_len(r.cls_len);
        return r.entry < v.w.n_slots && win_slot_class(r.cls_len) == uint32_t(IOC_WIN_VOTER) && v.flag[r.entry] == WINVAR_FAR;
    };
    uint32_t n_far = 0;
    for (uint32_t m0 = s.mb; m0 < s.me; m0 += 64u) {
        uint32_t pair, len;
        n_far += uint32_t(__popcll(__ballot(far(m0 + lane, pair, len))));
    }
    const bool runs = winvar_round_b(rule, v.w.win[x].n_voters, n_far);  // (the same in every lane)
    const WinMedian t = win_lower_median(s.mb, s.me, runs ? n_far : 0u, far);
    if (lane == 0) v.var[x] = ioc_window_variant{0, t.pair, t.len, 0u, 0u, 0u, n_far, 0u};
}

__global__ void __launch_bounds__(64 * WAVES)
k_win_decide(IocWinVarDev v, WinVarRule rule)
{
    const uint32_t lane = threadIdx.x & 63u;
    const u64 x = u64(blockIdx.x) * WAVES + (threadIdx.x >> 6);
    const SiteAt s = site_at(v.w, x);
    if (!s.ok) return;
    const u64 round_b = v.w.n_slots;  // (where the flags of round B begin)
    uint32_t n_voters = 0, n_far = 0, n_b = 0;
    for (uint32_t m0 = s.mb; m0 < s.me; m0 += 64u) {
        const SiteMember r = site_member(v.w, s, m0 + lane);
        const bool votes = r.entry < v.w.n_slots && win_slot_class(r.cls_len) == uint32_t(IOC_WIN_VOTER);
        const bool is_far = votes && v.flag[r.entry] == WINVAR_FAR;
        n_voters += uint32_t(__popcll(__ballot(votes)));
        n_far += uint32_t(__popcll(__ballot(is_far)));
        n_b += uint32_t(__popcll(__ballot(is_far && v.flag[round_b + r.entry] == WINVAR_NEAR)));
    }
    const bool ran = winvar_round_b(rule, n_voters, n_far) && v.var[x].template_pair_b >= 0;
    if (!ran) n_b = 0;
    const bool split = ran && winvar_splits(rule, n_voters, n_far, n_b);
    for (uint32_t m0 = s.mb; m0 < s.me; m0 += 64u) {
        const SiteMember r = site_member(v.w, s, m0 + lane);
        if (r.entry >= v.w.n_slots) continue;  // (no ballot or shuffle below)
        v.variant[r.entry] = winvar_variant(win_slot_class(r.cls_len), split, v.flag[r.entry], v.flag[round_b + r.entry]);
    }
    if (lane == 0) {
        ioc_window_variant o = v.var[x];  // (template B and n_far are k_win_template_far's)
        o.split = split ? 1 : 0, o.n_a = split ? n_voters - n_far : n_voters, o.n_b = n_b, o.n_other = ran ? n_far - n_b : 0u, o.n_far = n_far, o.reserved = 0u;
        v.var[x] = o;
    }
}

__global__ void __launch_bounds__(64 * WAVES)
k_win_rekey(IocWinVarDev v, IocReadInsertsDev k)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= v.w.n_pairs) return;
    const uint32_t g = uint32_t(v.w.seg_of_pair[i]);
    if (g >= v.w.n_segs) return;
    const u64 sb = u64(v.w.site_off[g]), se = u64(v.w.site_off[g + 1u]), x = sb + lane, at = u64(i) * v.w.stride + lane;
    const u64 key1 = v.w.keys[i];
    u64 key = 0, mask = 0, mine = 0;  // (mine: the two bits of the lane's site, where it has one)
    if (x < se && x < v.w.n_sites && lane < uint32_t(IOC_INSERTS_MAX) && lane < v.w.stride && at < v.w.n_slots) {
        const uint32_t state = uint32_t(key1 >> (2u * lane)) & 3u;
        const uint32_t st = winvar_state(state, win_slot_class(v.w.slots[at].cls_len), v.var[x].split != 0, v.variant[at]);
        key = u64(st) << (2u * lane), mask = blocks_state_mask(lane, st), mine = 3ull << (2u * lane);
    }
    key = wave_or64(key), mask = wave_or64(mask), mine = wave_or64(mine);
    if (lane == 0) k.reads[i].key = key | (key1 & ~mine), k.mask[i] = mask;  // (what lies behind the segment's sites stays what it was)
}

__device__ __forceinline__ u64 full_mask(const IocWinDev& w, uint32_t g) { return blocks_full_mask(uint32_t(w.site_off[g + 1u] - w.site_off[g])); }

__global__ void __launch_bounds__(64 * WAVES)
k_winvar_support(IocWinDev w, IocReadInsertsDev k, uint32_t min_alt)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= k.n_pairs) return;
    const uint32_t g = uint32_t(k.seg_of_pair[i]);
    if (g >= k.n_segs) return;
    const uint8_t flags = key_support(k, i, g, full_mask(w, g), min_alt, lane);
    if (lane == 0) k.flags[i] = flags;
}

__global__ void __launch_bounds__(64 * WAVES)
k_winvar_isoforms(IocWinDev w, IocReadInsertsDev k)
{
    const uint32_t lane = threadIdx.x & 63u, i = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (i >= k.n_pairs) return;
    const uint32_t g = uint32_t(k.seg_of_pair[i]);
    if (g >= k.n_segs) return;
    const KeyIsoform r = key_isoform(k, i, g, full_mask(w, g), lane);
    if (lane == 0) k.reads[i].group = r.group, k.reads[i].how = r.how;
}

__global__ void __launch_bounds__(64 * WAVES)
k_winvar_record(IocWinVarDev v, IocReadInsertsDev k, ioc_variants_seg* __restrict__ seg_out)
{
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (g >= k.n_segs) return;
    const uint32_t mb = k.mem_off[g], me = k.mem_off[g + 1u];
    const u64 sb = u64(v.w.site_off[g]), se = u64(v.w.site_off[g + 1u]);
    const uint32_t ns = uint32_t(min(se - sb, u64(IOC_INSERTS_MAX)));
    const KeyTallies t = key_tallies(k, mb, me, 0u, lane);
    const uint32_t n_split = uint32_t(__popcll(__ballot(lane < ns && sb + lane < v.w.n_sites && v.var[sb + lane].split != 0)));
    if (lane == 0)
        seg_out[g] = ioc_variants_seg{int32_t(ns), int32_t(n_split), int32_t(t.groups), int32_t(me - mb), int32_t(t.how_n[IOC_ISO_DIRECT]),
                                      int32_t(t.how_n[IOC_ISO_ASSIGNED]), int32_t(t.how_n[IOC_ISO_RARE]), int32_t(t.how_n[IOC_ISO_AMBIGUOUS])};
}

dim3 grid(uint64_t items) { return dim3(uint32_t((items + WAVES - 1u) / WAVES)); }

}  // namespace

static_assert(sizeof(ioc_window_variant) == 32 && sizeof(ioc_read_variants) == 16 && sizeof(ioc_variants_seg) == 32, "the records are laid out as the header says");

hipError_t iock_win_agree(hipStream_t st, const IocWinItem* items, const uint64_t* at, uint32_t n_items, const uint8_t* pool, uint64_t pool_bytes,
                          const uint8_t* base_planes, uint64_t plane_bytes, int32_t* agree, uint8_t* flag, uint64_t n_entries, int32_t min_agree)
{
    if (n_items == 0) return hipSuccess;
    hipLaunchKernelGGL(k_win_agree, grid(n_items), dim3(64 * WAVES), 0, st, items, at, n_items, pool, pool_bytes, base_planes, plane_bytes, agree, flag, n_entries,
                       min_agree);
    return hipGetLastError();
}

hipError_t iock_win_template_far(hipStream_t st, const IocWinVarDev& v, const WinVarRule& rule)
{
    if (v.w.n_sites == 0) return hipSuccess;
    hipLaunchKernelGGL(k_win_template_far, grid(v.w.n_sites), dim3(64 * WAVES), 0, st, v, rule);
    return hipGetLastError();
}

hipError_t iock_win_decide_rekey(hipStream_t st, const IocWinVarDev& v, const WinVarRule& rule, const IocReadInsertsDev& k, ioc_variants_seg* seg_out,
                                 hipEvent_t* each)
{
    const dim3 block(64 * WAVES);
    int step = 0;
    auto mark = [&]() { if (each) (void)hipEventRecord(each[step++], st); };
    mark();
    if (v.w.n_sites) hipLaunchKernelGGL(k_win_decide, grid(v.w.n_sites), block, 0, st, v, rule);
    mark();
    if (v.w.n_pairs) hipLaunchKernelGGL(k_win_rekey, grid(v.w.n_pairs), block, 0, st, v, k);
    mark();
    if (k.n_pairs) hipLaunchKernelGGL(k_winvar_support, grid(k.n_pairs), block, 0, st, v.w, k, uint32_t(rule.min_alt));
    mark();
    if (k.n_pairs) hipLaunchKernelGGL(k_winvar_isoforms, grid(k.n_pairs), block, 0, st, v.w, k);
    mark();
    if (k.n_segs) hipLaunchKernelGGL(k_winvar_record, grid(k.n_segs), block, 0, st, v, k, seg_out);
    mark();
    return hipGetLastError();
}
