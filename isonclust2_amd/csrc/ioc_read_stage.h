// ioc_read_stage.h — the bodies that the three read stages over bit planes share (ioc_read_blocks.hip, ioc_read_inserts.hip,
// ioc_read_ends.hip; the key functions serve ioc_window_variants.hip as well, over key2), each written once: the words of a segment, the windowed sum of 128 counts, the sweep that lists the runs of
// a plane into slots, the per-row counts over a segment's members, the masked popcounts of a slot's rows, and the keys of blocks
// and inserts — support, rank, isoform and the record's tallies.  Device code only.  A function here takes values and pointers, or
// the stage's view where the fields it reads have the same names in both; none takes a flag that says which stage is calling.
// The __global__ kernels stay in their files: guard lines, one call, the store of the stage's own record.
//
// A wave per item, nothing shared between waves: no LDS and no barrier, and every lane of the wave takes every step of a function
// here that has a ballot or a shuffle in it (all but seg_words and masked_counts).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "ioc_internal.h"
#include "ioc_read_inserts.h"
#include "ioc_wave.h"

__device__ __forceinline__ uint32_t seg_words(const IocPileSeg& s) { return uint32_t(s.rlen) / 64u + 1u; }  // ceil((rlen + 1) / 64)

// W(p0 + lane) of counts of which the lane holds own = the one at p0 + lane and halo = the one at p0 - 32 + lane (lanes 0 .. 31) or
// p0 + 32 + lane (lanes 32 .. 63), 0 outside rows 0 .. rlen so that the window needs no clamping.  A[0 .. 128) = the 32 below p0,
// the 64 from p0 on, the 32 behind them; sV and sH are the inclusive prefix sums of the middle and of the halo, and the inclusive
// prefix of A at idx is sH[idx], sH[31] + sV[idx - 32] or sV[63] + sH[idx - 64].  W = prefix(32 + lane + slack) - prefix(32 + lane -
// slack - 1); slack <= 32 keeps both inside -1 .. 127.
__device__ __forceinline__ uint32_t window_sums(uint32_t own, uint32_t halo, uint32_t slack, uint32_t lane)
{
    const uint32_t sV = wave_scan_incl(own, lane), sH = wave_scan_incl(halo, lane);
    const uint32_t left = shfl32(sH, 31u), mid = shfl32(sV, 63u);
    auto prefix = [&](int idx) -> uint32_t {
        const uint32_t fromH = shfl32(sH, uint32_t(idx < 32 ? idx : idx - 64) & 63u), fromV = shfl32(sV, uint32_t(idx - 32) & 63u);
        return idx < 0 ? 0u : idx < 32 ? fromH : idx < 96 ? left + fromV : mid + fromH;
    };
    const uint32_t hi = prefix(int(32u + lane + slack)), lo = prefix(int(32u + lane) - int(slack) - 1);
    return hi - lo;
}

// ---- runs into slots ----
// The runs of a plane are listed in ascending order: the k-th start and the k-th end are slot k's .first and .end (Slot: any
// record with these two).  One batch of 64 words, lane w word w whose first row is `row`: st / en are the lane's start and end bits
// (run_starts / run_ends, ioc_read_blocks.h); ranks by a wave scan and the running bases base_s / base_e, the starts and the ends
// below the batch.  Only the first `most` are written, and nothing outside the n_slots slots that `slots` has.
template <class Slot>
__device__ __forceinline__ void run_slots_put(unsigned long long st, unsigned long long en, uint32_t row, uint32_t lane, uint32_t& base_s, uint32_t& base_e,
                                              Slot* slots, unsigned long long sb, unsigned long long n_slots, uint32_t most)
{
    const uint32_t ns = uint32_t(__popcll(st)), ne = uint32_t(__popcll(en));
    const uint32_t is = wave_scan_incl(ns, lane), ie = wave_scan_incl(ne, lane);
    for (uint32_t k = base_s + is - ns; st && k < most; ++k, st &= st - 1ull)
        if (sb + k < n_slots) slots[sb + k].first = int32_t(row + uint32_t(__builtin_ctzll(st)));
    for (uint32_t k = base_e + ie - ne; en && k < most; ++k, en &= en - 1ull)
        if (sb + k < n_slots) slots[sb + k].end = int32_t(row + uint32_t(__builtin_ctzll(en)) + 1u);
    base_s += shfl32(is, 63), base_e += shfl32(ie, 63);
}

// The sweep for runs of any length over the W words from words[at] on (n_words: what the buffer holds): a run goes on across a
// word where the neighbour's edge bit is set, which comes by shuffle, across a batch by a carried bit and one word read ahead.
// Returns how many runs there are; the first `most` are in the slots from sb on.  (The sweep for runs of a least length is RunSweep,
// ioc_read_blocks.hip: at least = 1 it finds the same and loads more.)
template <class Slot>
__device__ __forceinline__ uint32_t run_list_any(const unsigned long long* words, unsigned long long at, unsigned long long n_words, uint32_t W, uint32_t lane,
                                                 Slot* slots, unsigned long long sb, unsigned long long n_slots, uint32_t most)
{
    auto load = [&](uint32_t i) -> unsigned long long { return i < W && at + i < n_words ? words[at + i] : 0ull; };
    uint32_t base_s = 0, base_e = 0;
    unsigned long long top = 0;  // whether the row right below the batch is set
    for (uint32_t b0 = 0; b0 < W; b0 += 64u) {
        const unsigned long long w = load(b0 + lane);
        const unsigned long long dn = shfl64(w, (lane + 63u) & 63u), up = shfl64(w, (lane + 1u) & 63u);
        const uint32_t left = uint32_t(lane ? dn >> 63 : top), right = uint32_t((lane < 63u ? up : load(b0 + 64u)) & 1ull);
        run_slots_put(run_starts(w, left), run_ends(w, right), (b0 + lane) * 64u, lane, base_s, base_e, slots, sb, n_slots, most);
        top = shfl64(w, 63u) >> 63;
    }
    return base_s;
}

// ---- a segment's members over two planes ----
// Word c of segment g's members in the planes a and b of per-pair words (pair i's from pair_word[i] on), the members 64 at a time:
// lane j fetches member j's two words, and row by row a ballot counts the members that have the row's bit.  Lane r keeps row r's
// two counts: .x of plane a, .y of plane b.  View: n_pairs, mem_off, members, pair_word, n_pair_words.
template <class View>
__device__ __forceinline__ uint2 member_row_counts(const View& v, uint32_t g, unsigned long long c, const unsigned long long* a, const unsigned long long* b,
                                                   uint32_t lane)
{
    uint32_t na = 0, nb = 0;
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u];
    for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
        unsigned long long aw = 0, bw = 0;
        if (m0 + lane < me) {
            const uint32_t i = v.members[m0 + lane];
            const unsigned long long w = i < v.n_pairs ? v.pair_word[i] + c : v.n_pair_words;
            if (w < v.n_pair_words) aw = a[w], bw = b[w];
        }
        for (uint32_t r = 0; r < 64u; ++r) {  // (row r of the chunk: how many of the 64 members have its bit; lane r keeps the sum)
            const uint32_t x = uint32_t(__popcll(__ballot((aw >> r) & 1ull))), y = uint32_t(__popcll(__ballot((bw >> r) & 1ull)));
            if (lane == r) na += x, nb += y;
        }
    }
    return make_uint2(na, nb);
}

// how many bits of rows [first, end) a pair has in the planes a (.x) and b (.y): its W words lie from w0 on, n_words in the planes
__device__ __forceinline__ uint2 masked_counts(const unsigned long long* a, const unsigned long long* b, unsigned long long w0, unsigned long long n_words,
                                               uint32_t W, long long first, long long end)
{
    uint32_t c = 0, s = 0;
    for (long long w = first / 64; w * 64 < end && w < (long long)W; ++w) {
        const unsigned long long m = run_row_mask(w * 64, first, end);
        if (w0 + (unsigned long long)w < n_words) c += uint32_t(__popcll(a[w0 + (unsigned long long)w] & m)), s += uint32_t(__popcll(b[w0 + (unsigned long long)w] & m));
    }
    return make_uint2(c, s);
}

// how many lanes have `hit`, and how many of those `before`, added to the two running counts
__device__ __forceinline__ void tally_hits(bool hit, bool before, uint32_t& same, uint32_t& earlier)
{
    same += uint32_t(__popcll(__ballot(hit)));
    earlier += uint32_t(__popcll(__ballot(hit && before)));
}

// ---- keys ----
// A read's key is two words, the major one (`pre`) and the stage's own, each with its mask; complete is a read whose masks are the
// segment's full ones.  The insert stage has the block stage's word as its major one (and none where the pointer is NULL); the block
// stage has no major word: there every `pre` below is the constant 0 and what is done with it compiles away, loads first of all.
// View: n_pairs, mem_off, members, reads[].key / .group / .how, mask, flags.
template <class View> inline constexpr bool two_word_keys = std::is_same<View, IocReadInsertsDev>::value;

template <class View>
__device__ __forceinline__ unsigned long long pre_key_of(const View& v, uint32_t i)
{
    if constexpr (two_word_keys<View>) return v.pre_key ? v.pre_key[(unsigned long long)i * v.pre_key_stride] : 0ull;
    else return 0ull;
}
template <class View>
__device__ __forceinline__ unsigned long long pre_mask_of(const View& v, uint32_t i)
{
    if constexpr (two_word_keys<View>) return v.pre_mask ? v.pre_mask[(unsigned long long)i * v.pre_mask_stride] : 0ull;
    else return 0ull;
}
template <class View>
__device__ __forceinline__ unsigned long long pre_full_of(const View& v, uint32_t g)
{
    if constexpr (two_word_keys<View>) return v.pre_full ? v.pre_full[g] : 0ull;
    else return 0ull;
}

// what a wave reads of member m of its segment (lane's member of a chunk): the pair, both words of its key and of its mask, its flags
struct Member {
    uint32_t pair = 0xFFFFFFFFu;
    unsigned long long pre = 0, key = 0, pre_mask = 0, mask = 0;
    uint32_t flags = 0;
    bool there = false;
};
template <class View>
__device__ __forceinline__ Member member_at(const View& v, uint32_t m, uint32_t me, bool with_flags)
{
    Member x;
    if (m >= me) return x;
    x.pair = v.members[m];
    if (x.pair >= v.n_pairs) return x;
    x.there = true, x.key = v.reads[x.pair].key, x.mask = v.mask[x.pair], x.pre = pre_key_of(v, x.pair), x.pre_mask = pre_mask_of(v, x.pair);
    if (with_flags) x.flags = v.flags[x.pair];
    return x;
}

enum : uint32_t { KEY_SUPPORTED = 1, KEY_FIRST = 2 };

// Read i of segment g, lanes over the segment's reads: the flags of its key — supported where the read is complete and at least
// min_alt complete reads carry the key, and first where none of them comes before it.  `full`: the full mask of the stage's word.
template <class View>
__device__ __forceinline__ uint8_t key_support(const View& v, uint32_t i, uint32_t g, unsigned long long full, uint32_t min_alt, uint32_t lane)
{
    const unsigned long long pre_full = pre_full_of(v, g), key = v.reads[i].key, pre = pre_key_of(v, i);
    const bool complete = v.mask[i] == full && pre_mask_of(v, i) == pre_full;
    uint32_t same = 0, earlier = 0;
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u];
    for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
        const Member x = member_at(v, m0 + lane, me, false);
        const bool hit = x.there && x.mask == full && x.pre_mask == pre_full && x.key == key && x.pre == pre;
        tally_hits(hit, x.pair < i, same, earlier);  // (a segment's reads are its pairs in ascending order)
    }
    return uint8_t(complete && same >= min_alt ? KEY_SUPPORTED | (earlier == 0u ? KEY_FIRST : 0u) : 0u);
}

// the rank of (pre, key) among the first occurrences of the supported keys of the segment: the isoform's number
template <class View>
__device__ __forceinline__ uint32_t key_rank(const View& v, uint32_t mb, uint32_t me, unsigned long long pre, unsigned long long key, uint32_t lane)
{
    uint32_t rank = 0;
    for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
        const Member x = member_at(v, m0 + lane, me, true);
        rank += uint32_t(__popcll(__ballot(x.there && (x.flags & KEY_FIRST) && inserts_key_less(x.pre, x.key, pre, key))));  // (unsigned, major word first)
    }
    return rank;
}

// Read i of segment g: its key's rank among the first occurrences of supported keys or, incomplete, the supported keys that agree
// with it under its masks and the rank of the single one.
struct KeyIsoform { int32_t group, how; };
template <class View>
__device__ __forceinline__ KeyIsoform key_isoform(const View& v, uint32_t i, uint32_t g, unsigned long long full, uint32_t lane)
{
    const unsigned long long key = v.reads[i].key, mask = v.mask[i], pre = pre_key_of(v, i), pre_mask = pre_mask_of(v, i);
    const uint32_t mb = v.mem_off[g], me = v.mem_off[g + 1u];
    KeyIsoform r{-1, 0};
    if (mask == full && pre_mask == pre_full_of(v, g)) {  // (uniform over the wave, like everything it branches on below)
        r.how = (v.flags[i] & KEY_SUPPORTED) ? IOC_ISO_DIRECT : IOC_ISO_RARE;
        if (r.how == IOC_ISO_DIRECT) r.group = int32_t(key_rank(v, mb, me, pre, key, lane));
    } else {
        uint32_t agreeing = 0;
        unsigned long long which_pre = 0, which_key = 0;
        for (uint32_t m0 = mb; m0 < me && (mask | pre_mask) != 0ull; m0 += 64u) {
            const Member x = member_at(v, m0 + lane, me, true);
            const unsigned long long hits = __ballot(x.there && (x.flags & KEY_FIRST) && inserts_key_agrees(pre, key, x.pre, x.key, pre_mask, mask));
            if (hits && agreeing == 0u) {
                which_key = shfl64(x.key, uint32_t(__builtin_ctzll(hits)));
                if constexpr (two_word_keys<View>) which_pre = shfl64(x.pre, uint32_t(__builtin_ctzll(hits)));
            }
            agreeing += uint32_t(__popcll(hits));
        }
        r.how = agreeing == 1u ? IOC_ISO_ASSIGNED : IOC_ISO_AMBIGUOUS;
        if (agreeing == 1u) r.group = int32_t(key_rank(v, mb, me, which_pre, which_key, lane));
    }
    return r;
}

// Segment g's record: the groups, the reads by how they came to theirs, and — lane b, for the n_kept slots the stage's word has
// states of — how many reads are in each of the four states at slot b.
struct KeyTallies { uint32_t groups = 0, how_n[4] = {0, 0, 0, 0}, state_n[4] = {0, 0, 0, 0}; };
template <class View>
__device__ __forceinline__ KeyTallies key_tallies(const View& v, uint32_t mb, uint32_t me, uint32_t n_kept, uint32_t lane)
{
    KeyTallies t;
    for (uint32_t m0 = mb; m0 < me; m0 += 64u) {
        const Member x = member_at(v, m0 + lane, me, true);
        const uint32_t how = x.there ? uint32_t(v.reads[x.pair].how) : 4u;
        t.groups += uint32_t(__popcll(__ballot(x.there && (x.flags & KEY_FIRST))));
#pragma unroll
        for (uint32_t h = 0; h < 4u; ++h) t.how_n[h] += uint32_t(__popcll(__ballot(how == h)));
        for (uint32_t b = 0; b < n_kept; ++b) {  // (slot b: how many of the 64 members are in each state; lane b keeps the sums)
            const uint32_t st = uint32_t(x.key >> (2u * b)) & 3u;
#pragma unroll
            for (uint32_t h = 0; h < 4u; ++h) {
                const uint32_t n = uint32_t(__popcll(__ballot(x.there && st == h)));
                if (lane == b) t.state_n[h] += n;
            }
        }
    }
    return t;
}
