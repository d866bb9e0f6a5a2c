// ioc_sink_plan.h — what the sink entry points (ioc_align_sinks.cpp) work out on the host before anything is launched: where the
// blocks of a device arena lie, which pairs a segment has, the split's tables, the bounds, and the segments and pairs of a call
// with everything a call refuses about them.  No HIP header and no ioc_ctx: tools/align_sink_check.cpp drives all of it on the CPU.
#ifndef IOC_SINK_PLAN_H
#define IOC_SINK_PLAN_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

#include "isonclust2_hip.h"

// A segment of the call and site kernels (ioc_pile_call.hip, ioc_pile_sites.hip, ioc_plane_pile.hip): rlen + 1 rows of the tables
// from row0 on, its frame rlen bytes at f_off of a pool of sequences, read reverse-complemented where rc is set.
struct IocPileSeg {
    int64_t row0, f_off;
    int32_t rlen, rc;
};

#pragma GCC visibility push(hidden)  // (internal to the library)

// The blocks of one device buffer, one behind the other, each starting at a multiple of 16: take(bytes) is where the next one
// lies, size() what the buffer has to hold.  A block of 0 bytes takes no room.
struct Arena {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t o = at; at += (bytes + 15) & ~size_t(15); return o; }
    size_t size() const { return at; }
};

// A segment's reads are its pairs in ascending order: segment g has members[mem_off[g] .. mem_off[g + 1]).
struct MemberLists { std::vector<uint32_t> mem_off, members; };
inline MemberLists member_lists(size_t n_segs, size_t n_pairs, const int32_t* seg_of_pair)
{
    MemberLists m{std::vector<uint32_t>(n_segs + 1, 0), std::vector<uint32_t>(n_pairs)};
    for (size_t i = 0; i < n_pairs; ++i) ++m.mem_off[size_t(seg_of_pair[i]) + 1];
    for (size_t g = 0; g < n_segs; ++g) m.mem_off[g + 1] += m.mem_off[g];
    std::vector<uint32_t> next(m.mem_off.begin(), m.mem_off.end() - 1);
    for (size_t i = 0; i < n_pairs; ++i) m.members[next[size_t(seg_of_pair[i])]++] = uint32_t(i);
    return m;
}

// The same per group.  Segment g has n_groups[g] groups and pair i is in group group[i] of its segment, or in none (-1, or a group
// the segment does not have: a call that cuts the groups short leaves the reads of the later ones in no list).  The group-segments
// are numbered in segment order, segment g's gseg_off[g] .. gseg_off[g + 1] (G = gseg_off[n_segs] in all), and group-segment x has
// gmembers[gmem_off[x] .. gmem_off[x + 1]), its pairs in ascending order; a group without reads has an empty list.  The caller has
// checked that every n_groups[g] is at least 0 and that G is at most 2^31 - 1.
struct GroupMemberLists { std::vector<uint32_t> gseg_off, gmem_off, gmembers; };
inline GroupMemberLists group_member_lists(size_t n_segs, size_t n_pairs, const int32_t* seg_of_pair, const int32_t* group, const int32_t* n_groups)
{
    GroupMemberLists m;
    m.gseg_off.assign(n_segs + 1, 0);
    for (size_t g = 0; g < n_segs; ++g) m.gseg_off[g + 1] = m.gseg_off[g] + uint32_t(n_groups[g]);
    const size_t G = m.gseg_off[n_segs];
    auto gseg_of = [&](size_t i) -> int64_t {
        const size_t g = size_t(seg_of_pair[i]);
        return group[i] >= 0 && group[i] < n_groups[g] ? int64_t(m.gseg_off[g]) + group[i] : -1;
    };
    m.gmem_off.assign(G + 1, 0);
    for (size_t i = 0; i < n_pairs; ++i)
        if (const int64_t x = gseg_of(i); x >= 0) ++m.gmem_off[size_t(x) + 1];
    for (size_t x = 0; x < G; ++x) m.gmem_off[x + 1] += m.gmem_off[x];
    m.gmembers = std::vector<uint32_t>(m.gmem_off[G]);
    std::vector<uint32_t> next(m.gmem_off.begin(), m.gmem_off.end() - 1);
    for (size_t i = 0; i < n_pairs; ++i)
        if (const int64_t x = gseg_of(i); x >= 0) m.gmembers[next[size_t(x)]++] = uint32_t(i);
    return m;
}

// The host lists of the block family (the calls that pile, search exon blocks and go on from there), each written once.
// How many pairs every segment has.
inline std::vector<int64_t> reads_per_seg(size_t n_segs, size_t n_pairs, const int32_t* seg_of_pair)
{
    std::vector<int64_t> reads(n_segs, 0);
    for (size_t i = 0; i < n_pairs; ++i) ++reads[size_t(seg_of_pair[i])];
    return reads;
}

// The isoform cut: of the found[g] isoforms a search counted in segment g the first min(found[g], max_iso) are kept, n_iso[g] of
// them, segment g's in iso_off[g] .. iso_off[g + 1] of the call's isoforms (iso_off[0] is the caller's 0).  A segment has at most as
// many isoforms as reads, every isoform having min_alt >= 1 reads of its own: a count outside 0 .. reads[g] is refused with
// IOC_ERR_HIP and msg set, `search` naming the stage that counted ("block", "insert").
struct IsoCut {
    std::vector<int32_t> n_iso;
    std::string msg;
    int from(const std::string& search, size_t n_segs, const int32_t* found, const int64_t* reads, int32_t max_iso, int64_t* iso_off)
    {
        n_iso.assign(n_segs, 0);
        for (size_t g = 0; g < n_segs; ++g) {
            if (found[g] < 0 || found[g] > reads[g]) return msg = "the " + search + " search returned more isoforms than reads", IOC_ERR_HIP;
            n_iso[g] = std::min(found[g], max_iso);
            iso_off[g + 1] = iso_off[g] + n_iso[g];
        }
        return IOC_OK;
    }
};

// The key of every kept isoform: that of its lowest-numbered IOC_ISO_DIRECT read, 0 where it has none.  A read in group -1 or in an
// isoform behind the cut speaks for none (and is in no list: group_member_lists).
inline std::vector<uint64_t> iso_keys(size_t n_pairs, const int32_t* seg_of_pair, const ioc_read_variants* reads, const int32_t* n_iso, const int64_t* iso_off, size_t n_segs)
{
    std::vector<uint64_t> key(n_segs ? size_t(iso_off[n_segs]) : 0, 0);
    std::vector<uint8_t> has(key.size(), 0);
    for (size_t i = 0; i < n_pairs; ++i) {
        const int32_t g = seg_of_pair[i], h = reads[i].group;
        if (h < 0 || h >= n_iso[g] || reads[i].how != IOC_ISO_DIRECT || has[size_t(iso_off[g] + h)]) continue;
        key[size_t(iso_off[g] + h)] = reads[i].key2, has[size_t(iso_off[g] + h)] = 1;
    }
    return key;
}

// The mask of a key of n states (n <= 32): both bits of every block, or site, at which the state is not IOC_BLOCK_NONE — the
// blocks_state_mask (ioc_read_blocks.h) of every state, which tools/align_sink_check.cpp holds it against.
inline uint64_t blocks_key_mask(uint64_t key, uint32_t n)
{
    uint64_t mask = 0;
    for (uint32_t b = 0; b < n; ++b)
        if (((key >> (2u * b)) & 3u) != uint64_t(IOC_BLOCK_NONE)) mask |= uint64_t(3) << (2u * b);
    return mask;
}

// The word of every segment an insert search takes from the block stage: the mask of a complete read of its n_blocks blocks
// (blocks_full_mask, ioc_read_blocks.h, likewise held against it).
inline std::vector<uint64_t> blocks_pre_full(size_t n_segs, const ioc_blocks_seg* seg)
{
    std::vector<uint64_t> full(n_segs, 0);
    for (size_t g = 0; g < n_segs; ++g) full[g] = seg[g].n_blocks >= 32 ? ~uint64_t(0) : (uint64_t(1) << (2u * uint32_t(seg[g].n_blocks))) - 1;
    return full;
}

// The split's tables (IocSplitDev, ioc_internal.h): segment g has ceil(reads / 64) words a site — T words in all, tile_seg says
// whose each is — and words x sites words of each bit plane from bit_off[g] on, P in all; seg_of_site: the segment of every site;
// most: the largest segment's sites.
struct SplitTables {
    std::vector<uint32_t> word_off;
    std::vector<int64_t> bit_off;
    std::vector<int32_t> tile_seg, seg_of_site;
    size_t T = 0, P = 0, most = 0;
};
inline SplitTables split_tables(size_t n_segs, const int64_t* site_off, const std::vector<uint32_t>& mem_off)
{
    SplitTables s;
    s.word_off.assign(n_segs + 1, 0), s.bit_off.assign(n_segs + 1, 0);
    for (size_t g = 0; g < n_segs; ++g) {
        const uint32_t words = (mem_off[g + 1] - mem_off[g] + 63u) / 64u;
        s.word_off[g + 1] = s.word_off[g] + words;
        s.bit_off[g + 1] = s.bit_off[g] + int64_t(words) * (site_off[g + 1] - site_off[g]);
        s.most = std::max(s.most, size_t(site_off[g + 1] - site_off[g]));
    }
    s.T = s.word_off[n_segs], s.P = size_t(s.bit_off[n_segs]);
    s.tile_seg.resize(s.T), s.seg_of_site.resize(n_segs ? size_t(site_off[n_segs]) : 0);
    for (size_t g = 0; g < n_segs; ++g) {
        std::fill(s.tile_seg.begin() + s.word_off[g], s.tile_seg.begin() + s.word_off[g + 1], int32_t(g));
        std::fill(s.seg_of_site.begin() + site_off[g], s.seg_of_site.begin() + site_off[g + 1], int32_t(g));
    }
    return s;
}

// The bounds.  A consensus call writes at most a base per row and IOC_PILE_INS_SLOTS in front of every row, row rlen included
// (what ioc_host_pileup_call asks of cap); a site search keeps at most max_sites sites of a segment, and a row yields at most
// two, its insertion site and its base site, and row rlen one.
inline int64_t pile_call_most(int64_t rlen) { return rlen + int64_t(IOC_PILE_INS_SLOTS) * (rlen + 1); }
inline int64_t pile_sites_most(int64_t rlen, int32_t max_sites) { return std::min<int64_t>(max_sites, 2 * rlen + 1); }
// (a block search keeps at most max_blocks blocks of a segment, and a block has at least one row)
inline int64_t pile_blocks_most(int64_t rlen, int32_t max_blocks) { return std::min<int64_t>(max_blocks, rlen); }
inline int64_t pile_call_bound(const std::vector<IocPileSeg>& segs)
{
    return std::accumulate(segs.begin(), segs.end(), int64_t(0), [](int64_t b, const IocPileSeg& s) { return b + pile_call_most(s.rlen); });
}
inline int64_t pile_sites_bound(const std::vector<IocPileSeg>& segs, int32_t max_sites)
{
    return std::accumulate(segs.begin(), segs.end(), int64_t(0), [=](int64_t b, const IocPileSeg& s) { return b + pile_sites_most(s.rlen, max_sites); });
}

// The segments and the pairs of a call.  Segment g owns the rows segs[g].row0 .. + rlen of the call's tables, n_rows in all; pair
// i is piled from row_base[i] on, its segment's first row, and has rlen + 1 bytes from plane[i] on in every plane of plane_bytes
// bytes (the pairs one behind the other); alleles_bound: a byte per pair and site its segment may keep (from_pool); correct_bound:
// what the correction of every pair may write, its segment's call bound each (ioc_planes_correct asks it of cap); blocks_bound(m):
// the blocks a block search of max_blocks m may keep over all segments (ioc_planes_blocks asks it of blocks_cap).  frame_bytes:
// what the frames take of their pool (from_rlen).  A constructor returns IOC_OK, or the status of what it refuses with msg set —
// the caller hands both to ioc_fail; `who` names the entry point in it.  What only some entry points refuse: a segment of more than
// 2^30 bases (the site search: two sites a row) / one that may call more than 2^31 - 1 bytes (the record's out_len, the kernels' byte counts).
enum : unsigned { PLAN_REFUSE_LONG = 1, PLAN_REFUSE_CALLED = 2 };
struct SinkPlan {
    std::vector<IocPileSeg> segs;
    std::vector<int64_t> row_base, plane;
    int64_t n_rows = 0, frame_bytes = 0, plane_bytes = 0, alleles_bound = 0, correct_bound = 0;
    std::string msg;
    int64_t blocks_bound(int32_t max_blocks) const
    {
        return std::accumulate(segs.begin(), segs.end(), int64_t(0), [=](int64_t b, const IocPileSeg& sg) { return b + pile_blocks_most(sg.rlen, max_blocks); });
    }
    int refuse(int status, const std::string& who, const std::string& what) { return msg = who.empty() ? what : who + ": " + what, status; }
    void place_pair(size_t i, const IocPileSeg& sg, int32_t max_sites)
    {
        row_base[i] = sg.row0, plane[i] = plane_bytes;
        plane_bytes += int64_t(sg.rlen) + 1;
        alleles_bound += pile_sites_most(sg.rlen, max_sites);
        correct_bound += pile_call_most(sg.rlen);
    }

    // the segments are sequences of the aligner's pool (offs: where each starts, and the end), the pairs' references as long as
    // their segments' frames; max_sites: of the site search behind it, for alleles_bound (0: none)
    int from_pool(const std::string& who, const std::vector<int64_t>& offs, int32_t n_segs, const ioc_polish_seg* in, int32_t n_pairs,
                  const ioc_aln_pair* pairs, const int32_t* seg_of_pair, int32_t max_sites, unsigned flags)
    {
        const int64_t n_seqs = offs.empty() ? 0 : int64_t(offs.size()) - 1;
        auto len = [&](int32_t id) { return offs[size_t(id) + 1] - offs[size_t(id)]; };
        auto inside = [&](int32_t id) { return id >= 0 && id < n_seqs; };
        segs = std::vector<IocPileSeg>(size_t(n_segs));  // (not resize(): its instantiation would join the library's exported symbols)
        for (int32_t g = 0; g < n_segs; ++g) {
            if (!inside(in[g].ref)) return refuse(IOC_ERR_ARG, who, "segment " + std::to_string(g) + " refers to a sequence outside the pool");
            const int64_t m = len(in[g].ref);
            if ((flags & PLAN_REFUSE_LONG) && m > (1 << 30)) return refuse(IOC_ERR_CAPACITY, who, "segment " + std::to_string(g) + " is longer than 2^30 bases");
            segs[size_t(g)] = IocPileSeg{n_rows, offs[size_t(in[g].ref)], int32_t(m), in[g].ref_revcomp ? 1 : 0};
            n_rows += m + 1;
        }
        row_base.assign(size_t(n_pairs), 0), plane.assign(size_t(n_pairs), 0);
        for (int32_t i = 0; i < n_pairs; ++i) {
            if (!inside(pairs[i].query) || !inside(pairs[i].ref)) return refuse(IOC_ERR_ARG, "", "alignment pair refers to a sequence outside the pool");
            if (seg_of_pair[i] < 0 || seg_of_pair[i] >= n_segs) return refuse(IOC_ERR_ARG, who, "pair " + std::to_string(i) + " names no segment");
            const IocPileSeg& sg = segs[size_t(seg_of_pair[i])];
            if (len(pairs[i].ref) != sg.rlen) return refuse(IOC_ERR_ARG, who, "the reference of pair " + std::to_string(i) + " is not as long as its segment's frame");
            place_pair(size_t(i), sg, max_sites);
        }
        return IOC_OK;
    }

    // the segments are rlen[g] bases long, their frames at frame_off[g] of `frames` (frame_off NULL: a call that reads no frames);
    // the pairs (n_pairs 0: none) name their segments and, where `group` is given, carry a group byte each
    int from_rlen(const std::string& who, int32_t n_segs, const int32_t* rlen, const void* frames, const int64_t* frame_off, int32_t n_pairs,
                  const int32_t* seg_of_pair, const uint8_t* group, unsigned flags)
    {
        segs = std::vector<IocPileSeg>(size_t(n_segs));
        for (int32_t g = 0; g < n_segs; ++g) {
            if (rlen[g] < 0 || (frame_off && (frame_off[g] < 0 || (rlen[g] > 0 && !frames))))
                return refuse(IOC_ERR_ARG, who, "segment " + std::to_string(g) + " has a negative length" + (frame_off ? " or frame offset" : ""));
            if ((flags & PLAN_REFUSE_LONG) && rlen[g] > (1 << 30)) return refuse(IOC_ERR_CAPACITY, who, "segment " + std::to_string(g) + " is longer than 2^30 bases");
            if ((flags & PLAN_REFUSE_CALLED) && pile_call_most(rlen[g]) > INT32_MAX)
                return refuse(IOC_ERR_CAPACITY, who, "segment " + std::to_string(g) + " may call more than 2^31 - 1 bytes");
            segs[size_t(g)] = IocPileSeg{n_rows, frame_off ? frame_off[g] : 0, rlen[g], 0};
            n_rows += int64_t(rlen[g]) + 1;
            if (frame_off) frame_bytes = std::max(frame_bytes, frame_off[g] + rlen[g]);
        }
        row_base.assign(size_t(n_pairs), 0), plane.assign(size_t(n_pairs), 0);
        for (int32_t i = 0; i < n_pairs; ++i) {
            if (seg_of_pair[i] < 0 || seg_of_pair[i] >= n_segs) return refuse(IOC_ERR_ARG, who, "pair " + std::to_string(i) + " names no segment");
            if (group && group[i] > 1 && group[i] != IOC_SPLIT_NONE)
                return refuse(IOC_ERR_ARG, who, "the group byte of pair " + std::to_string(i) + " is neither 0, 1 nor IOC_SPLIT_NONE");
            place_pair(size_t(i), segs[size_t(seg_of_pair[i])], 0);
        }
        return IOC_OK;
    }
};

// Whose slot is this: unit u (a segment, or a segment's starts or stops) has the slots base[u] .. base[u + 1] of a row of slots,
// and entry x of the table names the unit of slot x.
template <class Off>
inline std::vector<int32_t> slot_owners(const Off* base, size_t units)
{
    std::vector<int32_t> owner(units ? size_t(base[units]) : 0);
    for (size_t u = 0; u < units; ++u) std::fill(owner.begin() + int64_t(base[u]), owner.begin() + int64_t(base[u + 1]), int32_t(u));
    return owner;
}

// A search leaves unit u's records in its slots from base[u] on and says how many of them it kept, kept(u), which the caller has
// held against the slots the unit has: the kept ones are packed into `out`, unit after unit, and off[0 .. units] says where each
// unit's begin.
template <class Rec, class Kept>
inline void pack_kept_slots(const std::vector<Rec>& slot, const int64_t* base, size_t units, Kept kept, Rec* out, int64_t* off)
{
    off[0] = 0;
    for (size_t u = 0; u < units; ++u) {
        std::copy(slot.begin() + base[u], slot.begin() + base[u] + kept(u), out + off[u]);
        off[u + 1] = off[u] + kept(u);
    }
}

// The words of the segments' bit planes (the stages of ioc_read_blocks.hip, ioc_read_inserts.hip and ioc_read_ends.hip): segment g
// has ceil((rlen + 1) / 64) words from seg_word[g] on, T in all, and word_seg says whose each is.
struct SegWordTable {
    std::vector<uint64_t> seg_word;
    std::vector<int32_t> word_seg;
    size_t T = 0;
};
inline SegWordTable seg_word_table(const std::vector<IocPileSeg>& segs)
{
    SegWordTable t;
    t.seg_word.assign(segs.size() + 1, 0);
    for (size_t g = 0; g < segs.size(); ++g) t.seg_word[g + 1] = t.seg_word[g] + uint64_t(segs[g].rlen) / 64 + 1;
    t.T = size_t(t.seg_word[segs.size()]);
    t.word_seg = slot_owners(t.seg_word.data(), segs.size());
    return t;
}

// The block search's tables (IocReadBlocksDev, ioc_internal.h): the segments' words, and as many words of a pair from pair_word[i]
// on, P words in all; block_base: where a segment's min(max_blocks, rlen) block slots begin, and their sum.
struct BlocksTables : SegWordTable {
    std::vector<uint64_t> pair_word;
    std::vector<int64_t> block_base;
    size_t P = 0;
};
inline BlocksTables blocks_tables(const SinkPlan& p, const int32_t* seg_of_pair, int32_t max_blocks)
{
    const size_t n = p.segs.size(), np = p.plane.size();
    BlocksTables t;
    static_cast<SegWordTable&>(t) = seg_word_table(p.segs);
    t.block_base.assign(n + 1, 0), t.pair_word.assign(np, 0);
    for (size_t g = 0; g < n; ++g) t.block_base[g + 1] = t.block_base[g] + pile_blocks_most(p.segs[g].rlen, max_blocks);
    for (size_t i = 0; i < np; ++i) t.pair_word[i] = t.P, t.P += size_t(t.seg_word[size_t(seg_of_pair[i]) + 1] - t.seg_word[size_t(seg_of_pair[i])]);
    return t;
}

#pragma GCC visibility pop

#endif
