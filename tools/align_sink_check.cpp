// align_sink_check.cpp — the host side of the aligner's sink description (isonclust2_amd/csrc/ioc_align_sink.h) and what the sink
// entry points plan before they launch anything (ioc_sink_plan.h), driven on the CPU:
//
//  * AlnSink::subset / take_back, which decide what a re-run (every tile, version 1) sees of the caller's pairs and what it leaves
//    them: for every sink kind, idx empty, one pair, all pairs, out of order — a pair piled before the re-run stays piled and its
//    row_base reaches the re-run unchanged (ops_reserve turns it into -1 from `piled`), a pair the re-run leaves unanswered keeps
//    len == 0 and piled == 0, the records of pairs outside idx are untouched, the bytes' regions are the caller's own; a pile
//    that projects (project, project_ins) hands the re-run its pairs' plane offsets, the planes' addresses and both flags;
//  * AlnSink::answer_empty, the closed forms of a pair with an empty sequence, for every kind and both empty sides;
//  * ops_layout, the per-slice table's offsets: those the kernels' launchers have always been handed, for np in {0, 1, 3, 5, 1000};
//  * aln_route and the accepted parameter range, at their edges and with the extreme values an int32 argument can carry (no
//    overflow on the way: the sums are 64-bit);
//  * ioc_sink_plan.h, each planner against a plain restatement written here: the arena layout (block sizes 0, 1, 15, 16, 17; the
//    totals of one case per stage against the hand-chained sums the stages used to carry), member_lists (no segments, no pairs,
//    segments without pairs, pairs out of segment order, one segment for all), group_member_lists (the same per group: pairs in
//    -1 or in a group their segment lacks, empty groups, segments without groups), the split's tables (0, 1, 64, 65 and 128 members,
//    a segment without sites between two with), the words of the segments' bit planes with the block search's tables on top of
//    them (63, 64, 65, 128 and 129 rows), whose slot is whose and the packing of kept slots, the bounds at their edges, and both constructors of SinkPlan with every refusal's
//    status and message as the entry points have always worded them;
//  * the block family's host lists, likewise: reads per segment (no segments, segments without pairs), the isoform cut (found 0,
//    found above max_iso, found above the reads and found negative, both refused with IOC_ERR_HIP and the callers' words), the key
//    of every kept isoform (group -1, a group behind the cut, two direct reads in one isoform, an isoform without a direct read),
//    a key's mask against blocks_state_mask state by state (IOC_BLOCK_NONE states among them) and the segments' full masks against
//    blocks_full_mask (n_blocks 0, 31 and 32).
//
// Host code only (the header includes no HIP header); meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/align_sink_check tools/align_sink_check.cpp && /tmp/align_sink_check
//
// Exit status 0 and "ok" when everything holds.
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "ioc_align_sink.h"
#include "ioc_read_blocks.h"
#include "ioc_sink_plan.h"

namespace {

long g_checks = 0;
bool g_ok = true;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        ++g_checks;                                                         \
        if (!(cond)) {                                                      \
            fprintf(stderr, "line %d (%s): %s\n", __LINE__, g_what, #cond); \
            g_ok = false;                                                   \
        }                                                                   \
    } while (0)
const char* g_what = "";

struct Kind {
    const char* name;
    SinkKind kind;
    bool stats;
    PileKind pile;
    int project = 0;  // 1: the pile projects (two planes); 2: and what the pairs insert (project_ins: six more); 3: and the weights (project_weights: seven more)
};
const Kind KINDS[] = {{"bytes", SinkKind::bytes, false, PileKind::none},
                      {"stats", SinkKind::reduced, true, PileKind::none},
                      {"counts", SinkKind::reduced, false, PileKind::counts},
                      {"counts+stats", SinkKind::reduced, true, PileKind::counts},
                      {"ins", SinkKind::reduced, false, PileKind::ins},
                      {"ins+stats", SinkKind::reduced, true, PileKind::ins},
                      {"weighted", SinkKind::reduced, false, PileKind::weighted},
                      {"weighted+stats", SinkKind::reduced, true, PileKind::weighted},
                      {"counts+project", SinkKind::reduced, false, PileKind::counts, 1},
                      {"counts+project+stats", SinkKind::reduced, true, PileKind::counts, 1},
                      {"counts+project_ins", SinkKind::reduced, false, PileKind::counts, 2},
                      {"counts+project_ins+stats", SinkKind::reduced, true, PileKind::counts, 2},
                      {"counts+project_weights", SinkKind::reduced, false, PileKind::counts, 3},
                      {"counts+project_weights+stats", SinkKind::reduced, true, PileKind::counts, 3}};

// the caller's arrays of a call over P pairs, of exactly the sizes an entry point gives them (a read or write outside them is the
// sanitizer's to find); the device tables are never dereferenced by the host: distinct addresses do
struct Caller {
    static constexpr int P = 6;
    static constexpr int64_t ROOM = 10;  // bytes per pair's region
    std::vector<uint8_t> buf;
    std::vector<int64_t> base, len, row_base, plane;
    static constexpr int64_t PLANE_BYTES = 1234;
    uint8_t t_planes[8];  // (one byte per plane: only the addresses count)
    std::vector<ioc_aln_stats> stats;
    std::vector<uint8_t> piled;
    AlnTally tally;
    ioc_pileup_col t_cols[1];
    ioc_pileup_ins t_ins[1];
    ioc_pileup_col t_wcols[1];
    ioc_pileup_ins t_wins[1];
    AlnSink sink;
    explicit Caller(const Kind& k) : len(P, 0)
    {
        sink.kind = k.kind;
        sink.len = len.data();
        sink.tally = &tally;
        if (k.kind == SinkKind::bytes) {
            buf.assign(size_t(P * ROOM), uint8_t('.'));
            for (int i = 0; i < P; ++i) base.push_back(i * ROOM);
            sink.bytes = {buf.data(), base.data()};
        }
        if (k.stats) {
            stats.assign(P, ioc_aln_stats{});
            for (int i = 0; i < P; ++i) stats[size_t(i)].length = 1000 + i;  // (what an earlier run left)
            sink.with_stats = true;
            sink.stats = stats.data();
        }
        if (k.pile != PileKind::none) {
            for (int i = 0; i < P; ++i) row_base.push_back(100 * i + 7);
            piled.assign(P, 0);
            sink.pile.kind = k.pile;
            sink.pile.cols = t_cols;
            if (k.pile == PileKind::ins) sink.pile.ins = t_ins;
            if (k.pile == PileKind::weighted) sink.pile.wcols = t_wcols, sink.pile.wins = t_wins;
            sink.pile.rows = 700;
            sink.pile.row_base = row_base.data();
            sink.pile.piled = piled.data();
        }
        if (k.project) {
            for (int i = 0; i < P; ++i) plane.push_back(200 * i + 3);
            sink.pile.project = true;
            sink.pile.base_planes = t_planes, sink.pile.ins_planes = t_planes + 1;
            sink.pile.plane_bytes = PLANE_BYTES;
            sink.pile.plane = plane.data();
            if (k.project >= 2) sink.pile.project_ins = true, sink.pile.slot_planes = t_planes + 2;
            if (k.project == 3) sink.pile.project_weights = true, sink.pile.weight_planes = t_planes + 3;
        }
    }
};

// a re-run over idx: pair x of it answers unless x is in `silent`; an answered pair gets a length, a record, and is piled unless it
// already was (as ops_fetch_reduced leaves the sub-sink's arrays)
void check_subset(const Kind& k, const std::vector<int32_t>& idx, const std::vector<size_t>& silent, const std::vector<int32_t>& piled_before)
{
    g_what = k.name;
    Caller c(k);
    const bool pile = k.pile != PileKind::none;
    for (int32_t i : piled_before)
        if (pile) c.piled[size_t(i)] = 1;
    const std::vector<ioc_aln_stats> stats_before = c.stats;
    const std::vector<uint8_t> piled_b = c.piled;
    const AlnSubSink sub = c.sink.subset(idx);
    const AlnSink& s = sub.sink;

    // the re-run's sink: the same kind, tables and tally; arrays of its own, one entry per pair of idx
    EXPECT(s.kind == c.sink.kind && s.tally == &c.tally && s.has_stats() == k.stats && s.has_pile() == pile);
    EXPECT(s.pile.kind == c.sink.pile.kind && s.pile.cols == c.sink.pile.cols && s.pile.ins == c.sink.pile.ins && s.pile.wcols == c.sink.pile.wcols &&
           s.pile.wins == c.sink.pile.wins && s.pile.rows == c.sink.pile.rows && s.pile_bytes() == c.sink.pile_bytes());
    EXPECT(sub.len.size() == idx.size() && s.len == sub.len.data());
    for (size_t x = 0; x < idx.size(); ++x) EXPECT(s.len[x] == 0);
    if (k.kind == SinkKind::bytes) {
        EXPECT(s.bytes.buf == c.buf.data() && sub.base.size() == idx.size() && s.bytes.base == sub.base.data());
        for (size_t x = 0; x < idx.size(); ++x) EXPECT(s.bytes.base[x] == c.base[size_t(idx[x])]);
    }
    if (k.stats) {
        EXPECT(sub.stats.size() == idx.size() && s.stats == sub.stats.data());
        const ioc_aln_stats zero{};
        for (size_t x = 0; x < idx.size(); ++x) EXPECT(memcmp(&s.stats[x], &zero, sizeof zero) == 0);
    }
    if (pile) {
        EXPECT(sub.row_base.size() == idx.size() && sub.piled.size() == idx.size() && s.pile.row_base == sub.row_base.data() && s.pile.piled == sub.piled.data());
        for (size_t x = 0; x < idx.size(); ++x) {
            EXPECT(s.pile.row_base[x] == c.row_base[size_t(idx[x])]);  // (unchanged, piled or not)
            EXPECT(s.pile.piled[x] == piled_b[size_t(idx[x])]);
        }
    }
    EXPECT(s.projects() == (k.project != 0) && s.projects_ins() == (k.project >= 2) && s.projects_weights() == (k.project == 3));
    if (k.project) {
        EXPECT(sub.plane.size() == idx.size() && s.pile.plane == sub.plane.data() && s.pile.plane_bytes == Caller::PLANE_BYTES);
        EXPECT(s.pile.base_planes == c.sink.pile.base_planes && s.pile.ins_planes == c.sink.pile.ins_planes && s.pile.slot_planes == c.sink.pile.slot_planes);
        EXPECT((s.pile.slot_planes != nullptr) == (k.project >= 2) && (s.pile.weight_planes != nullptr) == (k.project == 3));
        for (size_t x = 0; x < idx.size(); ++x) EXPECT(s.pile.plane[x] == c.plane[size_t(idx[x])]);
    } else {
        EXPECT(sub.plane.empty());
    }

    // the re-run, as ops_fetch / ops_fetch_reduced write through the sink
    std::vector<uint8_t> answered(idx.size(), 1);
    for (size_t x : silent)
        if (x < idx.size()) answered[x] = 0;
    for (size_t x = 0; x < idx.size(); ++x) {
        if (!answered[x]) continue;
        if (k.kind == SinkKind::bytes) memset(s.bytes.buf + s.bytes.base[x], 'a' + int(x), 3);
        if (s.has_stats()) s.stats[x].length = 50 + int32_t(x);
        if (s.has_pile()) s.pile.piled[x] = 1;
        s.len[x] = 3 + int64_t(x);
    }
    c.sink.take_back(idx, sub);

    std::vector<int> where(Caller::P, -1);  // caller's pair -> its place in idx
    for (size_t x = 0; x < idx.size(); ++x) where[size_t(idx[x])] = int(x);
    for (int i = 0; i < Caller::P; ++i) {
        const int x = where[size_t(i)];
        const bool ans = x >= 0 && answered[size_t(x)];
        EXPECT(c.len[size_t(i)] == (ans ? 3 + x : 0));
        if (k.kind == SinkKind::bytes) {
            const std::string got(reinterpret_cast<const char*>(c.buf.data()) + i * Caller::ROOM, size_t(Caller::ROOM));
            EXPECT(got == (ans ? std::string(3, char('a' + x)) + std::string(7, '.') : std::string(10, '.')));
        }
        if (k.stats) {
            // outside idx: untouched; in idx: the re-run's record, an empty one where it had no answer either
            const int32_t want = x < 0 ? stats_before[size_t(i)].length : ans ? 50 + x : 0;
            EXPECT(c.stats[size_t(i)].length == want);
        }
        if (pile) EXPECT(c.piled[size_t(i)] == ((piled_b[size_t(i)] || ans) ? 1 : 0));
    }
}

void check_empty(const Kind& k)
{
    g_what = k.name;
    for (int side = 0; side < 2; ++side) {
        Caller c(k);
        const int64_t n = side ? 0 : 7, m = side ? 9 : 0, l = n + m;
        const size_t i = 2;
        c.sink.answer_empty(i, n, m);
        for (size_t j = 0; j < size_t(Caller::P); ++j) EXPECT(c.len[j] == (j == i ? l : 0));
        if (k.kind == SinkKind::bytes)
            for (size_t b = 0; b < c.buf.size(); ++b) {
                const bool in = b >= i * Caller::ROOM && b < i * Caller::ROOM + size_t(l);
                EXPECT(c.buf[b] == (in ? (n ? 'i' : 'd') : '.'));
            }
        if (k.stats) {
            ioc_aln_stats want{};
            want.length = int32_t(l);
            (n ? want.lead_i : want.lead_d) = int32_t(l);
            EXPECT(memcmp(&c.stats[i], &want, sizeof want) == 0);
            for (size_t j = 0; j < size_t(Caller::P); ++j)
                if (j != i) EXPECT(c.stats[j].length == 1000 + int32_t(j));
        }
        if (k.pile != PileKind::none)
            for (uint8_t p : c.piled) EXPECT(p == 0);  // (nothing is added, so nothing is marked)
    }
}

void check_layout(const Kind& k)
{
    g_what = k.name;
    // (project_ins and project_weights add no column: their planes sit at the pair's `plane` offset like the two, and the q_len column a
    // weight projection reads lies inside every projecting table, between q_off and plane)
    const size_t per_pair = k.kind == SinkKind::bytes ? 12 : k.project ? 40 : k.pile == PileKind::weighted ? 32 : k.pile != PileKind::none ? 28 : 16;
    for (size_t np : {size_t(0), size_t(1), size_t(3), size_t(5), size_t(1000)}) {
        Caller c(k);
        const OpsLayout a = ops_layout(np, k.kind, k.pile, k.project != 0), b = c.sink.layout(np);
        EXPECT(memcmp(&a, &b, sizeof a) == 0);
        EXPECT(a.end == 0 && a.len == 8 * np && a.room == 12 * np && a.row_base == 16 * np && a.q_off == 24 * np && a.q_len == 28 * np);
        EXPECT(a.bytes == ((np * per_pair + 15) / 16) * 16 && a.bytes % 16 == 0 && a.bytes >= np * per_pair && a.bytes < np * per_pair + 16);
        EXPECT(a.row_base % 8 == 0);
        EXPECT(a.spare == (k.kind == SinkKind::reduced ? 4u : 0u));
        // every column the kind has ends inside the table
        if (k.kind == SinkKind::reduced) EXPECT(a.room + 4 * np <= a.bytes);
        if (k.pile != PileKind::none) EXPECT(a.q_off + 4 * np <= a.bytes);
        if (k.pile == PileKind::weighted) EXPECT(a.q_len + 4 * np <= a.bytes);
        if (k.project) EXPECT(a.plane == 32 * np && a.plane % 8 == 0 && a.plane + 8 * np <= a.bytes);
        if (k.project) EXPECT(a.q_len == 28 * np && a.q_len + 4 * np <= a.plane);
    }
}

void check_routes()
{
    g_what = "routes";
    for (int go = 2; go <= 5; ++go) EXPECT(aln_route(2, -2, 1, go) == ALN_ROUTE_V2);  // the default parameters: version 2, as ever
    EXPECT(aln_route(2, -6, 1, 5) == ALN_ROUTE_V2 && aln_route(2, -6, 1, 4) == ALN_ROUTE_COMPARE);       // cx 0 / -1
    EXPECT(aln_route(250, -2, 1, 4) == ALN_ROUTE_PROFILE && aln_route(250, -2, 1, 5) == ALN_ROUTE_COMPARE);  // cm 255 / 256
    EXPECT(aln_route(2, -2, 2, 2) == ALN_ROUTE_V2 && aln_route(2, -2, 3, 2) == ALN_ROUTE_PROFILE);       // gd 0 / -1
    EXPECT(aln_route(28, -2, 1, 2) == ALN_ROUTE_V2 && aln_route(29, -2, 1, 2) == ALN_ROUTE_PROFILE);     // max(cm, cx) 31 / 32
    const int32_t lo = INT32_MIN, hi = INT32_MAX;
    for (int32_t a : {lo, -1, 0, 1, hi})
        for (int32_t b : {lo, -1, 0, 1, hi})
            for (int32_t g : {lo, -1, 0, 1, hi}) {
                const int r = aln_route(a, b, g, 5);
                EXPECT(r >= ALN_ROUTE_COMPARE && r <= ALN_ROUTE_V2);
                EXPECT(aln_params_ok(a, b, g) == (g >= 0 && aln_param_weight(a, b, g) <= ALN_PARAM_MOST));
                EXPECT(aln_params_ok(a, b, g) == (a > -(1 << 24) && a < (1 << 24) && b > -(1 << 24) && b < (1 << 24) && g >= 0 && g <= 1));
            }
    // the default parameters: every pair a pool can hold (n + m < 2^26, prepare_pairs)
    EXPECT(aln_params_ok(2, -2, 1) && aln_span_ok(2, -2, 1, (int64_t(1) << 26) - 1, 0));
    EXPECT(aln_span_ok(1 << 20, -2, 0, 500, 523) && !aln_span_ok(1 << 20, -2, 0, 500, 524));  // (2^20 + 5) x 1023 <= 2^30 < ... x 1024
}


// ---- ioc_sink_plan.h ----
size_t up16(size_t v) { return (v + 15) / 16 * 16; }

void check_arena()
{
    g_what = "arena";
    Arena a;
    size_t want = 0;
    for (size_t b : {size_t(0), size_t(1), size_t(15), size_t(16), size_t(17), size_t(0), size_t(0), size_t(33)}) {
        EXPECT(a.take(b) == want && want % 16 == 0);  // (a block of 0 bytes: the next one starts where it does)
        want += b == 0 ? 0 : b <= 16 ? 16 : b <= 32 ? 32 : 48;
        EXPECT(a.size() == want);
    }
    // one case per stage: the blocks in the stage's order against the sums that were chained by hand
    const size_t n = 3, np = 5, bound = 7, ab = 11, seg = sizeof(IocPileSeg), site = sizeof(ioc_pile_site), st = sizeof(ioc_polish_stats);
    {  // the site search and the allele gather (a_call)
        const size_t o_len = up16(n * seg), o_off = o_len + up16(n * 8), o_found = o_off + up16((n + 1) * 8), o_sites = o_found + up16(n * 8),
                     o_sop = o_sites + up16(bound * site), o_plane = o_sop + up16(np * 4), o_aoff = o_plane + up16(np * 8), o_all = o_aoff + up16((np + 1) * 8),
                     total = o_all + up16(ab);
        Arena l;
        EXPECT(l.take(n * seg) == 0 && l.take(n * 8) == o_len && l.take((n + 1) * 8) == o_off && l.take(n * 8) == o_found && l.take(bound * site) == o_sites);
        EXPECT(l.take(np * 4) == o_sop && l.take(np * 8) == o_plane && l.take((np + 1) * 8) == o_aoff && l.take(ab) == o_all && l.size() == total);
    }
    {  // the call (a_call): the records are 32 bytes, so the block behind them starts where the unrounded sum put it
        const size_t o_len = up16(n * seg), o_off = o_len + up16(n * 8), o_st = o_off + up16((n + 1) * 8), o_seq = o_st + n * st, o_qual = o_seq + up16(bound),
                     total = o_qual + up16(bound);
        Arena l;
        EXPECT(st % 16 == 0 && l.take(n * seg) == 0 && l.take(n * 8) == o_len && l.take((n + 1) * 8) == o_off && l.take(n * st) == o_st);
        EXPECT(l.take(bound) == o_seq && l.take(bound) == o_qual && l.size() == total);
    }
    for (int on_device = 0; on_device < 2; ++on_device) {  // the split (a_split) and the group pile (a_gpile): blocks that are 0 bytes where nothing is uploaded
        const size_t S = 9, T = 4, P = 13, bytes = 21, rows = 17, work = 6;
        const size_t split[] = {(n + 1) * 8, (np + 1) * 8, np * 4, (n + 1) * 4, np * 4, (n + 1) * 4, (n + 1) * 8, T * 4, S * 4, S * 8, P * 8, P * 8, T * 8, T * 8, S * 8,
                                S, n * 4, np, np * 4, n * sizeof(ioc_split_seg), on_device ? 0 : S * site, on_device ? 0 : bytes};
        const size_t gpile[] = {2 * n * seg, work * 8, np * 8, on_device ? 0 : (n + 1) * 4, on_device ? 0 : np * 4, on_device ? 0 : np, on_device ? 0 : P,
                                on_device ? 0 : 6 * P, rows * sizeof(ioc_pileup_col), rows * sizeof(ioc_pileup_ins)};
        Arena l, g;
        size_t at = 0;
        for (size_t b : split) {
            EXPECT(l.take(b) == at);
            at += up16(b);
        }
        EXPECT(l.size() == at);
        at = 0;
        for (size_t b : gpile) {
            EXPECT(g.take(b) == at);
            at += up16(b);
        }
        EXPECT(g.size() == at);
    }
}

void check_member_lists()
{
    g_what = "member_lists";
    const struct { size_t n; std::vector<int32_t> sop; } cases[] = {
        {0, {}}, {3, {}}, {4, {1, 1, 3}} /* none at the front, in the middle */, {4, {0, 2, 0}} /* ... at the end */, {3, {2, 0, 1, 0, 2, 2, 1}} /* out of order */,
        {3, {1, 1, 1, 1}} /* all in one */, {1, {0}}};
    for (const auto& k : cases) {
        const MemberLists m = member_lists(k.n, k.sop.size(), k.sop.data());
        std::vector<uint32_t> off{0}, mem;
        for (size_t g = 0; g < k.n; ++g) {
            for (size_t i = 0; i < k.sop.size(); ++i)
                if (size_t(k.sop[i]) == g) mem.push_back(uint32_t(i));
            off.push_back(uint32_t(mem.size()));
        }
        EXPECT(m.mem_off == off && m.members == mem);
    }
}

void check_group_member_lists()
{
    g_what = "group_member_lists";
    const struct { std::vector<int32_t> ng, sop, grp; } cases[] = {
        {{}, {}, {}}, {{2, 0, 3}, {}, {}} /* no pairs */, {{0, 0}, {0, 1, 1}, {-1, -1, -1}} /* pairs and no groups */,
        {{2, 4, 1, 0}, {1, 0, 1, 1, 0, 2, 1, 0, 1, 3}, {2, 0, 0, -1, 1, 0, 2, 0, 5, -1}} /* out of order, -1, an empty group, a group the segment lacks */,
        {{3}, {0, 0, 0, 0}, {1, 1, 1, 1}} /* all in one */, {{1, 1}, {1, 0}, {0, 0}}};
    for (const auto& k : cases) {
        const size_t n = k.ng.size();
        const GroupMemberLists m = group_member_lists(n, k.sop.size(), k.sop.data(), k.grp.data(), k.ng.data());
        std::vector<uint32_t> gseg{0}, off{0}, mem;
        for (size_t g = 0; g < n; ++g) {
            for (int32_t h = 0; h < k.ng[g]; ++h) {
                for (size_t i = 0; i < k.sop.size(); ++i)
                    if (size_t(k.sop[i]) == g && k.grp[i] == h) mem.push_back(uint32_t(i));
                off.push_back(uint32_t(mem.size()));
            }
            gseg.push_back(gseg.back() + uint32_t(k.ng[g]));
        }
        EXPECT(m.gseg_off == gseg && m.gmem_off == off && m.gmembers == mem);
    }
}

void check_split_tables()
{
    g_what = "split_tables";
    static_assert(std::is_same<decltype(SplitTables::bit_off), std::vector<int64_t>>::value, "words x sites are summed in 64 bits");
    const std::vector<uint32_t> members{0, 1, 64, 65, 128, 3};
    const std::vector<int64_t> sites{3, 2, 0, 5, 1, 4};  // (a segment without sites between two with)
    for (size_t n = 0; n <= members.size(); ++n) {
        std::vector<uint32_t> mem_off{0};
        std::vector<int64_t> site_off{0};
        for (size_t g = 0; g < n; ++g) mem_off.push_back(mem_off[g] + members[g]), site_off.push_back(site_off[g] + sites[g]);
        const SplitTables s = split_tables(n, site_off.data(), mem_off);
        std::vector<uint32_t> word_off{0};
        std::vector<int64_t> bit_off{0};
        std::vector<int32_t> tile_seg, seg_of_site;
        size_t most = 0;
        for (size_t g = 0; g < n; ++g) {
            uint32_t words = 0;
            while (64 * words < members[g]) ++words;
            word_off.push_back(word_off[g] + words), bit_off.push_back(bit_off[g] + int64_t(words) * sites[g]);
            tile_seg.insert(tile_seg.end(), words, int32_t(g)), seg_of_site.insert(seg_of_site.end(), size_t(sites[g]), int32_t(g));
            most = sites[g] > int64_t(most) ? size_t(sites[g]) : most;
        }
        EXPECT(s.word_off == word_off && s.bit_off == bit_off && s.tile_seg == tile_seg && s.seg_of_site == seg_of_site);
        EXPECT(s.T == word_off[n] && s.P == size_t(bit_off[n]) && s.most == most);
    }
    const std::vector<uint32_t> words_of{0, 1, 1, 2, 2};  // 0, 1, 64 | 65, 128 members: a word boundary either side
    for (size_t g = 0; g < 5; ++g) EXPECT(split_tables(1, std::vector<int64_t>{0, 1}.data(), {0, members[g]}).T == words_of[g]);
}

// the words of the segments' bit planes, the blocks' tables on top of them, whose slot is whose, and the packing of kept slots
void check_slot_tables()
{
    g_what = "slot tables";
    const std::vector<int32_t> rlens{0, 1, 62, 63, 64, 127, 128, 600, 0};  // rlen + 1 rows: 63 | 64 | 65 and 128 | 129 rows either side of a word
    for (size_t n = 0; n <= rlens.size(); ++n) {
        std::vector<IocPileSeg> segs;
        std::vector<uint64_t> seg_word{0};
        std::vector<int32_t> word_seg;
        for (size_t g = 0; g < n; ++g) {
            uint64_t words = 0;
            while (64 * words < uint64_t(rlens[g]) + 1) ++words;
            segs.push_back(IocPileSeg{0, 0, rlens[g], 0});
            seg_word.push_back(seg_word[g] + words), word_seg.insert(word_seg.end(), size_t(words), int32_t(g));
        }
        const SegWordTable t = seg_word_table(segs);
        EXPECT(t.seg_word == seg_word && t.word_seg == word_seg && t.T == word_seg.size());
        SinkPlan pn;
        pn.segs = segs;
        std::vector<int32_t> sop;
        for (size_t g = n; g-- > 0;) sop.push_back(int32_t(g)), sop.push_back(int32_t(g));  // (two pairs a segment, out of segment order)
        pn.plane.assign(sop.size(), 0);
        const BlocksTables b = blocks_tables(pn, sop.data(), 4);
        EXPECT(b.seg_word == seg_word && b.word_seg == word_seg && b.T == t.T && b.P == 2 * t.T && b.block_base.size() == n + 1);
        uint64_t at = 0;
        for (size_t i = 0; i < sop.size(); ++i) {
            EXPECT(b.pair_word[i] == at);
            at += seg_word[size_t(sop[i]) + 1] - seg_word[size_t(sop[i])];
        }
        for (size_t g = 0; g < n; ++g) EXPECT(b.block_base[g + 1] - b.block_base[g] == (rlens[g] < 4 ? rlens[g] : 4));
    }
    const std::vector<int64_t> base{0, 3, 3, 4, 9};  // (a unit without slots between two with)
    EXPECT(slot_owners(base.data(), 4) == (std::vector<int32_t>{0, 0, 0, 2, 3, 3, 3, 3, 3}));
    EXPECT(slot_owners(base.data(), 0).empty() && slot_owners(std::vector<uint64_t>{0, 0}.data(), 1).empty());
    const std::vector<int32_t> slot{10, 11, 12, 20, 30, 31, 32, 33, 34}, kept{2, 0, 1, 5};
    std::vector<int32_t> out(8, -1);
    std::vector<int64_t> off(5, -1);
    pack_kept_slots(slot, base.data(), 4, [&](size_t u) { return kept[u]; }, out.data(), off.data());
    EXPECT(out == (std::vector<int32_t>{10, 11, 20, 30, 31, 32, 33, 34}) && off == (std::vector<int64_t>{0, 2, 2, 3, 8}));
    int64_t none = -1;
    pack_kept_slots(std::vector<int32_t>{}, base.data(), 0, [](size_t) { return 0; }, static_cast<int32_t*>(nullptr), &none);
    EXPECT(none == 0);
}

void check_bounds()
{
    g_what = "bounds";
    const int32_t rlen = 5;
    const std::vector<IocPileSeg> one{{0, 0, rlen, 0}}, two{{0, 0, 0, 0}, {1, 0, 1, 0}};
    EXPECT(pile_sites_bound(one, 1) == 1 && pile_sites_bound(one, 2 * rlen) == 2 * rlen && pile_sites_bound(one, 2 * rlen + 1) == 2 * rlen + 1 &&
           pile_sites_bound(one, 2 * rlen + 2) == 2 * rlen + 1);
    EXPECT(pile_call_most(0) == IOC_PILE_INS_SLOTS && pile_call_most(1) == 1 + 2 * IOC_PILE_INS_SLOTS && pile_call_bound(two) == 1 + 3 * IOC_PILE_INS_SLOTS);
    EXPECT(pile_call_bound({}) == 0 && pile_sites_bound({}, 7) == 0 && pile_sites_bound(two, 2) == 1 + 2 && pile_sites_bound(two, INT32_MAX) == 1 + 3);
}

// a constructor's verdict: the status, and the message where it refuses
#define REFUSED(call, st, text)                        \
    do {                                               \
        SinkPlan p_;                                   \
        EXPECT(p_.call == (st) && p_.msg == (text));   \
    } while (0)

void check_plan_rlen()
{
    g_what = "plan from rlen";
    const char frames[16] = {};
    {  // lengths 0 among the others; frames that overlap: frame_bytes is the largest end, not the sum
        const int32_t rlen[] = {5, 0, 3};
        const int64_t f_off[] = {10, 2, 0};
        const int32_t sop[] = {2, 0, 2, 1};
        const uint8_t group[] = {0, 1, IOC_SPLIT_NONE, 1};
        SinkPlan p;
        EXPECT(p.from_rlen("ioc_planes_polish", 3, rlen, frames, f_off, 4, sop, group, 0) == IOC_OK && p.msg.empty());
        EXPECT(p.n_rows == 6 + 1 + 4 && p.frame_bytes == 15 && p.plane_bytes == 4 + 6 + 4 + 1 && p.alleles_bound == 0);
        const int64_t row0[] = {0, 6, 7}, plane[] = {0, 4, 10, 14};
        for (int g = 0; g < 3; ++g) EXPECT(p.segs[g].row0 == row0[g] && p.segs[g].f_off == f_off[g] && p.segs[g].rlen == rlen[g] && p.segs[g].rc == 0);
        for (int i = 0; i < 4; ++i) EXPECT(p.row_base[i] == row0[sop[i]] && p.plane[i] == plane[i]);
        REFUSED(from_rlen("ioc_planes_polish", 3, rlen, frames, f_off, 4, std::vector<int32_t>{2, -1, 2, 1}.data(), group, 0), IOC_ERR_ARG, "ioc_planes_polish: pair 1 names no segment");
        REFUSED(from_rlen("ioc_planes_polish", 3, rlen, frames, f_off, 4, std::vector<int32_t>{2, 0, 2, 3}.data(), group, 0), IOC_ERR_ARG, "ioc_planes_polish: pair 3 names no segment");
        REFUSED(from_rlen("ioc_planes_polish", 3, rlen, frames, f_off, 4, sop, std::vector<uint8_t>{0, 1, 2, 1}.data(), 0), IOC_ERR_ARG,
                "ioc_planes_polish: the group byte of pair 2 is neither 0, 1 nor IOC_SPLIT_NONE");
        SinkPlan q;  // (no group bytes: not looked at; no frame offsets: a site search, f_off 0)
        EXPECT(q.from_rlen("ioc_pileup_sites", 3, rlen, nullptr, nullptr, 0, nullptr, nullptr, PLAN_REFUSE_LONG) == IOC_OK && q.frame_bytes == 0 && q.n_rows == 11 && q.segs[2].f_off == 0);
    }
    const int32_t zeros[] = {0, 0}, mixed[] = {0, 2}, neg[] = {1, -1};
    const int64_t f0[] = {0, 0}, fneg[] = {0, -1};
    SinkPlan p;
    EXPECT(p.from_rlen("ioc_pileup_call", 2, zeros, nullptr, f0, 0, nullptr, nullptr, PLAN_REFUSE_CALLED) == IOC_OK && p.n_rows == 2 && p.frame_bytes == 0);
    for (const char* who : {"ioc_pileup_call", "ioc_planes_polish"}) {
        const std::string w = who;
        REFUSED(from_rlen(w, 2, mixed, nullptr, f0, 0, nullptr, nullptr, 0), IOC_ERR_ARG, w + ": segment 1 has a negative length or frame offset");
        REFUSED(from_rlen(w, 2, neg, frames, f0, 0, nullptr, nullptr, 0), IOC_ERR_ARG, w + ": segment 1 has a negative length or frame offset");
        REFUSED(from_rlen(w, 2, zeros, frames, fneg, 0, nullptr, nullptr, 0), IOC_ERR_ARG, w + ": segment 1 has a negative length or frame offset");
    }
    REFUSED(from_rlen("ioc_pileup_sites", 2, neg, nullptr, nullptr, 0, nullptr, nullptr, PLAN_REFUSE_LONG), IOC_ERR_ARG, "ioc_pileup_sites: segment 1 has a negative length");
    // 7 rlen + 6 > 2^31 - 1 first at rlen 306783378; a site search's 2^30
    const int32_t most[] = {306783377}, over[] = {3, 306783378}, l30[] = {1 << 30}, l30p[] = {(1 << 30) + 1};
    SinkPlan a, b, d;
    EXPECT(a.from_rlen("ioc_pileup_call", 1, most, frames, f0, 0, nullptr, nullptr, PLAN_REFUSE_CALLED) == IOC_OK && pile_call_bound(a.segs) == INT32_MAX - 2);
    REFUSED(from_rlen("ioc_pileup_call", 2, over, frames, f0, 0, nullptr, nullptr, PLAN_REFUSE_CALLED), IOC_ERR_CAPACITY, "ioc_pileup_call: segment 1 may call more than 2^31 - 1 bytes");
    EXPECT(b.from_rlen("ioc_planes_polish", 2, over, frames, f0, 0, nullptr, nullptr, 0) == IOC_OK);  // (that entry point asks later, once its pairs are known)
    EXPECT(d.from_rlen("ioc_pileup_sites", 1, l30, nullptr, nullptr, 0, nullptr, nullptr, PLAN_REFUSE_LONG) == IOC_OK && d.n_rows == (int64_t(1) << 30) + 1);
    REFUSED(from_rlen("ioc_pileup_sites", 1, l30p, nullptr, nullptr, 0, nullptr, nullptr, PLAN_REFUSE_LONG), IOC_ERR_CAPACITY, "ioc_pileup_sites: segment 0 is longer than 2^30 bases");
}

void check_plan_pool()
{
    g_what = "plan from the pool";
    const std::vector<int64_t> offs{0, 4, 4, 9, 14};  // four sequences: 4, 0, 5 and 5 bases
    const int32_t n_seqs = 4, max_sites = 9;
    const ioc_polish_seg segs[] = {{2, 0}, {1, 1}, {0, 0}};  // (an empty sequence as a segment)
    const ioc_aln_pair pairs[] = {{0, 3, 0, 0, 0.0}, {1, 0, 0, 0, 0.0}, {3, 2, 1, 0, 0.0}, {0, 1, 0, 0, 0.0}};  // references of 5, 4, 5 and 0 bases
    const int32_t sop[] = {0, 2, 0, 1};
    for (const char* who : {"ioc_align_pairs_polish", "ioc_align_pairs_alleles", "ioc_align_pairs_split", "ioc_align_pairs_split_polish"}) {
        const std::string w = who;
        const unsigned flags = w == "ioc_align_pairs_polish" ? 0 : PLAN_REFUSE_LONG;
        SinkPlan p;
        EXPECT(p.from_pool(w, offs, 3, segs, 4, pairs, sop, max_sites, flags) == IOC_OK && p.msg.empty());
        EXPECT(p.n_rows == 6 + 1 + 5 && p.plane_bytes == 6 + 5 + 6 + 1 && p.frame_bytes == 0);
        const int64_t row0[] = {0, 6, 7}, f_off[] = {4, 4, 0}, plane[] = {0, 6, 11, 17};
        const int32_t rlen[] = {5, 0, 4}, rc[] = {0, 1, 0};
        int64_t ab = 0;
        for (int g = 0; g < 3; ++g) EXPECT(p.segs[g].row0 == row0[g] && p.segs[g].f_off == f_off[g] && p.segs[g].rlen == rlen[g] && p.segs[g].rc == rc[g]);
        for (int i = 0; i < 4; ++i) {
            EXPECT(p.row_base[i] == row0[sop[i]] && p.plane[i] == plane[i]);
            ab += 2 * rlen[sop[i]] + 1 < max_sites ? 2 * rlen[sop[i]] + 1 : max_sites;
        }
        EXPECT(p.row_base[0] == p.row_base[2] && p.plane[2] == p.plane[0] + 6 + 5 && p.alleles_bound == ab && ab == 9 + 9 + 9 + 1);
        for (int32_t bad : {-1, n_seqs}) {
            const ioc_polish_seg sb[] = {{2, 0}, {bad, 0}, {0, 0}};
            REFUSED(from_pool(w, offs, 3, sb, 4, pairs, sop, max_sites, flags), IOC_ERR_ARG, w + ": segment 1 refers to a sequence outside the pool");
            const ioc_aln_pair pq[] = {{bad, 3, 0, 0, 0.0}}, pr[] = {{0, bad, 0, 0, 0.0}};
            REFUSED(from_pool(w, offs, 3, segs, 1, pq, sop, max_sites, flags), IOC_ERR_ARG, "alignment pair refers to a sequence outside the pool");
            REFUSED(from_pool(w, offs, 3, segs, 1, pr, sop, max_sites, flags), IOC_ERR_ARG, "alignment pair refers to a sequence outside the pool");
        }
        for (int32_t bad : {-1, 3}) {
            const int32_t sb[] = {0, 2, bad, 1};
            REFUSED(from_pool(w, offs, 3, segs, 4, pairs, sb, max_sites, flags), IOC_ERR_ARG, w + ": pair 2 names no segment");
        }
        const int32_t off_by_one[] = {0, 0, 0, 1};  // pair 1's reference has 4 bases, segment 0's frame 5
        REFUSED(from_pool(w, offs, 3, segs, 4, pairs, off_by_one, max_sites, flags), IOC_ERR_ARG, w + ": the reference of pair 1 is not as long as its segment's frame");
        REFUSED(from_pool(w, {}, 1, segs, 0, nullptr, nullptr, max_sites, flags), IOC_ERR_ARG, w + ": segment 0 refers to a sequence outside the pool");
        const std::vector<int64_t> long_pool{0, (int64_t(1) << 30) + 1};
        const ioc_polish_seg s0[] = {{0, 0}};
        SinkPlan q;
        if (flags) REFUSED(from_pool(w, long_pool, 1, s0, 0, nullptr, nullptr, max_sites, flags), IOC_ERR_CAPACITY, w + ": segment 0 is longer than 2^30 bases");
        else EXPECT(q.from_pool(w, long_pool, 1, s0, 0, nullptr, nullptr, 0, flags) == IOC_OK && q.n_rows == (int64_t(1) << 30) + 2);
    }
}

// The block family's host lists, each against a plain restatement: reads per segment, the isoform cut with both refusals, the keys
// of the kept isoforms, a key's mask and the segments' full masks.
void check_block_lists()
{
    g_what = "block family lists";
    // reads per segment: no segments, segments without pairs (1 and 3), pairs out of segment order
    EXPECT(reads_per_seg(0, 0, nullptr).empty());
    const int32_t sop[] = {2, 0, 2, 2, 0, 4, 2, 4};
    const size_t n = 5, np = sizeof sop / sizeof sop[0];
    const std::vector<int64_t> reads = reads_per_seg(n, np, sop);
    EXPECT(reads == (std::vector<int64_t>{2, 0, 4, 0, 2}) && reads_per_seg(3, 0, nullptr) == (std::vector<int64_t>{0, 0, 0}));

    // the cut: found 0 (with and without reads), found below, at and above max_iso, found as large as the reads
    const int32_t max_iso = 2;
    const int32_t found[] = {2, 0, 4, 0, 1};
    std::vector<int64_t> iso_off(n + 1, 0);
    IsoCut cut;
    EXPECT(cut.from("insert", n, found, reads.data(), max_iso, iso_off.data()) == IOC_OK && cut.msg.empty());
    int64_t at = 0;
    for (size_t g = 0; g < n; ++g) {
        const int32_t want = found[g] < max_iso ? found[g] : max_iso;
        EXPECT(cut.n_iso[g] == want && iso_off[g] == at);
        at += want;
    }
    EXPECT(iso_off[n] == at && at == 2 + 0 + 2 + 0 + 1);
    IsoCut none;
    int64_t zero = 0;
    EXPECT(none.from("block", 0, nullptr, nullptr, max_iso, &zero) == IOC_OK && none.n_iso.empty() && zero == 0);
    // the refusals: more isoforms than reads (one more than the two reads; any at all in a segment without reads), fewer than none —
    // IOC_ERR_HIP, the words the block and the insert callers have always used, the offsets of the segments before it written
    for (const char* search : {"block", "insert"}) {
        const std::string text = std::string("the ") + search + " search returned more isoforms than reads";
        const int32_t over[] = {2, 0, 4, 0, 3}, empty_seg[] = {2, 1, 4, 0, 1}, neg[] = {2, 0, -1, 0, 1};
        for (const int32_t* bad : {over, empty_seg, neg}) {
            std::vector<int64_t> off(n + 1, 0);
            IsoCut c;
            EXPECT(c.from(search, n, bad, reads.data(), max_iso, off.data()) == IOC_ERR_HIP && c.msg == text);
            const size_t stop = bad == over ? 4 : bad == empty_seg ? 1 : 2;
            for (size_t g = 0; g <= n; ++g) EXPECT(off[g] == (g <= stop ? iso_off[g] : 0));
        }
    }

    // the keys.  Segment 2 (pairs 0, 2, 3, 6; isoforms 0 and 1 kept, 2 and 3 behind the cut): isoform 0 has two direct reads, pairs 3
    // and 6 — the lower pair number wins, though its key is the larger; isoform 1 has no direct read, pair 0 being assigned: key 0;
    // pair 2 is direct in isoform 3, behind the cut.  Segment 0: pair 1 direct in isoform 1, pair 4 rare in group -1, isoform 0 without
    // reads.  Segment 4: pair 5 direct in isoform 0, pair 7 direct in isoform 1, which the cut leaves the segment without.
    const ioc_read_variants rd[] = {{0x11, 1, IOC_ISO_ASSIGNED},   {0x22, 1, IOC_ISO_DIRECT},  {0x33, 3, IOC_ISO_DIRECT}, {0x44, 0, IOC_ISO_DIRECT},
                                    {0x55, -1, IOC_ISO_RARE},      {0x66, 0, IOC_ISO_DIRECT},  {0x04, 0, IOC_ISO_DIRECT}, {0x88, 1, IOC_ISO_DIRECT}};
    const std::vector<uint64_t> keys = iso_keys(np, sop, rd, cut.n_iso.data(), iso_off.data(), n);
    std::vector<uint64_t> want(size_t(iso_off[n]), 0);
    std::vector<int> has(want.size(), 0);
    for (size_t i = 0; i < np; ++i) {  // (the restatement: in pair order, the first direct read of a kept isoform)
        const int32_t g = sop[i], h = rd[i].group;
        if (h < 0 || h >= (found[g] < max_iso ? found[g] : max_iso) || rd[i].how != IOC_ISO_DIRECT) continue;
        const size_t x = size_t(iso_off[g] + h);
        if (!has[x]) want[x] = rd[i].key2, has[x] = 1;
    }
    EXPECT(keys == want && keys == (std::vector<uint64_t>{0, 0x22, 0x44, 0, 0x66}));
    {  // an assigned read in front of the direct one does not speak for the isoform
        const ioc_read_variants two[] = {{0x7, 0, IOC_ISO_ASSIGNED}, {0x9, 0, IOC_ISO_DIRECT}};
        const int32_t s0[] = {0, 0}, n1[] = {1};
        const int64_t o1[] = {0, 1};
        EXPECT(iso_keys(2, s0, two, n1, o1, 1) == std::vector<uint64_t>{0x9});
    }
    EXPECT(iso_keys(0, nullptr, nullptr, nullptr, &zero, 0).empty());

    // a key's mask against blocks_state_mask state by state, and the full masks against blocks_full_mask: n_blocks 0, 1, 31, 32
    const uint64_t some[] = {0, ~uint64_t(0), 0x5555555555555555ull, 0xAAAAAAAAAAAAAAAAull, 0xC000000000000003ull, 0x3ull << 60, 0x1B1B1B1B1B1B1B1Bull, 0xE4E4E4E4E4E4E4E4ull};
    for (const uint64_t key : some)
        for (const uint32_t nb : {0u, 1u, 2u, 31u, 32u}) {
            uint64_t m = 0;
            for (uint32_t b = 0; b < nb; ++b) m |= blocks_state_mask(b, uint32_t(key >> (2u * b)) & 3u);
            EXPECT(blocks_key_mask(key, nb) == m && (m & ~blocks_full_mask(nb)) == 0);
        }
    EXPECT(blocks_key_mask(~uint64_t(0), 32) == 0 && blocks_key_mask(0, 32) == ~uint64_t(0) && blocks_key_mask(0, 31) == ~uint64_t(0) >> 2);
    EXPECT(blocks_key_mask(uint64_t(IOC_BLOCK_NONE) << 2 | IOC_BLOCK_SKIP, 3) == 0x33);  // (NONE at block 1 between two states)
    const ioc_blocks_seg none_seg{};
    std::vector<ioc_blocks_seg> bs(4, none_seg);
    bs[1].n_blocks = 31, bs[2].n_blocks = 32, bs[3].n_blocks = 1;
    const std::vector<uint64_t> full = blocks_pre_full(bs.size(), bs.data());
    for (size_t g = 0; g < bs.size(); ++g) EXPECT(full[g] == blocks_full_mask(uint32_t(bs[g].n_blocks)));
    EXPECT(full == (std::vector<uint64_t>{0, ~uint64_t(0) >> 2, ~uint64_t(0), 3}) && blocks_pre_full(0, nullptr).empty());
}

}  // namespace

int main()
{
    check_routes();
    check_arena();
    check_member_lists();
    check_group_member_lists();
    check_split_tables();
    check_slot_tables();
    check_bounds();
    check_plan_rlen();
    check_plan_pool();
    check_block_lists();
    for (const Kind& k : KINDS) {
        Caller c(k);
        g_what = k.name;
        const uint64_t per_row = k.pile == PileKind::none     ? 0
                                 : k.pile == PileKind::counts ? sizeof(ioc_pileup_col)
                                 : k.pile == PileKind::ins    ? sizeof(ioc_pileup_col) + sizeof(ioc_pileup_ins)
                                                              : 2 * sizeof(ioc_pileup_col) + sizeof(ioc_pileup_ins);
        // the planes: a byte per row and pair each, two of them, six more with project_ins and seven more with project_weights
        const uint64_t planes = k.project == 3 ? 3 + 2 * IOC_PILE_INS_SLOTS : k.project == 2 ? 2 + IOC_PILE_INS_SLOTS : k.project == 1 ? 2 : 0;
        EXPECT(c.sink.pile_bytes() == 700 * per_row + planes * uint64_t(Caller::PLANE_BYTES));
        EXPECT(c.sink.reduced() == (k.kind == SinkKind::reduced) && c.sink.has_stats() == k.stats && c.sink.has_pile() == (k.pile != PileKind::none));
        check_subset(k, {}, {}, {});
        check_subset(k, {}, {}, {1, 4});
        check_subset(k, {3}, {}, {});
        check_subset(k, {3}, {0}, {});     // (the re-run has no answer either)
        check_subset(k, {3}, {}, {3});     // (piled before the re-run)
        check_subset(k, {3}, {0}, {3});    // (... and stays so though the re-run says nothing)
        check_subset(k, {0, 1, 2, 3, 4, 5}, {}, {});
        check_subset(k, {0, 1, 2, 3, 4, 5}, {1, 4}, {0, 4});
        check_subset(k, {5, 0, 3}, {}, {});
        check_subset(k, {5, 0, 3}, {1}, {0, 2});
        check_subset(k, {4, 2, 5, 1}, {0, 3}, {5, 1, 3});
        check_empty(k);
        check_layout(k);
    }
    if (!g_ok) return 1;
    printf("ok: %ld checks of subset / take_back, answer_empty, ops_layout over %zu sink kinds, the routes and the sink plans\n", g_checks, sizeof KINDS / sizeof KINDS[0]);
    return 0;
}
