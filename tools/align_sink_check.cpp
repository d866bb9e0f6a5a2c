// align_sink_check.cpp — the host side of the aligner's sink description (isonclust2_amd/csrc/ioc_align_sink.h), driven on the CPU:
//
//  * AlnSink::subset / take_back, which decide what a re-run (every tile, version 1) sees of the caller's pairs and what it leaves
//    them: for every sink kind, idx empty, one pair, all pairs, out of order — a pair piled before the re-run stays piled and its
//    row_base reaches the re-run unchanged (ops_reserve turns it into -1 from `piled`), a pair the re-run leaves unanswered keeps
//    len == 0 and piled == 0, the records of pairs outside idx are untouched, the bytes' regions are the caller's own; a pile
//    that projects (project, project_ins) hands the re-run its pairs' plane offsets, the planes' addresses and both flags;
//  * AlnSink::answer_empty, the closed forms of a pair with an empty sequence, for every kind and both empty sides;
//  * ops_layout, the per-slice table's offsets: those the kernels' launchers have always been handed, for np in {0, 1, 3, 5, 1000};
//  * aln_route and the accepted parameter range, at their edges and with the extreme values an int32 argument can carry (no
//    overflow on the way: the sums are 64-bit).
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
#include <vector>

#include "ioc_align_sink.h"

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
    int project = 0;  // 1: the pile projects (two planes); 2: and what the pairs insert (project_ins: six more)
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
                      {"counts+project_ins+stats", SinkKind::reduced, true, PileKind::counts, 2}};

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
            if (k.project == 2) sink.pile.project_ins = true, sink.pile.slot_planes = t_planes + 2;
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
    EXPECT(s.projects() == (k.project != 0) && s.projects_ins() == (k.project == 2));
    if (k.project) {
        EXPECT(sub.plane.size() == idx.size() && s.pile.plane == sub.plane.data() && s.pile.plane_bytes == Caller::PLANE_BYTES);
        EXPECT(s.pile.base_planes == c.sink.pile.base_planes && s.pile.ins_planes == c.sink.pile.ins_planes && s.pile.slot_planes == c.sink.pile.slot_planes);
        EXPECT((s.pile.slot_planes != nullptr) == (k.project == 2));
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
    // (project_ins adds no column: the slot planes sit at the pair's `plane` offset like the two)
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

}  // namespace

int main()
{
    check_routes();
    for (const Kind& k : KINDS) {
        Caller c(k);
        g_what = k.name;
        const uint64_t per_row = k.pile == PileKind::none     ? 0
                                 : k.pile == PileKind::counts ? sizeof(ioc_pileup_col)
                                 : k.pile == PileKind::ins    ? sizeof(ioc_pileup_col) + sizeof(ioc_pileup_ins)
                                                              : 2 * sizeof(ioc_pileup_col) + sizeof(ioc_pileup_ins);
        // the planes: a byte per row and pair each, two of them, and six more with project_ins
        const uint64_t planes = k.project == 2 ? 2 + IOC_PILE_INS_SLOTS : k.project == 1 ? 2 : 0;
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
    printf("ok: %ld checks of subset / take_back, answer_empty, ops_layout over %zu sink kinds, and the routes\n", g_checks, sizeof KINDS / sizeof KINDS[0]);
    return 0;
}
