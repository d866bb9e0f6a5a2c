// group_pile_check.cpp — the indexing of k_group_pile (isonclust2_amd/csrc/ioc_group_pile.hip), restated lane by lane on the CPU
// and compared with the definition in ioc_align.cpp:
//
//  * the host's side as the stage has it (SinkRun::groups_pile): every group's own member list from group_member_lists
//    (ioc_sink_plan.h), the group-segments in segment order with their rows one behind the other, a work item per 64 rows of a
//    group-segment that has reads;
//  * the kernel's walk — IOC_GROUP_PILE_WAVES waves taking the group's list interleaved at group_pile_at, group_pile_steps steps
//    each, IOC_GROUP_PILE_AHEAD steps at a time: lane l of the wave reads where the member of step l of the chunk has its planes
//    (group_pile_no_plane for a step behind the list), every step takes its offset from that lane, and the steps go two by two,
//    the bytes of the NEXT member read before the current member's are added (a step that reads nothing holds
//    group_pile_no_base / 0), a lane per row, the counters of waves 1 .. through an "LDS" block of exactly the kernel's size at
//    plane_part_at, wave 0 adding them in wave order and writing its row — against ioc_host_planes_pile over the members of
//    every group: segments of 0, 1, 62 .. 65, 127, 128, 255 .. 257 and 600 rows' length, 0, 1, 2, 3, 5 and 70 groups a segment,
//    groups of 0 to 9, 65, 130 and 255 to 261 members (around the four waves, the eight members of a round and the 256 members of a
//    workgroup's chunks), pairs in -1, a segment whose
//    pairs are all in -1, a segment with pairs but no groups, the segments' pairs interleaved.  Every read of the planes, the
//    lists and the tables is bounds-checked, every member must be read exactly once by exactly one wave, every LDS word and every
//    table word must have exactly one writer, the rows of a group without reads none.
//
// Host code only; meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/group_pile_check tools/group_pile_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/group_pile_check
//
// Exit status 0 and "ok" when everything agrees.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "ioc_group_pile.h"
#include "ioc_pile_call.h"
#include "ioc_sink_plan.h"
#include "isonclust2_hip.h"

namespace {

constexpr uint32_t SLOTS = IOC_PILE_INS_SLOTS;
long g_items = 0, g_members = 0, g_gsegs = 0;

struct GroupCase {
    std::vector<int32_t> rlen, n_groups;      // per segment
    std::vector<int32_t> seg_of_pair, group;  // per pair
};

struct Bytes { uint32_t b, sl[SLOTS]; };

bool check_pile(const GroupCase& gc, std::mt19937& rng)
{
    const size_t n = gc.rlen.size(), np = gc.seg_of_pair.size();
    // the host's side of groups_pile: planes, lists, group-segments, work items
    std::vector<uint64_t> plane(np);
    uint64_t P = 0;
    for (size_t i = 0; i < np; ++i) plane[i] = P, P += uint64_t(gc.rlen[size_t(gc.seg_of_pair[i])]) + 1u;
    std::vector<uint8_t> base(P), slots(size_t(SLOTS) * P);
    for (uint8_t& b : base) b = "\0\1\2\3\4\5\7\7\7"[rng() % 9u];
    for (uint8_t& s : slots) s = rng() % 3u ? 0 : uint8_t(rng() % 6u);
    const GroupMemberLists m = group_member_lists(n, np, gc.seg_of_pair.data(), gc.group.data(), gc.n_groups.data());
    const size_t G = m.gseg_off.at(n), M = m.gmembers.size();
    if (m.gmem_off.size() != G + 1 || m.gmem_off.at(G) != M) return false;
    // the lists' own semantics: ascending pairs, every pair of a group in its list and in no other, -1 in none
    {
        std::vector<uint32_t> listed(np, 0);
        for (size_t g = 0; g < n; ++g)
            for (size_t x = m.gseg_off[g]; x < m.gseg_off[g + 1]; ++x)
                for (uint32_t at = m.gmem_off[x]; at < m.gmem_off[x + 1]; ++at) {
                    const uint32_t i = m.gmembers.at(at);
                    if (i >= np || size_t(gc.seg_of_pair[i]) != g || size_t(gc.group[i]) != x - m.gseg_off[g] || (at > m.gmem_off[x] && m.gmembers[at - 1] >= i)) {
                        fprintf(stderr, "member %u of group-segment %zu does not belong there\n", i, x);
                        return false;
                    }
                    ++listed[i];
                }
        for (size_t i = 0; i < np; ++i)
            if (listed[i] != (gc.group[i] >= 0 && gc.group[i] < gc.n_groups[size_t(gc.seg_of_pair[i])] ? 1u : 0u)) {
                fprintf(stderr, "pair %zu is in %u lists\n", i, listed[i]);
                return false;
            }
    }
    std::vector<IocPileSeg> gsegs(G);
    int64_t n_rows = 0;
    for (size_t g = 0; g < n; ++g)
        for (size_t x = m.gseg_off[g]; x < m.gseg_off[g + 1]; ++x) gsegs[x] = IocPileSeg{n_rows, 0, gc.rlen[g], 0}, n_rows += int64_t(gc.rlen[g]) + 1;
    std::vector<IocGroupWork> work;
    for (size_t x = 0; x < G; ++x)
        for (int64_t row = 0; m.gmem_off[x + 1] > m.gmem_off[x] && row <= int64_t(gsegs[x].rlen); row += IOC_GROUP_PILE_ROWS)
            work.push_back(IocGroupWork{uint32_t(x), uint32_t(row)});
    g_gsegs += long(G);

    // the definition
    std::vector<ioc_pileup_col> want_c(size_t(n_rows), ioc_pileup_col{}), got_c = want_c;
    std::vector<ioc_pileup_ins> want_i(size_t(n_rows), ioc_pileup_ins{}), got_i = want_i;
    for (size_t i = 0; i < np; ++i) {
        const size_t g = size_t(gc.seg_of_pair[i]), rows = size_t(gc.rlen[g]) + 1u;
        if (gc.group[i] < 0 || gc.group[i] >= gc.n_groups[g]) continue;
        std::vector<uint8_t> mine(size_t(SLOTS) * rows);  // (the definition's layout: slot-major over the pair's own rows)
        for (size_t j = 0; j < SLOTS; ++j) memcpy(mine.data() + j * rows, slots.data() + j * P + plane[i], rows);
        const IocPileSeg& gs = gsegs.at(m.gseg_off[g] + size_t(gc.group[i]));
        if (ioc_host_planes_pile(base.data() + plane[i], mine.data(), gc.rlen[g], want_c.data() + gs.row0, want_i.data() + gs.row0) != IOC_OK) return false;
        ++g_members;
    }

    // the kernel, work item by work item
    constexpr uint32_t W = IOC_GROUP_PILE_WAVES, ACC = 6u + SLOTS * 5u;
    const uint32_t n_members = uint32_t(M), n_pairs = uint32_t(np);
    // gp_load: the bytes at row p of the member whose planes start at at0, or bytes that add nothing
    auto load = [&](uint64_t at0, uint32_t p, bool live) {
        Bytes v;
        v.b = group_pile_no_base();
        for (uint32_t j = 0; j < SLOTS; ++j) v.sl[j] = 0u;
        if (at0 == group_pile_no_plane()) return v;
        const uint64_t at = at0 + p;
        if (live && at < P) {
            v.b = base.at(size_t(at));
            for (uint32_t j = 0; j < SLOTS; ++j) v.sl[j] = slots.at(size_t(uint64_t(j) * P + at));
        }
        return v;
    };
    std::vector<uint32_t> wrote_c(size_t(n_rows), 0), wrote_i(size_t(n_rows), 0);
    for (const IocGroupWork& wk : work) {
        ++g_items;
        if (wk.gseg >= G) return false;
        std::vector<uint32_t> part(size_t(W - 1u) * ACC * 64u, 0xDEADBEEFu), part_writers(part.size(), 0);
        const IocPileSeg s = gsegs.at(wk.gseg);
        const uint32_t m0 = m.gmem_off.at(wk.gseg), m1 = std::min(m.gmem_off.at(wk.gseg + 1u), n_members);
        std::vector<uint32_t> reads(M, 0);  // how often a position of the list was read, by any lane of any wave
        std::vector<std::vector<uint32_t>> cnt(W, std::vector<uint32_t>(64u * ACC, 0));  // [wave][lane * ACC + counter]: the registers
        for (uint32_t wave = 0; wave < W; ++wave) {
            const uint32_t steps = group_pile_steps(m0, m1, wave);
            for (uint32_t t0 = 0; t0 < steps; t0 += IOC_GROUP_PILE_AHEAD) {
                uint64_t mine[64];  // the register `mine` of the wave's 64 lanes
                for (uint32_t lane = 0; lane < 64u; ++lane) {
                    mine[lane] = group_pile_no_plane();
                    if (t0 + lane >= steps) continue;
                    const uint32_t x = group_pile_at(m0, wave, t0 + lane);
                    if (x < m0 || x >= m1) return false;
                    const uint32_t i = m.gmembers.at(x);
                    ++reads.at(x);
                    if (i < n_pairs) mine[lane] = plane.at(i);
                }
                const uint32_t n = std::min<uint32_t>(IOC_GROUP_PILE_AHEAD, steps - t0);
                for (uint32_t s2 = 0; s2 < n; s2 += IOC_GROUP_PILE_FLIGHT) {
                    const uint64_t a0 = mine[s2], a1 = s2 + 1u < n ? mine[s2 + 1u] : group_pile_no_plane();  // (readlane: s2 + 1 < 64 where it is read)
                    for (uint32_t lane = 0; lane < 64u; ++lane) {
                        const uint32_t p = wk.row + lane;
                        const bool live = p <= uint32_t(s.rlen);
                        uint32_t* c = &cnt[wave][size_t(lane) * ACC];
                        const Bytes cur = load(a0, p, live), nxt = load(a1, p, live);  // (both in flight before either is added)
                        for (uint32_t v = 0; v < 6u; ++v) c[v] += uint32_t(plane_base_adds(cur.b, v)) + uint32_t(plane_base_adds(nxt.b, v));
                        for (uint32_t j = 0; j < SLOTS; ++j)
                            for (uint32_t ch = 0; ch < 5u; ++ch) c[6u + j * 5u + ch] += uint32_t(plane_slot_adds(cur.sl[j], ch)) + uint32_t(plane_slot_adds(nxt.sl[j], ch));
                    }
                }
            }
        }
        for (uint32_t x = 0; x < M; ++x)
            if (reads[x] != (x >= m0 && x < m1 ? 1u : 0u)) {
                fprintf(stderr, "member position %u was read %u times by the work item of group-segment %u\n", x, reads[x], wk.gseg);
                return false;
            }
        for (uint32_t wave = 1; wave < W; ++wave)
            for (uint32_t lane = 0; lane < 64u; ++lane)
                for (uint32_t k = 0; k < ACC; ++k) {
                    const size_t to = size_t(wave - 1u) * ACC * 64u + lane + plane_part_at(k);
                    part.at(to) = cnt[wave][size_t(lane) * ACC + k];
                    ++part_writers.at(to);
                }
        for (uint32_t w : part_writers)
            if (w != 1u) {
                fprintf(stderr, "an LDS word has %u writers\n", w);
                return false;
            }
        for (uint32_t lane = 0; lane < 64u; ++lane) {
            uint32_t* c = &cnt[0][size_t(lane) * ACC];
            for (uint32_t wave = 1; wave < W; ++wave)
                for (uint32_t k = 0; k < ACC; ++k) c[k] += part.at(size_t(wave - 1u) * ACC * 64u + lane + plane_part_at(k));
            const uint32_t p = wk.row + lane;
            const uint64_t row = uint64_t(s.row0) + p;
            if (p > uint32_t(s.rlen) || row >= uint64_t(n_rows)) continue;
            ioc_pileup_col col{};
            ioc_pileup_ins in{};
            col.a = c[0], col.c = c[1], col.g = c[2], col.t = c[3], col.other = c[4], col.del = c[5];
            for (uint32_t j = 0; j < SLOTS; ++j)
                for (uint32_t ch = 0; ch < 5u; ++ch) {
                    in.slot[j][ch] = c[6u + j * 5u + ch];
                    col.ins_bases += in.slot[j][ch];
                    if (j == 0u) col.ins_runs += in.slot[j][ch];
                }
            got_c.at(size_t(row)) = col, got_i.at(size_t(row)) = in;
            ++wrote_c.at(size_t(row)), ++wrote_i.at(size_t(row));
        }
    }
    for (size_t x = 0; x < G; ++x)
        for (int64_t r = 0; r <= int64_t(gsegs[x].rlen); ++r) {
            const uint32_t want = m.gmem_off[x + 1] > m.gmem_off[x] ? 1u : 0u;
            if (wrote_c[size_t(gsegs[x].row0 + r)] != want || wrote_i[size_t(gsegs[x].row0 + r)] != want) {
                fprintf(stderr, "row %lld of group-segment %zu has %u writers, not %u\n", (long long)r, x, wrote_c[size_t(gsegs[x].row0 + r)], want);
                return false;
            }
        }
    if ((n_rows > 0 && (memcmp(got_c.data(), want_c.data(), size_t(n_rows) * sizeof(ioc_pileup_col)) != 0 ||
                        memcmp(got_i.data(), want_i.data(), size_t(n_rows) * sizeof(ioc_pileup_ins)) != 0))) {
        fprintf(stderr, "the tables differ from the definition's: %zu segments, %zu pairs\n", n, np);
        return false;
    }
    return true;
}

}  // namespace

int main()
{
    std::mt19937 rng(20261020u);
    static_assert(IOC_PILE_CALL_CHUNK == 256 && IOC_GROUP_PILE_ROWS == 64 && IOC_GROUP_PILE_WAVES == 4 && IOC_GROUP_PILE_FLIGHT == 2 && IOC_GROUP_PILE_AHEAD == 64,
                  "the sizes below are placed around these");
    const std::vector<int32_t> lens = {0, 1, 62, 63, 64, 65, 127, 128, 255, 256, 257, 600};
    // every group of a segment `members` pairs, 0 .. 5 groups a segment in turn, a pair in -1 per segment, the segments' pairs interleaved
    // (255 .. 261 members: around the 64 steps of a chunk of each of the four waves, and one step into the next chunk)
    for (uint32_t members : {0u, 1u, 2u, 3u, 4u, 5u, 6u, 7u, 8u, 9u, 65u, 130u, 255u, 256u, 257u, 261u})
        for (int mix = 0; mix < 2; ++mix) {
            GroupCase gc;
            gc.rlen = lens;
            for (size_t g = 0; g < lens.size(); ++g) gc.n_groups.push_back(int32_t((g + size_t(mix)) % 6u));
            for (uint32_t k = 0; k <= members * 5u; ++k)
                for (size_t g = 0; g < lens.size(); ++g) {
                    const int32_t ng = gc.n_groups[g];
                    if (k > members * uint32_t(ng)) continue;
                    gc.seg_of_pair.push_back(int32_t(g));
                    gc.group.push_back(k == members * uint32_t(ng) ? -1 : mix == 0 ? int32_t(k % uint32_t(ng)) : int32_t(k / members));
                }
            if (!check_pile(gc, rng)) return 1;
        }
    {  // 70 groups of 0 .. 9 members, random membership; a segment whose pairs are all in -1; a segment with pairs but no groups
        GroupCase gc;
        gc.rlen = {256, 64, 65, 3};
        gc.n_groups = {70, 3, 0, 2};
        for (uint32_t k = 0; k < 330u; ++k) {
            gc.seg_of_pair.push_back(0), gc.group.push_back(int32_t(rng() % 71u) - 1);
            if (k < 7u) gc.seg_of_pair.push_back(1), gc.group.push_back(-1);
            if (k < 5u) gc.seg_of_pair.push_back(2), gc.group.push_back(-1);
            if (k < 9u) gc.seg_of_pair.push_back(3), gc.group.push_back(int32_t(k >= 8u));
        }
        if (!check_pile(gc, rng)) return 1;
    }
    if (!check_pile(GroupCase{}, rng) || !check_pile(GroupCase{{5, 0}, {3, 2}, {}, {}}, rng) || !check_pile(GroupCase{{5, 0}, {0, 0}, {0, 1}, {-1, -1}}, rng)) return 1;
    printf("ok: %ld work items of k_group_pile over %ld group-segments and %ld members\n", g_items, g_gsegs, g_members);
    return 0;
}
