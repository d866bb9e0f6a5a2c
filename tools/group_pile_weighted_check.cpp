// group_pile_weighted_check.cpp — the indexing of k_ops_project_weights and k_group_pile_weighted
// (isonclust2_amd/csrc/ioc_group_pile_weighted.hip), restated lane by lane on the CPU and compared with the definitions in
// ioc_align.cpp:
//
//  * k_ops_project_weights' walk — PileAcc (ioc_ops_pileup.h) in 64-byte steps from the aligned-down address at every head
//    offset 0 .. 3, the lane of a '=' / 'X', of a 'D' and of an 'I' below IOC_PILE_INS_SLOTS storing its weight into plane
//    weight_plane_base / weight_plane_slot of the seven weight planes, the quality bytes read inside the pair's own qlen bytes
//    only — against ioc_host_ops_project_weights: runs of 0, 1, 5, 6, 7, 13 and 70 'I' at every position of a step, a 'D' at
//    both ends of the query, qlen 0 and 1, quality bytes 0, 33, 34, 35, 126 and 255 among random ones.  Every plane byte that the
//    definition sets has exactly one writer, every other byte none, and every read of the quality bytes is bounds-checked;
//  * k_group_pile_weighted's walk as tools/group_pile_check.cpp restates k_group_pile's — the group's own member list interleaved
//    over IOC_GROUP_PILE_WAVES waves, IOC_GROUP_PILE_AHEAD steps known ahead, the steps two by two, fourteen bytes a member and
//    lane, GPW_ACC counters a lane, the counters of waves 1 .. through an "LDS" block of exactly the kernel's size
//    (group_pile_weighted_lds_words) at plane_part_at, wave 0 adding them in wave order and writing its row of the three tables —
//    against ioc_host_planes_pile (gcols) and ioc_host_planes_pile_weighted (gwcols, gwins) over the members of every group, on
//    the shapes of tools/group_pile_check.cpp with weight bytes from 0, 1, 2, 40, 93 and 255.  Every read is bounds-checked, every
//    position of a list is read exactly once by exactly one wave, every LDS word and every table word has exactly one writer,
//    the rows of a group without reads none.
//
// Host code only; meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/group_pile_weighted_check tools/group_pile_weighted_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/group_pile_weighted_check
//
// Exit status 0 and "ok" when everything agrees.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ioc_group_pile_weighted.h"
#include "ioc_pile_call.h"
#include "ioc_sink_plan.h"
#include "isonclust2_hip.h"

namespace {

constexpr uint32_t SLOTS = IOC_PILE_INS_SLOTS, WP = IOC_WEIGHT_PLANES;
long g_strings = 0, g_run_over_edge = 0, g_items = 0, g_members = 0, g_gsegs = 0;

// k_ops_project_weights' loop over one string that stands `head` bytes behind a dword boundary: the pair's planes start at byte 0
// of planes of rlen + 1 bytes, its qualities at byte 0 of a pool of qlen bytes; `writers` counts the stores per byte
int drive_project(const std::string& ops, const std::vector<uint8_t>& qual, uint32_t rlen, uint32_t head, std::vector<uint8_t>& planes, std::vector<uint8_t>& writers)
{
    int faults = 0;
    const uint64_t plane_bytes = uint64_t(rlen) + 1u, pool_bytes = qual.size(), qo = 0, po = 0;
    const uint32_t q_len = uint32_t(qual.size());
    const uint32_t qn = qo >= pool_bytes ? 0u : uint32_t(pool_bytes - qo < uint64_t(q_len) ? pool_bytes - qo : uint64_t(q_len));
    // the quality bytes as the kernel may read them: del_weight and the lanes below index [0, qn) only — a copy of exactly qn
    // bytes, so that the sanitizer sees any read beside it
    std::vector<uint8_t> qq_store(qual.begin(), qual.begin() + qn);
    const uint8_t* qq = qq_store.data();
    const uint32_t span = head + uint32_t(ops.size());
    const uint32_t nsteps = (((span + 3u) / 4u + 63u) / 64u) * 4u;
    auto mask = [&](uint32_t step, char what) {
        unsigned long long m = 0;
        for (uint32_t l = 0; l < 64u; ++l) {
            const uint32_t pos = step * 64u + l;
            const char b = (pos >= head && pos < span) ? ops[pos - head] : char(0);
            if (b == what) m |= 1ull << l;
        }
        return m;
    };
    auto store = [&](uint32_t k, uint64_t at_row, uint32_t w) {
        const size_t to = size_t(uint64_t(k) * plane_bytes + at_row);
        planes.at(to) = uint8_t(w);
        ++writers.at(to);
    };
    PileAcc acc;
    for (uint32_t s = 0; s < nsteps; ++s) {
        acc.begin(mask(s, '='), mask(s, 'X'), mask(s, 'I'), mask(s, 'D'), mask(s, 'i'), mask(s, 'd'));
        for (uint32_t l = 0; l < 64u; ++l) {
            const uint64_t at_row = po + acc.row(l);
            const uint32_t qp = acc.qpos(l);
            const bool votes = acc.is_base(l) || acc.is_del(l) || acc.is_ins(l);
            if (votes && at_row >= plane_bytes) {  // (the kernel skips these; a string of its pair never asks for one)
                ++faults;
                continue;
            }
            if (at_row >= plane_bytes) continue;
            if (acc.is_base(l)) {
                if (qp < qn) store(weight_plane_base(), at_row, pile_qual_weight(qq[qp]));
                else ++faults;
            } else if (acc.is_del(l)) {
                store(weight_plane_base(), at_row, acc.del_weight(l, qn, qq));
            } else if (acc.is_ins(l)) {
                const uint32_t k = acc.ins_index(l);
                if (k >= SLOTS) continue;
                if (qp < qn) store(weight_plane_slot(k), at_row, pile_qual_weight(qq[qp]));
                else ++faults;
            }
        }
        acc.end_len();
        acc.end();
    }
    return faults;
}

bool check_string(const std::string& ops, std::mt19937& rng, bool one_run)
{
    uint32_t qlen = 0, rlen = 0;
    for (char b : ops) {
        qlen += b == '=' || b == 'X' || b == 'I' || b == 'i';
        rlen += b == '=' || b == 'X' || b == 'D' || b == 'd';
    }
    std::string query(qlen, 'A');
    std::vector<uint8_t> qual(qlen);
    for (uint8_t& b : qual) b = rng() % 3u ? uint8_t(rng() % 256u) : uint8_t("\0\41\42\43\176\377"[rng() % 6u]);
    const size_t rows = size_t(rlen) + 1u, bytes = size_t(WP) * rows;
    std::vector<uint8_t> want(bytes, 0xEE);
    if (ioc_host_ops_project_weights(ops.data(), int64_t(ops.size()), query.data(), reinterpret_cast<const char*>(qual.data()), int32_t(qlen), int32_t(rlen), want.data(),
                                     want.data() + rows) != IOC_OK) {
        fprintf(stderr, "the definition refused a string of %zu bytes\n", ops.size());
        return false;
    }
    // which bytes the definition sets (a weight is never 0)
    for (uint32_t head = 0; head < 4u; ++head) {
        std::vector<uint8_t> got(bytes, 0), writers(bytes, 0);
        const int faults = drive_project(ops, qual, rlen, head, got, writers);
        ++g_strings;
        if (faults || (one_run && got != want)) {
            fprintf(stderr, "mismatch: %zu bytes, head %u, %d faults: %.120s\n", ops.size(), head, faults, ops.c_str());
            return false;
        }
        for (size_t x = 0; x < bytes; ++x) {
            if (one_run && writers[x] != (want[x] ? 1u : 0u)) {
                fprintf(stderr, "byte %zu has %u writers: %.120s\n", x, unsigned(writers[x]), ops.c_str());
                return false;
            }
            // (two runs in front of one row: the definition overwrites in string order, the lanes in any — the same bytes are touched)
            if (!one_run && (writers[x] != 0u) != (want[x] != 0u)) return false;
        }
        for (size_t x = 1; x < ops.size(); ++x) g_run_over_edge += ops[x] == 'I' && ops[x - 1] == 'I' && (head + x) % 64u == 0u;
    }
    return true;
}

struct GroupCase {
    std::vector<int32_t> rlen, n_groups;      // per segment
    std::vector<int32_t> seg_of_pair, group;  // per pair
};

struct Bytes { uint32_t b, sl[SLOTS], wb, wsl[SLOTS]; };

bool check_pile(const GroupCase& gc, std::mt19937& rng)
{
    const size_t n = gc.rlen.size(), np = gc.seg_of_pair.size();
    // the host's side of groups_pile: planes, lists, group-segments, work items
    std::vector<uint64_t> plane(np);
    uint64_t P = 0;
    for (size_t i = 0; i < np; ++i) plane[i] = P, P += uint64_t(gc.rlen[size_t(gc.seg_of_pair[i])]) + 1u;
    std::vector<uint8_t> base(P), slots(size_t(SLOTS) * P), weights(size_t(WP) * P);
    for (uint8_t& b : base) b = "\0\1\2\3\4\5\7\7\7"[rng() % 9u];
    for (uint8_t& s : slots) s = rng() % 3u ? 0 : uint8_t(rng() % 6u);
    for (uint8_t& w : weights) w = uint8_t("\0\1\2\50\135\377"[rng() % 6u]);  // 0, 1, 2, 40, 93, 255: whatever byte a plane holds is added
    const GroupMemberLists m = group_member_lists(n, np, gc.seg_of_pair.data(), gc.group.data(), gc.n_groups.data());
    const size_t G = m.gseg_off.at(n), M = m.gmembers.size();
    if (m.gmem_off.size() != G + 1 || m.gmem_off.at(G) != M) return false;
    std::vector<IocPileSeg> gsegs(G);
    int64_t n_rows = 0;
    for (size_t g = 0; g < n; ++g)
        for (size_t x = m.gseg_off[g]; x < m.gseg_off[g + 1]; ++x) gsegs[x] = IocPileSeg{n_rows, 0, gc.rlen[g], 0}, n_rows += int64_t(gc.rlen[g]) + 1;
    std::vector<IocGroupWork> work;
    for (size_t x = 0; x < G; ++x)
        for (int64_t row = 0; m.gmem_off[x + 1] > m.gmem_off[x] && row <= int64_t(gsegs[x].rlen); row += IOC_GROUP_PILE_ROWS)
            work.push_back(IocGroupWork{uint32_t(x), uint32_t(row)});
    g_gsegs += long(G);

    // the definitions
    std::vector<ioc_pileup_col> want_c(size_t(n_rows), ioc_pileup_col{}), got_c = want_c, want_wc = want_c, got_wc = want_c;
    std::vector<ioc_pileup_ins> unused_i(size_t(n_rows), ioc_pileup_ins{}), want_wi = unused_i, got_wi = unused_i;
    for (size_t i = 0; i < np; ++i) {
        const size_t g = size_t(gc.seg_of_pair[i]), rows = size_t(gc.rlen[g]) + 1u;
        if (gc.group[i] < 0 || gc.group[i] >= gc.n_groups[g]) continue;
        std::vector<uint8_t> mine(size_t(SLOTS) * rows), wmine(size_t(SLOTS) * rows);  // (the definitions' layout: slot-major over the pair's own rows)
        for (size_t j = 0; j < SLOTS; ++j) {
            memcpy(mine.data() + j * rows, slots.data() + j * P + plane[i], rows);
            memcpy(wmine.data() + j * rows, weights.data() + size_t(weight_plane_slot(uint32_t(j))) * P + plane[i], rows);
        }
        const IocPileSeg& gs = gsegs.at(m.gseg_off[g] + size_t(gc.group[i]));
        if (ioc_host_planes_pile(base.data() + plane[i], mine.data(), gc.rlen[g], want_c.data() + gs.row0, unused_i.data() + gs.row0) != IOC_OK) return false;
        if (ioc_host_planes_pile_weighted(base.data() + plane[i], mine.data(), weights.data() + size_t(weight_plane_base()) * P + plane[i], wmine.data(), gc.rlen[g],
                                          want_wc.data() + gs.row0, want_wi.data() + gs.row0) != IOC_OK)
            return false;
        ++g_members;
    }

    // the kernel, work item by work item
    constexpr uint32_t W = IOC_GROUP_PILE_WAVES, ACC = GPW_ACC;
    const uint32_t n_members = uint32_t(M), n_pairs = uint32_t(np);
    // gpw_load: the fourteen bytes at row p of the member whose planes start at at0, or bytes that add nothing
    auto load = [&](uint64_t at0, uint32_t p, bool live) {
        Bytes v;
        v.b = group_pile_no_base(), v.wb = 0u;
        for (uint32_t j = 0; j < SLOTS; ++j) v.sl[j] = 0u, v.wsl[j] = 0u;
        if (at0 == group_pile_no_plane()) return v;
        const uint64_t at = at0 + p;
        if (live && at < P) {
            v.b = base.at(size_t(at));
            v.wb = weights.at(size_t(uint64_t(weight_plane_base()) * P + at));
            for (uint32_t j = 0; j < SLOTS; ++j) {
                v.sl[j] = slots.at(size_t(uint64_t(j) * P + at));
                v.wsl[j] = weights.at(size_t(uint64_t(weight_plane_slot(j)) * P + at));
            }
        }
        return v;
    };
    // gpw_add
    auto add = [&](uint32_t* c, const Bytes& v) {
        for (uint32_t k = 0; k < 6u; ++k) {
            c[GPW_COUNT + k] += uint32_t(plane_base_adds(v.b, k));
            c[GPW_WBASE + k] += plane_base_weighs(v.b, v.wb, k);
        }
        for (uint32_t j = 0; j < SLOTS; ++j) {
            const uint32_t in = uint32_t(plane_slot_inserts(v.sl[j]));
            c[GPW_BASES] += in;
            if (j == 0u) c[GPW_RUNS] += in;
            for (uint32_t ch = 0; ch < 5u; ++ch) c[GPW_WSLOT + j * 5u + ch] += plane_slot_weighs(v.sl[j], v.wsl[j], ch);
        }
    };
    std::vector<uint32_t> wrote_c(size_t(n_rows), 0), wrote_wc(size_t(n_rows), 0), wrote_wi(size_t(n_rows), 0);
    for (const IocGroupWork& wk : work) {
        ++g_items;
        if (wk.gseg >= G) return false;
        std::vector<uint32_t> part(group_pile_weighted_lds_words(), 0xDEADBEEFu), part_writers(part.size(), 0);
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
                const uint32_t nn = std::min<uint32_t>(IOC_GROUP_PILE_AHEAD, steps - t0);
                for (uint32_t s2 = 0; s2 < nn; s2 += IOC_GROUP_PILE_FLIGHT) {
                    const uint64_t a0 = mine[s2], a1 = s2 + 1u < nn ? mine[s2 + 1u] : group_pile_no_plane();  // (readlane: s2 + 1 < 64 where it is read)
                    for (uint32_t lane = 0; lane < 64u; ++lane) {
                        const uint32_t p = wk.row + lane;
                        const bool live = p <= uint32_t(s.rlen);
                        uint32_t* c = &cnt[wave][size_t(lane) * ACC];
                        const Bytes cur = load(a0, p, live), nxt = load(a1, p, live);  // (both in flight before either is added)
                        add(c, cur), add(c, nxt);
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
            ioc_pileup_col col{}, wcol{};
            ioc_pileup_ins win{};
            col.a = c[GPW_COUNT + 0u], col.c = c[GPW_COUNT + 1u], col.g = c[GPW_COUNT + 2u], col.t = c[GPW_COUNT + 3u], col.other = c[GPW_COUNT + 4u];
            col.del = c[GPW_COUNT + 5u], col.ins_runs = c[GPW_RUNS], col.ins_bases = c[GPW_BASES];
            wcol.a = c[GPW_WBASE + 0u], wcol.c = c[GPW_WBASE + 1u], wcol.g = c[GPW_WBASE + 2u], wcol.t = c[GPW_WBASE + 3u], wcol.other = c[GPW_WBASE + 4u];
            wcol.del = c[GPW_WBASE + 5u];
            for (uint32_t j = 0; j < SLOTS; ++j)
                for (uint32_t ch = 0; ch < 5u; ++ch) win.slot[j][ch] = c[GPW_WSLOT + j * 5u + ch];
            got_c.at(size_t(row)) = col, got_wc.at(size_t(row)) = wcol, got_wi.at(size_t(row)) = win;
            ++wrote_c.at(size_t(row)), ++wrote_wc.at(size_t(row)), ++wrote_wi.at(size_t(row));
        }
    }
    for (size_t x = 0; x < G; ++x)
        for (int64_t r = 0; r <= int64_t(gsegs[x].rlen); ++r) {
            const uint32_t want = m.gmem_off[x + 1] > m.gmem_off[x] ? 1u : 0u;
            const size_t at = size_t(gsegs[x].row0 + r);
            if (wrote_c[at] != want || wrote_wc[at] != want || wrote_wi[at] != want) {
                fprintf(stderr, "row %lld of group-segment %zu has %u writers, not %u\n", (long long)r, x, wrote_c[at], want);
                return false;
            }
        }
    if (n_rows > 0 && (memcmp(got_c.data(), want_c.data(), size_t(n_rows) * sizeof(ioc_pileup_col)) != 0 ||
                       memcmp(got_wc.data(), want_wc.data(), size_t(n_rows) * sizeof(ioc_pileup_col)) != 0 ||
                       memcmp(got_wi.data(), want_wi.data(), size_t(n_rows) * sizeof(ioc_pileup_ins)) != 0)) {
        fprintf(stderr, "the tables differ from the definitions': %zu segments, %zu pairs\n", n, np);
        return false;
    }
    return true;
}

}  // namespace

int main()
{
    std::mt19937 rng(20261020u);
    // runs of 0, 1, 5, 6, 7, 13 and 70 at every position of a step, between bases and deletions; a 'D' at both ends of the query
    for (uint32_t run : {0u, 1u, 5u, 6u, 7u, 13u, 70u})
        for (uint32_t before = 0; before < 130u; ++before) {
            std::string ops = before % 2u ? "D" : "";
            for (uint32_t x = 0; x < before; ++x) ops += "=X=D"[rng() % 4u];
            ops += std::string(run, 'I') + "=D=" + std::string(run, 'I') + (before % 3u ? "D" : "");
            if (!check_string(ops, rng, true)) return 1;
        }
    for (const char* ops : {"", "DD", "ddd", "=", "I", "D=D", "d=D", "ii=D=I=dd", "DDI"})
        if (!check_string(ops, rng, true)) return 1;
    if (!check_string(std::string(70, 'I'), rng, true) || !check_string("IIIiI=", rng, false)) return 1;
    for (int t = 0; t < 300; ++t) {
        std::string ops;
        const uint32_t len = rng() % 700u;
        bool one_run = true, seen = false;  // (seen: a run of 'I' stands in front of the current row already)
        for (uint32_t x = 0; x < len; ++x) {
            const char b = "====XXIIIDDid"[rng() % 13u];
            if (b == 'I') {
                if (seen && (ops.empty() || ops.back() != 'I')) one_run = false;
                seen = true;
            } else if (b != 'i') {
                seen = false;
            }
            ops += b;
        }
        if (!check_string(ops, rng, one_run)) return 1;
    }
    if (g_run_over_edge == 0) {
        fprintf(stderr, "no run went over the edge of a step\n");
        return 1;
    }

    static_assert(IOC_PILE_CALL_CHUNK == 256 && IOC_GROUP_PILE_ROWS == 64 && IOC_GROUP_PILE_WAVES == 4 && IOC_GROUP_PILE_FLIGHT == 2 && IOC_GROUP_PILE_AHEAD == 64,
                  "the sizes below are placed around these");
    const std::vector<int32_t> lens = {0, 1, 62, 63, 64, 65, 127, 128, 255, 256, 257, 600};
    // every group of a segment `members` pairs, 0 .. 5 groups a segment in turn, a pair in -1 per segment, the segments' pairs interleaved
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
    printf("ok: %ld drives of k_ops_project_weights' walk (%ld runs over a step's edge), %ld work items of k_group_pile_weighted over %ld group-segments and %ld members\n",
           g_strings, g_run_over_edge, g_items, g_gsegs, g_members);
    return 0;
}
