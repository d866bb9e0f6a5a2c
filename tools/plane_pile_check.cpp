// plane_pile_check.cpp — the indexing of the two kernels of isonclust2_amd/csrc/ioc_plane_pile.hip, restated lane by lane on the
// CPU and compared with the definitions in ioc_align.cpp:
//
//  * PileAcc (ioc_ops_pileup.h) as k_ops_project_ins uses it — 64-byte steps from the aligned-down address at every head offset
//    0 .. 3, one "lane" per byte, the lane of an 'I' byte whose index in its run is below IOC_PILE_INS_SLOTS storing
//    plane_slot_byte(channel) into slot plane ins_index at its row — against ioc_host_ops_project_ins: runs of 0, 1, 6, 7 and 70
//    'I' bytes at every position of a step (on its first byte, on its last, across its edge), random strings.  The planes are
//    handed over in blocks of exactly their size, and every byte must have at most one writer;
//  * k_plane_pile's walk — a work item per 64 rows of a group-segment that has reads, IOC_PLANE_PILE_WAVES waves taking the
//    members interleaved, a lane per row, the counters of waves 1 .. through an "LDS" block of exactly the kernel's size at
//    plane_part_at, wave 0 adding them in wave order and writing its row — against ioc_host_planes_pile over the members of every
//    group: segments of 0, 1, 63, 64, 65, 255, 256, 257 rows' length (around the lanes of a work item and IOC_PILE_CALL_CHUNK),
//    0 to 9 and 65 members (around the waves' share), the three group bytes mixed, the segments' pairs interleaved.  Every LDS
//    word and every table word must have exactly one writer, the rows of a group without reads none.
//
// Host code only; meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iisonclust2_amd/csrc \
//       -o /tmp/plane_pile_check tools/plane_pile_check.cpp isonclust2_amd/csrc/ioc_align.cpp && /tmp/plane_pile_check
//
// Exit status 0 and "ok" when everything agrees.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ioc_pile_call.h"
#include "ioc_plane_pile.h"
#include "isonclust2_hip.h"

namespace {

constexpr uint32_t SLOTS = IOC_PILE_INS_SLOTS;

// k_ops_project_ins' loop over one string that stands `head` bytes behind a dword boundary; `writers` counts the stores per byte
int drive_project(const std::string& ops, const std::string& query, uint32_t rlen, uint32_t head, std::vector<uint8_t>& slots, std::vector<uint8_t>& writers)
{
    int faults = 0;
    const uint64_t plane_bytes = uint64_t(rlen) + 1u, pool_bytes = query.size();
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
    PileAcc acc;
    for (uint32_t s = 0; s < nsteps; ++s) {
        acc.begin(mask(s, '='), mask(s, 'X'), mask(s, 'I'), mask(s, 'D'), mask(s, 'i'), mask(s, 'd'));
        for (uint32_t l = 0; l < 64u; ++l) {
            if (!acc.is_ins(l)) continue;
            const uint64_t at_row = acc.row(l), at = acc.qpos(l);
            const uint32_t k = acc.ins_index(l);
            if (k >= SLOTS) continue;
            if (at_row >= plane_bytes || at >= pool_bytes) {  // (the kernel skips these; a string of its pair never asks for one)
                ++faults;
                continue;
            }
            const size_t to = size_t(uint64_t(k) * plane_bytes + at_row);
            slots.at(to) = uint8_t(plane_slot_byte(PileAcc::channel(uint8_t(query[size_t(at)]))));
            ++writers.at(to);
        }
        acc.end_len();
        acc.end();
    }
    return faults;
}

long g_strings = 0, g_run_over_edge = 0, g_first = 0, g_last = 0, g_items = 0, g_members = 0;

bool check_string(const std::string& ops, std::mt19937& rng, bool one_run)
{
    uint32_t qlen = 0, rlen = 0;
    for (char b : ops) {
        qlen += b == '=' || b == 'X' || b == 'I' || b == 'i';
        rlen += b == '=' || b == 'X' || b == 'D' || b == 'd';
    }
    std::string query(qlen, 'A');
    for (char& ch : query) ch = "ACGTACGTACGTNacR"[rng() % 16u];
    const size_t bytes = size_t(SLOTS) * (size_t(rlen) + 1u);
    std::vector<uint8_t> want(bytes, 0xEE);
    if (ioc_host_ops_project_ins(ops.data(), int64_t(ops.size()), query.data(), int32_t(qlen), int32_t(rlen), want.data()) != IOC_OK) {
        fprintf(stderr, "the definition refused a string of %zu bytes\n", ops.size());
        return false;
    }
    for (uint32_t head = 0; head < 4u; ++head) {
        std::vector<uint8_t> got(bytes, 0), writers(bytes, 0);
        const int faults = drive_project(ops, query, rlen, head, got, writers);
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
        for (size_t x = 0; x < ops.size(); ++x) {
            if (ops[x] != 'I') continue;
            const bool starts = x == 0 || ops[x - 1] != 'I';
            g_run_over_edge += !starts && (head + x) % 64u == 0u;
            g_first += starts && (head + x) % 64u == 0u;
            g_last += starts && (head + x) % 64u == 63u;
        }
    }
    return true;
}

// one call of k_plane_pile and what it must give
struct PileCase {
    std::vector<int32_t> rlen;          // per segment
    std::vector<int32_t> seg_of_pair;   // per pair
    std::vector<uint8_t> group;         // per pair
};

bool check_pile(const PileCase& pc, std::mt19937& rng)
{
    const size_t n = pc.rlen.size(), np = pc.seg_of_pair.size();
    // the host's side of group_polish_device: planes, lists, group-segments, work items
    std::vector<uint64_t> plane(np);
    uint64_t P = 0;
    for (size_t i = 0; i < np; ++i) plane[i] = P, P += uint64_t(pc.rlen[size_t(pc.seg_of_pair[i])]) + 1u;
    std::vector<uint8_t> base(P), slots(size_t(SLOTS) * P);
    for (uint8_t& b : base) b = "\0\1\2\3\4\5\7\7\7"[rng() % 9u];
    for (uint8_t& s : slots) s = rng() % 3u ? 0 : uint8_t(rng() % 6u);
    std::vector<uint32_t> mem_off(n + 1, 0), members(np), reads(2 * n, 0);
    for (size_t i = 0; i < np; ++i) ++mem_off[size_t(pc.seg_of_pair[i]) + 1];
    for (size_t g = 0; g < n; ++g) mem_off[g + 1] += mem_off[g];
    {
        std::vector<uint32_t> next(mem_off.begin(), mem_off.end() - 1);
        for (size_t i = 0; i < np; ++i) members[next[size_t(pc.seg_of_pair[i])]++] = uint32_t(i);
    }
    struct GSeg { int64_t row0; int32_t rlen; };
    std::vector<GSeg> gsegs(2 * n);
    int64_t n_rows = 0;
    for (size_t g = 0; g < n; ++g)
        for (int h = 0; h < 2; ++h) gsegs[2 * g + size_t(h)] = GSeg{n_rows, pc.rlen[g]}, n_rows += int64_t(pc.rlen[g]) + 1;
    for (size_t i = 0; i < np; ++i)
        if (pc.group[i] <= 1) ++reads[2 * size_t(pc.seg_of_pair[i]) + pc.group[i]];
    std::vector<IocPlaneWork> work;
    for (size_t x = 0; x < 2 * n; ++x)
        for (int64_t row = 0; reads[x] > 0 && row <= int64_t(gsegs[x].rlen); row += IOC_PLANE_PILE_ROWS) work.push_back(IocPlaneWork{uint32_t(x), uint32_t(row)});

    // the definition
    std::vector<ioc_pileup_col> want_c(size_t(n_rows), ioc_pileup_col{}), got_c = want_c;
    std::vector<ioc_pileup_ins> want_i(size_t(n_rows), ioc_pileup_ins{}), got_i = want_i;
    for (size_t i = 0; i < np; ++i) {
        if (pc.group[i] > 1) continue;
        const size_t g = size_t(pc.seg_of_pair[i]), rows = size_t(pc.rlen[g]) + 1u;
        std::vector<uint8_t> mine(size_t(SLOTS) * rows);  // (the definition's layout: slot-major over the pair's own rows)
        for (size_t j = 0; j < SLOTS; ++j) memcpy(mine.data() + j * rows, slots.data() + j * P + plane[i], rows);
        const GSeg& gs = gsegs[2 * g + pc.group[i]];
        if (ioc_host_planes_pile(base.data() + plane[i], mine.data(), pc.rlen[g], want_c.data() + gs.row0, want_i.data() + gs.row0) != IOC_OK) return false;
        ++g_members;
    }

    // the kernel, work item by work item
    constexpr uint32_t W = IOC_PLANE_PILE_WAVES, ACC = 6u + SLOTS * 5u;
    std::vector<uint32_t> wrote_c(size_t(n_rows), 0), wrote_i(size_t(n_rows), 0);
    for (const IocPlaneWork& wk : work) {
        ++g_items;
        std::vector<uint32_t> part(size_t(W - 1u) * ACC * 64u, 0xDEADBEEFu), part_writers(part.size(), 0);
        const uint32_t g = wk.gseg >> 1, h = wk.gseg & 1u;
        const GSeg s = gsegs.at(wk.gseg);
        std::vector<std::vector<uint32_t>> cnt(W, std::vector<uint32_t>(64u * ACC, 0));  // [wave][lane * ACC + counter]: the registers
        for (uint32_t wave = 0; wave < W; ++wave)
            for (uint32_t x = mem_off.at(g) + wave; x < mem_off.at(g + 1u); x += W) {
                const uint32_t i = members.at(x);
                if (i >= np || uint32_t(pc.group[i]) != h) continue;
                for (uint32_t lane = 0; lane < 64u; ++lane) {
                    const uint32_t p = wk.row + lane;
                    const uint64_t at = plane[i] + p;
                    if (p > uint32_t(s.rlen) || at >= P) continue;
                    uint32_t* c = &cnt[wave][size_t(lane) * ACC];
                    const uint32_t b = base.at(size_t(at));
                    for (uint32_t v = 0; v < 6u; ++v) c[v] += plane_base_adds(b, v);
                    for (uint32_t j = 0; j < SLOTS; ++j)
                        for (uint32_t ch = 0; ch < 5u; ++ch) c[6u + j * 5u + ch] += plane_slot_adds(slots.at(size_t(uint64_t(j) * P + at)), ch);
                }
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
    for (size_t x = 0; x < 2 * n; ++x)
        for (int64_t r = 0; r <= int64_t(gsegs[x].rlen); ++r) {
            const uint32_t want = reads[x] > 0 ? 1u : 0u;
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
    std::mt19937 rng(20261019u);
    // runs of 0, 1, 6, 7 and 70 at every position of a step; with the heads 0 .. 3 every run starts on a first and on a last byte
    for (uint32_t run : {0u, 1u, 6u, 7u, 70u})
        for (uint32_t before = 0; before < 130u; ++before) {
            std::string ops;
            for (uint32_t x = 0; x < before; ++x) ops += "=X=D"[rng() % 4u];
            ops += std::string(run, 'I') + "=D=" + std::string(run, 'I');
            if (!check_string(ops, rng, true)) return 1;
        }
    if (!check_string("", rng, true) || !check_string(std::string(70, 'I'), rng, true) || !check_string("IIIiI=", rng, false)) return 1;
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
    if (g_run_over_edge == 0 || g_first == 0 || g_last == 0) {
        fprintf(stderr, "the strings did not reach the edges of a step\n");
        return 1;
    }

    // k_plane_pile: rows around the work item's 64 and IOC_PILE_CALL_CHUNK, members around the waves' share
    static_assert(IOC_PILE_CALL_CHUNK == 256 && IOC_PLANE_PILE_ROWS == 64 && IOC_PLANE_PILE_WAVES == 4, "the sizes below are placed around these");
    const std::vector<int32_t> lens = {0, 1, 62, 63, 64, 65, 127, 128, 255, 256, 257};
    for (uint32_t members : {0u, 1u, 2u, 3u, 4u, 5u, 7u, 8u, 9u, 65u})
        for (int mix = 0; mix < 3; ++mix) {
            PileCase pc;
            pc.rlen = lens;
            for (uint32_t m = 0; m < members; ++m)
                for (size_t g = 0; g < lens.size(); ++g) {  // (the segments' pairs interleaved)
                    pc.seg_of_pair.push_back(int32_t(g));
                    pc.group.push_back(mix == 0 ? uint8_t(m % 2u) : mix == 1 ? uint8_t(g % 2u ? IOC_SPLIT_NONE : 1) : uint8_t("\0\1\377"[rng() % 3u]));
                }
            if (!check_pile(pc, rng)) return 1;
        }
    if (!check_pile(PileCase{}, rng) || !check_pile(PileCase{{5, 0}, {}, {}}, rng)) return 1;
    printf("ok: %ld drives of k_ops_project_ins' walk (%ld runs over a step's edge, %ld on its first byte, %ld on its last), %ld work items of k_plane_pile over %ld members\n",
           g_strings, g_run_over_edge, g_first, g_last, g_items, g_members);
    return 0;
}
