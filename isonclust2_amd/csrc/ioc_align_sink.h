// ioc_align_sink.h — where the batched aligner's walks leave their operation bytes: the caller's side of an emitting call
// (ioc_align_gpu.hip runs it, ioc_align_sinks.cpp's entry points describe it).  Host code only, and no HIP header: the device
// tables are plain pointers here, and tools/align_sink_check.cpp drives everything below on the CPU.
#ifndef IOC_ALIGN_SINK_H
#define IOC_ALIGN_SINK_H

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "isonclust2_hip.h"

#pragma GCC visibility push(hidden)  // (internal to the library: none of this is part of its exported symbols)

// what a call's IOC_TRACE line reports; owned by the entry point, added to by every run — the call's own, the re-runs'
struct AlnTally {
    double ms_copy = 0;    // what the copies from the device took the host, and ...
    int64_t copied = 0;    // ... how many bytes they were
    double ms_stats = 0;   // k_ops_stats' device time, and ...
    int64_t records = 0;   // ... how many records came back
    double ms_pileup = 0;  // k_ops_pileup's device time
    double ms_call = 0;    // k_pile_call's device time (the polish path)
    double ms_project = 0; // k_ops_project's device time (a pile that projects), ...
    double ms_sites = 0;   // ... k_pile_sites' and ...
    double ms_alleles = 0; // ... k_site_alleles' (ioc_align_pairs_alleles)
    double ms_project_ins = 0;  // k_ops_project_ins' device time (a pile that projects what the pairs insert as well), and ...
    double ms_plane_pile = 0;   // ... k_plane_pile's (ioc_planes_polish, ioc_align_pairs_split_polish)
    double ms_group_pile = 0;   // k_group_pile's device time (ioc_planes_polish_groups, ioc_align_pairs_blocks_polish)
    double ms_project_weights = 0;      // k_ops_project_weights' device time (a pile that projects the weights of the votes as well), and ...
    double ms_group_pile_weighted = 0;  // ... k_group_pile_weighted's (ioc_planes_polish_groups_weighted, ioc_align_pairs_blocks_polish_weighted)
    double ms_correct = 0;      // k_read_correct's device time, both passes and the scan (ioc_planes_correct, ioc_align_pairs_correct)
    double ms_iso_correct = 0;  // k_iso_correct_count with the scan and k_iso_correct_emit (ioc_planes_correct_groups, ioc_align_pairs_blocks_correct)
    double ms_blocks = 0;       // the eight kernels of ioc_read_blocks.hip, their device time together (ioc_planes_blocks, ioc_align_pairs_blocks)
    double ms_project_ilen = 0; // k_ops_project_ilen's device time (a pile that projects the length plane as well), and ...
    double ms_inserts[8] = {};  // ... the eight kernels of ioc_read_inserts.hip, in the order they run (ioc_planes_inserts, ioc_align_pairs_blocks_inserts)
    double ms_project_qpos = 0; // k_ops_project_qpos' device time (a pile that projects the position plane as well), and ...
    double ms_win_walk = 0;     // (IOC_WIN_SPLIT: k_win_align's walk on its own; ms_windows[2] is the fill then)
    double ms_windows[4] = {};  // ... k_win_bounds, k_win_template, k_win_align and k_group_pile over the sites (ioc_planes_insert_windows, ioc_align_pairs_blocks_inserts_seq)
    double ms_winvar[8] = {};   // k_win_agree (both rounds), k_win_template_far, k_win_align over round B, then k_win_decide, k_win_rekey and the three of the
                                // recount, in the order they run (ioc_planes_insert_window_variants); ms_windows[2] is round A then, ms_windows[3] the slots' pile
    int64_t win_voters = 0, win_voters_b = 0;  // ... the alignments of round A, and those of round B
    double ms_splice[3] = {};   // k_splice_plan, k_splice_call's count pass with the scan, and its write pass (ioc_planes_isoforms_full,
                                // ioc_align_pairs_isoforms_full, where ms_group_pile is k_group_pile over the combined isoforms)
    double ms_ends[8] = {};     // the eight kernels of ioc_read_ends.hip, in the order they run (ioc_reads_ends, ioc_align_pairs_blocks_ends)
    double ms_split[9] = {};     // the split's kernels, in the order of IocSplitStep (timed under IOC_TRACE only), and ...
    int64_t split_uploaded = 0;  // ... what the split uploaded (ioc_alleles_split, ioc_align_pairs_split)
};

// ---- which kernel family a pair takes, by its scoring parameters (ioc_host_align_route; prepare_pairs asks nothing else) ----
// The forward passes add cm = match + gap_extend + gap_open on a diagonal step over equal bases, cx = mismatch + gap_extend +
// gap_open over different ones, and subtract gd = gap_open - gap_extend where a gap may open (fwd_cells, ioc_align_gpu.hip).
constexpr int ALN_V2_GUARD = 28000;     // version 2: |value - 32768| a rebase accepts
constexpr int ALN_V2_STRIP_COLS = 1024;  // ... the columns of a tile, whose top row is cut to 16 bits around its first column
constexpr int ALN_V2_ROWS_PER_CHECK = 64;  // ... and the rows a lane runs between two rebases (16 steps of 4 rows)
constexpr int ALN_V2_RISE_MOST = 32767 / ALN_V2_STRIP_COLS;  // 31
static_assert(ALN_V2_RISE_MOST * ALN_V2_ROWS_PER_CHECK <= 65535 - (32768 + ALN_V2_GUARD), "64 rows' rise fits above the guard");
enum : int { ALN_ROUTE_COMPARE = 0, ALN_ROUTE_PROFILE = 1, ALN_ROUTE_V2 = 2 };

// the query-profile kernels hold cm and cx as bytes (32-bit cells: version 1's profile form; version 2)
inline bool aln_profile_ok(int64_t match, int64_t mismatch, int64_t gap_extend, int64_t gap_open)
{
    const int64_t cm = match + gap_extend + gap_open, cx = mismatch + gap_extend + gap_open;
    return cm >= 0 && cm <= 255 && cx >= 0 && cx <= 255;
}

// Version 2's 16-bit halves on top of that.  gd goes into a half as an unsigned number and is subtracted with one 32-bit
// operation for both halves: it must not be negative.  And a slanted score rises by at most max(cm, cx) per column along a row
// and per row down a column, which the window has to survive where nothing looks at it: the top row of a tile is cut to 16 bits
// around its first column before a lane's first rebase (1024 columns' rise must stay inside a half: max(cm, cx) <= 31), and a
// value the guard accepted runs 64 rows until the next rebase (64 x 31 is below the 4767 a half has left above the guard).  A
// half that overflows carries into the other pair of the couple, so this is a matter of both pairs' results.
inline bool aln_v2_ok(int64_t match, int64_t mismatch, int64_t gap_extend, int64_t gap_open)
{
    const int64_t rise = (match > mismatch ? match : mismatch) + gap_extend + gap_open;
    return aln_profile_ok(match, mismatch, gap_extend, gap_open) && gap_open - gap_extend >= 0 && rise <= ALN_V2_RISE_MOST;
}

inline int aln_route(int64_t match, int64_t mismatch, int64_t gap_extend, int64_t gap_open)
{
    return aln_v2_ok(match, mismatch, gap_extend, gap_open)        ? ALN_ROUTE_V2
           : aln_profile_ok(match, mismatch, gap_extend, gap_open) ? ALN_ROUTE_PROFILE
                                                                    : ALN_ROUTE_COMPARE;
}

// What the 32-bit kernels can hold at all (isonclust2_hip.h states it next to ioc_align_pairs).  A score lies within
// max(|match|, |mismatch|) x min(n, m) of 0 and its slanted form within gap_extend x (n + m) of that: under the bound below
// both stay inside 2^29, the kernels' "no score" (ALN_NEG), and the sum of two of them inside an int.
constexpr int64_t ALN_PARAM_MOST = int64_t(1) << 24;
constexpr int64_t ALN_SPAN_MOST = int64_t(1) << 30;
inline int64_t aln_param_weight(int64_t match, int64_t mismatch, int64_t gap_extend)
{
    const int64_t a = match < 0 ? -match : match, b = mismatch < 0 ? -mismatch : mismatch;
    return (a > b ? a : b) + 2 * gap_extend + 5;  // (5: the largest gap_open, ioc_host_gap_open)
}
inline bool aln_params_ok(int64_t match, int64_t mismatch, int64_t gap_extend)
{
    return gap_extend >= 0 && aln_param_weight(match, mismatch, gap_extend) <= ALN_PARAM_MOST;
}
inline bool aln_span_ok(int64_t match, int64_t mismatch, int64_t gap_extend, int64_t n, int64_t m)
{
    return aln_param_weight(match, mismatch, gap_extend) * (n + m) <= ALN_SPAN_MOST;
}

enum class SinkKind { bytes, reduced };               // the bytes go to the host / stay on the device and are reduced there
enum class PileKind { none, counts, ins, weighted };  // the variant of k_ops_pileup a reduced sink runs

// The per-slice table of a run in front of the slice's bytes (ops_reserve): a column per device pair each, np pairs.  The offsets
// do not depend on the kind; the kind says how many of the columns there are.
struct OpsLayout {
    size_t end;       // uint64: one past the last byte of the pair's region
    size_t len;       // uint32: bytes written
    size_t room;      // uint32: query length + reference length (a reduced sink)
    size_t row_base;  // int64: first row, -1 for a pair that has been added already (a pile)
    size_t q_off;     // uint32: where the query starts in the pool (a pile)
    size_t q_len;     // uint32: the query's length (a weighted pile, a pile that projects the weights: a projecting table has the column)
    size_t plane;     // uint64: where the pair's planes start (a pile that projects)
    size_t bytes;     // the slice's bytes: the table, rounded up to 16
    size_t spare;     // behind the bytes: k_ops_stats and k_ops_pileup read the dword that holds a string's last byte whole
};
inline OpsLayout ops_layout(size_t np, SinkKind kind, PileKind pile, bool project = false)
{
    const bool reduced = kind == SinkKind::reduced;
    const size_t per_pair = !reduced ? 12 : pile == PileKind::none ? 16 : project ? 40 : pile == PileKind::weighted ? 32 : 28;
    return OpsLayout{0, np * 8, np * 12, np * 16, np * 24, np * 28, np * 32, (np * per_pair + 15) & ~size_t(15), reduced ? size_t(4) : size_t(0)};
}

struct AlnSubSink;

// The caller's side, indexed by the caller's pair.  len[i]: the length written for pair i, whatever the kind (0: no answer yet).
struct AlnSink {
    SinkKind kind = SinkKind::bytes;
    int64_t* len = nullptr;
    AlnTally* tally = nullptr;
    // bytes: pair i's go to buf + base[i] (room: query length + reference length), in forward order; ioc_align_pairs_ops packs them
    // when the call is over
    struct Bytes {
        uint8_t* buf = nullptr;
        const int64_t* base = nullptr;
    } bytes;
    // reduced, optional (with_stats): pair i's record goes to stats[i]
    bool with_stats = false;
    ioc_aln_stats* stats = nullptr;
    // reduced, optional: pair i's alignment is added to the rows from row_base[i] on of the call's tables on the device, ONCE:
    // piled[i] says that it has been, whichever run did it
    struct Pile {
        PileKind kind = PileKind::none;
        ioc_pileup_col* cols = nullptr;   // (device) counts: every kind
        ioc_pileup_ins* ins = nullptr;    // (device) ins: what the pairs insert
        ioc_pileup_col* wcols = nullptr;  // (device) weighted: the sums of weights, and ...
        ioc_pileup_ins* wins = nullptr;   // (device) ... those of what the pairs insert
        int64_t rows = 0;                 // records per table
        const int64_t* row_base = nullptr;
        uint8_t* piled = nullptr;
        // optional, with any kind (project): pair i's alignment is projected as well (k_ops_project), by the run that piles it,
        // into reference length + 1 bytes of each of the two planes from byte plane[i] on
        bool project = false;
        uint8_t* base_planes = nullptr;  // (device) what the pair says at every row, IOC_ALLELE_NONE where nothing, and ...
        uint8_t* ins_planes = nullptr;   // (device) ... whether it inserts in front of it
        int64_t plane_bytes = 0;         // bytes per plane
        const int64_t* plane = nullptr;
        // optional, with project (project_ins): what the pair inserts is projected too (k_ops_project_ins), into reference length + 1
        // bytes of each of IOC_PILE_INS_SLOTS more planes, one behind the other, from byte plane[i] of each on
        bool project_ins = false;
        uint8_t* slot_planes = nullptr;  // (device) [all slot-0 planes] .. [all slot-5 planes], plane_bytes each
        // optional, with project_ins (project_weights): the weight of every vote of the pair is projected too (k_ops_project_weights),
        // under the pool's quality bytes, into reference length + 1 bytes of each of 1 + IOC_PILE_INS_SLOTS more planes
        bool project_weights = false;
        uint8_t* weight_planes = nullptr;  // (device) [wbase plane][all wslot-0 planes] .. [all wslot-5 planes], plane_bytes each
        // optional, with project (project_ilen): how many bases the pair inserts in front of every row is projected too
        // (k_ops_project_ilen), into reference length + 1 bytes of one more plane from byte plane[i] on
        bool project_ilen = false;
        uint8_t* ilen_planes = nullptr;  // (device) plane_bytes
        // optional, with project (project_qpos): where every row lies in the pair's query is projected too (k_ops_project_qpos),
        // into reference length + 1 words of a plane of 32-bit words from word plane[i] on
        bool project_qpos = false;
        uint32_t* qpos_planes = nullptr;  // (device) plane_bytes words
    } pile;

    bool reduced() const { return kind == SinkKind::reduced; }
    bool has_stats() const { return reduced() && with_stats; }
    bool has_pile() const { return reduced() && pile.kind != PileKind::none; }
    bool projects() const { return has_pile() && pile.project; }
    bool projects_ins() const { return projects() && pile.project_ins; }
    bool projects_weights() const { return projects_ins() && pile.project_weights; }
    bool projects_ilen() const { return projects() && pile.project_ilen; }
    bool projects_qpos() const { return projects() && pile.project_qpos; }
    uint64_t planes() const  // (in bytes per row and pair: a position plane counts four)
    {
        const uint64_t ilen = (pile.project && pile.project_ilen ? 1 : 0) + (pile.project && pile.project_qpos ? 4 : 0);
        return ilen + (!pile.project ? 0 : !pile.project_ins ? 2 : 2 + uint64_t(IOC_PILE_INS_SLOTS) + (pile.project_weights ? 1 + uint64_t(IOC_PILE_INS_SLOTS) : 0));
    }
    // what the tables hold of the device for the whole call (ck_budget's `held`)
    uint64_t pile_bytes() const
    {
        if (!has_pile()) return 0;
        const uint64_t per_row = pile.kind == PileKind::counts ? sizeof(ioc_pileup_col)
                                 : pile.kind == PileKind::ins  ? sizeof(ioc_pileup_col) + sizeof(ioc_pileup_ins)
                                                               : 2 * sizeof(ioc_pileup_col) + sizeof(ioc_pileup_ins);
        return uint64_t(pile.rows) * per_row + planes() * uint64_t(pile.plane_bytes);
    }
    OpsLayout layout(size_t np) const { return ops_layout(np, kind, reduced() ? pile.kind : PileKind::none, projects()); }

    // Pair i has an empty sequence (query length n, reference length m, one of them 0): all of it is one free end gap, and no walk —
    // n + m bytes 'i' or 'd', a record that is all lead_i or lead_d, nothing for a pile.
    void answer_empty(size_t i, int64_t n, int64_t m) const
    {
        const int64_t l = n + m;
        if (!reduced()) memset(bytes.buf + bytes.base[i], n ? 'i' : 'd', size_t(l));
        if (has_stats()) {
            ioc_aln_stats& s = stats[i];
            s = ioc_aln_stats{};
            s.length = int32_t(l);
            (n ? s.lead_i : s.lead_d) = int32_t(l);
        }
        len[i] = l;
    }

    // A re-run of the caller's pairs idx: the sink of pair x of the re-run is that of the caller's pair idx[x].  The bytes go straight
    // to the caller's regions and the tables are the call's own; lengths, records and `piled` are the re-run's until take_back.
    AlnSubSink subset(const std::vector<int32_t>& idx) const;
    // ... and what the re-run left, into the caller's arrays: every pair of idx gets the re-run's length and record (nothing, if the
    // re-run had no answer either) and keeps `piled` if it was or has now been added
    void take_back(const std::vector<int32_t>& idx, const AlnSubSink& sub) const;
};

struct AlnSubSink {
    AlnSink sink;
    std::vector<int64_t> len, base, row_base, plane;
    std::vector<ioc_aln_stats> stats;
    std::vector<uint8_t> piled;
    AlnSubSink() = default;
    AlnSubSink(AlnSubSink&&) = default;  // (a moved vector keeps its block: sink's pointers stay good; there is no copy)
};

inline AlnSubSink AlnSink::subset(const std::vector<int32_t>& idx) const
{
    AlnSubSink s;
    s.sink = *this;
    s.len.assign(idx.size(), 0);
    s.sink.len = s.len.data();
    if (!reduced()) {
        for (int32_t i : idx) s.base.push_back(bytes.base[i]);
        s.sink.bytes.base = s.base.data();
    }
    if (has_stats()) {
        s.stats = std::vector<ioc_aln_stats>(idx.size(), ioc_aln_stats{});
        s.sink.stats = s.stats.data();
    }
    if (has_pile()) {
        for (int32_t i : idx) s.row_base.push_back(pile.row_base[i]), s.piled.push_back(pile.piled[i]);
        s.sink.pile.row_base = s.row_base.data();
        s.sink.pile.piled = s.piled.data();
    }
    if (projects()) {
        for (int32_t i : idx) s.plane.push_back(pile.plane[i]);
        s.sink.pile.plane = s.plane.data();
    }
    return s;
}

inline void AlnSink::take_back(const std::vector<int32_t>& idx, const AlnSubSink& sub) const
{
    for (size_t x = 0; x < idx.size(); ++x) {
        len[idx[x]] = sub.len[x];
        if (has_stats()) stats[idx[x]] = sub.stats[x];
        if (has_pile()) pile.piled[idx[x]] = sub.piled[x];
    }
}

#pragma GCC visibility pop

#endif
